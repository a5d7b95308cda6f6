"""The masked range search's plan facts and mask-word addressing, on the CPU under the sanitizers.

tests/c/range_masked_plan_check.cpp is a stand-alone program with its own main: it includes csrc/range_plan.h and csrc/maskset_plan.h and
checks the table-free LDS need and chunk, the invariant "every chunk begins on a round of 64" over the case table's lengths and forced
chunks of 64, 256 and 1024, the mask words of every item of every list through maskset::round_word (inside the list's row, every selected
position exactly once in the count and in the fill pass, nothing at or behind list_len), and per_query_bytes.  Built with AddressSanitizer
and UndefinedBehaviorSanitizer, the runtimes linked statically into the program, and run as an ordinary child process: nothing is
preloaded, nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import masked as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivfadc.jl_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "range_masked_plan_check.cpp")


def test_plan_facts_and_mask_words_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the masked range plan check"
    exe = os.path.join(str(tmp_path), "range_masked_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"range_masked_plan_check ok: (\d+) shapes, (\d+) chunk begins, (\d+) items over (\d+) lengths, (\d+) points, (\d+) empty rounds",
                  r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) >= 100 and int(m.group(2)) > 100 and int(m.group(3)) > 500 and int(m.group(4)) == len(mk.LENS)
    assert int(m.group(5)) > 10000 and int(m.group(6)) > 0, "some rounds of the table have no selected lane: the skip is exercised"


def test_case_table_lengths_are_the_programs():
    src = open(SRC).read()
    m = re.search(r"CASE_LENS\[\] = \{([^}]*)\}", src)
    assert m and tuple(int(x) for x in m.group(1).split(",")) == mk.LENS


def test_headers_state_the_invariant_and_the_unmeasured_default():
    plan = open(os.path.join(CSRC, "range_plan.h")).read()
    assert "INVARIANT" in plan and "chunk_is_round_aligned" in plan and "TABLE_FREE_CHUNK = 1024" in plan
    assert plan.count("REASONED, NOT MEASURED") == 2, "both default chunks say that they are reasoned, not measured"
    for word in ("hip/hip_runtime", "hipStream", "__global__"):
        assert word not in plan, word
    kern = open(os.path.join(CSRC, "range.hip.h")).read()
    assert kern.count("template <bool FILL, bool U16, bool MASKED>") == 1, "one body, six instantiations"
    for name in ("range_masked_count_kernel", "range_masked_fill_kernel", "range_u16_count_kernel", "range_u16_fill_kernel"):
        assert kern.count("void %s(" % name) == 1, name
    assert "mask_row(" in kern and "mask_round(" in kern and "__ballot(valid)" in kern and "__ballot(alive)" in kern
