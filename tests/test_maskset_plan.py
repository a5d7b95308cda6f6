"""The mask-set layout, its bit addressing and the masked search's planner, on the CPU under the sanitizers.

tests/c/maskset_plan_check.cpp is a stand-alone program with its own main: it includes csrc/maskset_plan.h (the layout and the one
definition of "word and bit of position p" that the build kernel, the scan kernel and the generic path share), csrc/subset_plan.h (the
work items and the bit test the build kernel reuses) and csrc/plan.h (make_plan_masked), restates the build lane by lane in plain C++ and
reads it back bit by bit for every position of the case-table lengths, runs the planner over the grid of tests/c/plan_grid.h, and replays
tests/plan_table.tsv to show that make_plan / make_plan_u16 still decide what they decided.  Built with AddressSanitizer and
UndefinedBehaviorSanitizer and run as an ordinary child process: nothing is preloaded, nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import masked as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivfadc.jl_amd", "csrc")
TABLE = os.path.join(ROOT, "tests", "plan_table.tsv")


def test_layout_bits_and_planner_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the mask-set check"
    exe = os.path.join(str(tmp_path), "maskset_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",      # (the runtimes are in the program)
                           os.path.join(ROOT, "tests", "c", "maskset_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe, TABLE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-4000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    rows = sum(1 for _ in open(TABLE)) - 1
    m = re.search(r"maskset_plan_check ok: (\d+) lengths, (\d+) grid cases, (\d+) table rows", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) == 2 * len(mk.LENS) and int(m.group(2)) > 100000 and int(m.group(3)) == rows >= 200


def test_case_table_lengths_are_the_programs():
    src = open(os.path.join(ROOT, "tests", "c", "maskset_plan_check.cpp")).read()
    m = re.search(r"CASE_LENS\[\] = \{([^}]*)\}", src)
    assert m and tuple(int(x) for x in m.group(1).split(",")) == mk.LENS


def test_headers_are_plain_cpp_and_shared_with_the_kernels():
    """maskset_plan.h names no HIP type; maskset.hip.h takes the layout and the bit test from the plan headers instead of restating them,
    calls the four-wave kernel's shared pieces, and holds neither inline assembly nor atomics other than the kept counts'; plan.h appends
    the new form LAST, so the integers tests/plan_table.tsv prints do not move."""
    plan = open(os.path.join(CSRC, "maskset_plan.h")).read()
    for word in ("hip/hip_runtime", "hipStream", "__global__"):
        assert word not in plan, word
    kern = open(os.path.join(CSRC, "maskset.hip.h")).read()
    body = kern.split("#pragma once")[1]
    assert '#include "maskset_plan.h"' in kern and '#include "subset_plan.h"' in kern
    assert kern.count("subset::subset_selected(") == 1, "the bit test is subset_plan.h's, called once"
    for shared in ("build_residuals<QG>(", "build_tables_t<QG, 0, TAB_INTERLEAVED>(", "WSel<SMALL>", "publish_bound<QG>(", "merge_waves(", "scan_emit<",
                   "carve_lds<QG, SMALL>(", "maskset::round_word(", "maskset::row_start("):
        assert shared in body, shared
    assert "asm" not in body and ">> 5" not in body and "& 31" not in body
    assert re.search(r"enum class ScanForm \{[^}]*U16DirectWide, Masked \};", open(os.path.join(CSRC, "plan.h")).read())
    gen = open(os.path.join(CSRC, "generic.hip.h")).read()
    assert gen.count("maskset::slot_selected(") == 2 and "KEY_MAX" in gen
