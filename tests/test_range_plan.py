"""The range search's planner and the kernels' index arithmetic, on the CPU under the sanitizers.

tests/c/range_plan_check.cpp is a stand-alone program with its own main: it includes csrc/range_plan.h -- chunk lengths, the (probe,
chunk) items and their positions, the radius test, the LDS need, sub-batches, sort groups and lims -- restates the count pass, the scan
and the fill pass of csrc/range.hip.h lane by lane in plain C++ on top of it, and checks them over the case table's list lengths, a grid
of shapes and SIFT1B-sized counts.  Built with AddressSanitizer and UndefinedBehaviorSanitizer and run as an ordinary child process:
nothing is preloaded, nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import masked as mk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivfadc.jl_amd", "csrc")


def test_planner_and_item_arithmetic_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the range planner check"
    exe = os.path.join(str(tmp_path), "range_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",      # (the runtimes are in the program)
                           os.path.join(ROOT, "tests", "c", "range_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"range_plan_check ok: (\d+) shapes, (\d+) simulated searches over (\d+) lengths, (\d+) points, (\d+) grid cases", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) >= 100 and int(m.group(2)) >= 200 and int(m.group(3)) == len(mk.LENS) and int(m.group(5)) > 5000


def test_case_table_lengths_are_the_programs():
    src = open(os.path.join(ROOT, "tests", "c", "range_plan_check.cpp")).read()
    m = re.search(r"CASE_LENS\[\] = \{([^}]*)\}", src)
    assert m and tuple(int(x) for x in m.group(1).split(",")) == mk.LENS


def test_plan_header_is_plain_cpp_and_shared_with_the_kernels():
    """range_plan.h names no HIP type (it compiles with g++ above) and says that its default chunk is reasoned, not measured; range.hip.h
    and the host runtime take the item arithmetic, the radius test and the plan from it instead of restating them; the kernels hold no
    inline assembly."""
    plan = open(os.path.join(CSRC, "range_plan.h")).read()
    for word in ("hip/hip_runtime", "hipStream", "__global__"):
        assert word not in plan, word
    assert "REASONED, NOT MEASURED" in plan
    kern = open(os.path.join(CSRC, "range.hip.h")).read()
    body = kern.split("#pragma once")[1]
    assert '#include "range_plan.h"' in kern and "NO REFERENCE COUNTERPART" in kern
    for shared in ("range_plan::probe_of(", "range_plan::chunk_of(", "range_plan::chunk_begin(", "range_plan::chunk_end(", "range_plan::radius_live(",
                   "range_plan::radius_bits(", "emit_result("):
        assert shared in body, shared
    assert "asm" not in body and body.count("atomicAdd(s_cnt") == 2, "one LDS atomic per wave and round (fill), one per wave (count)"
    host = open(os.path.join(CSRC, "ivfadc_hip.hip")).read()
    assert "range_plan::make_plan(" in host and "range_plan::next_group(" in host and "range_plan::make_lims(" in host
