"""The host planner of the subset views and the kernels' index arithmetic, on the CPU under the sanitizers.

tests/c/subset_plan_check.cpp is a stand-alone program: it includes csrc/subset_plan.h -- the work items, the per-list totals and item
bases, subset_point and the bit test the two kernels share -- restates count and scatter lane by lane in plain C++ on top of them, and
compares the outcome with a brute-force filter over the lengths and masks of tests/subset.py at every code stride.  Built with
AddressSanitizer and UndefinedBehaviorSanitizer and run as an ordinary child process: an index that leaves its list, a slot written
twice, a shift of 64 or a word read behind nbits ends it with a report."""
import os
import shutil
import subprocess

import pytest

import subset as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_and_index_arithmetic_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the planner check"
    exe = os.path.join(str(tmp_path), "subset_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",      # (the runtimes are in the program)
                           os.path.join(ROOT, "tests", "c", "subset_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert ("subset_plan_check ok: SUBSET_CHUNK %d, 80 cases" % sb.chunk()) in r.stdout, r.stdout


def test_plan_header_is_plain_cpp_and_shared_with_the_kernels():
    """subset_plan.h names no HIP type (it compiles with g++ above), and subset.hip.h takes the chunk, the point arithmetic and the bit
    test from it instead of restating them."""
    plan = open(sb.PLAN_H).read()
    assert "hip/hip_runtime" not in plan and "hipStream" not in plan and "__global__" not in plan
    kern = open(os.path.join(os.path.dirname(sb.PLAN_H), "subset.hip.h")).read()
    assert '#include "subset_plan.h"' in kern
    assert kern.count("subset::subset_selected(") == 1 and kern.count("subset::subset_point(") == 2
    assert "SUBSET_CHUNK =" not in kern and "atomic" not in kern.split("#pragma once")[1]
