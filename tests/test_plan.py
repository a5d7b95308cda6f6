"""The search planner on the CPU, under the sanitizers.

csrc/plan.h decides what every search runs -- the scan kernel, queries per code stream, chunk size, dynamic LDS, sub-batch, coarse stage --
as a pure function of a small struct of facts (PlanFacts), in plain C++ on csrc/scan_layouts.h, which the kernel headers share.
tests/c/plan_check.cpp is a stand-alone program around it: it replays tests/plan_table.tsv -- the decisions of the commit that moved the
planner out of ivfadc_hip.hip, pinned row by row: the BASELINE shapes at bench.py's batch sizes, both sides of every threshold, every
outcome -- and checks over the whole grid of tests/c/plan_grid.h what must hold of any rule (LDS within a CU, 1 <= nb <= nq, at most 64
chunks per list, a form only where its kernels are instantiated, ...).  A row changes only in a pull request that means to change the
plan (DESIGN.md 4.0 says how the table is regenerated)."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivfadc.jl_amd", "csrc")
TABLE = os.path.join(ROOT, "tests", "plan_table.tsv")


def test_pinned_plans_and_invariants_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the planner check"
    exe = os.path.join(str(tmp_path), "plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",      # (the runtimes are in the program)
                           os.path.join(ROOT, "tests", "c", "plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe, TABLE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-4000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    rows = sum(1 for _ in open(TABLE)) - 1
    assert ("plan_check ok: 1205920 grid cases, %d table rows" % rows) in r.stdout, r.stdout[-2000:]
    assert rows >= 200 and os.path.getsize(TABLE) < 100 * 1024


def test_planner_headers_are_plain_cpp_and_shared_with_the_kernels():
    """plan.h and scan_layouts.h name no HIP header or type (they compile with g++ above) and read neither the environment nor the handle;
    the kernel headers take W8Lds, NfLds and the UInt16 sizes from scan_layouts.h instead of restating them, and ivfadc_hip.hip holds no
    planner of its own any more."""
    plan = open(os.path.join(CSRC, "plan.h")).read()
    lay = open(os.path.join(CSRC, "scan_layouts.h")).read()
    for text in (plan, lay):
        for word in ("hip/hip_runtime", "hipStream", "hipError", "__global__", "__device__", "getenv", "fail(", "ivfadc_index"):
            assert word not in text, word
    assert re.findall(r'#include "([^"]+)"', plan) == ["scan_layouts.h"] and not re.findall(r'#include "([^"]+)"', lay)
    for name, gone in (("wg8scan.hip.h", ("struct W8Lds", "W8_NW =", "W8_TAB_BYTES =", "bool w8_ds_ok")),
                       ("nfscan.hip.h", ("struct NfLds", "NF_QG =", "NF_POOL =")),
                       ("u16scan.hip.h", ("U16_P =", "U16_PASS =", "U16_TAB_FLOATS =", "u16_lds_bytes(int", "u16_direct_wide_lds_bytes(int"))):
        kern = open(os.path.join(CSRC, name)).read()
        for word in gone:
            assert word not in kern, (name, word)
    # (kernels.hip.h includes wg8scan.hip.h and nfscan.hip.h inside namespace ivf, so it is the one that includes the layouts for them)
    for name in ("kernels.hip.h", "u16scan.hip.h"):
        assert '#include "scan_layouts.h"' in open(os.path.join(CSRC, name)).read(), name
    assert "struct W8Lds" in lay and "struct NfLds" in lay and "U16_PASS =" in lay
    host = open(os.path.join(CSRC, "ivfadc_hip.hip")).read()
    assert '#include "plan.h"' in host and "PlanFacts plan_facts(const ivfadc_index *h)" in host
    for word in ("struct Plan", "make_plan(ivfadc_index", "make_plan_u16(ivfadc_index", "plan_list_major(", "plan_query_major(", "size_t scan_lds_bytes",
                 "size_t lb_lds_bytes", "LDS_MAX ="):
        assert word not in host, word
    # the plan's LDS figure of the matrix-core rounds is asserted against the kernel's own layout at every instantiation
    assert host.count("static_assert(lb_lds_bytes(M_, D_, P_) == lb_kernel_lds<M_, D_, P_>") == 1
