"""The planner of ivfadc_rerank and the kernels' addressing on the CPU: tests/c/rerank_plan_check.cpp (its own main) restates the slice loop,
rerank_dist_kernel's fetch, tile and chain and rerank_select_kernel's merge network on csrc/rerank_plan.h over small grids and at the
2^31 - 1 edge, built with ASan and UBSan and run as an ordinary child process: nothing is preloaded."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_and_kernel_arithmetic_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the rerank planner check"
    exe = os.path.join(str(tmp_path), "rerank_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "c", "rerank_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"rerank_plan_check ok: (\d+) pairs written once, (\d+) slices", r.stdout)
    assert m and int(m.group(1)) > 1000000 and int(m.group(2)) > 9 * 8 * 3 * 2, r.stdout[-2000:]
