"""The large-K search's planner on the CPU, under the sanitizers.

tests/c/selscan_plan_check.cpp is a stand-alone program with its own main: it includes csrc/selscan_plan.h -- the LDS layout of
sel_scan_kernel, the buffer capacity (automatic and forced), the served rule and the sub-batch -- and checks them over a grid of
(d, m, K, forced capacity).  Built with AddressSanitizer and UndefinedBehaviorSanitizer and run as an ordinary child process: nothing is
preloaded, nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_capacity_and_served_rule_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the planner check"
    exe = os.path.join(str(tmp_path), "selscan_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",      # (the runtimes are in the program)
                           os.path.join(ROOT, "tests", "c", "selscan_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"selscan_plan_check ok: (\d+) cases, (\d+) served", r.stdout)
    assert m and int(m.group(1)) >= 10000 and 1000 <= int(m.group(2)) < int(m.group(1)), r.stdout[-2000:]
