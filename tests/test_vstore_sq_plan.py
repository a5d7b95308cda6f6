"""tests/c/vstore_sq_plan_check.cpp (its own main) on csrc/vstore_sq_plan.h, built with ASan and UBSan, run as an ordinary child process."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stride_range_and_chunk_addressing_under_the_sanitizers(tmp_path):
    exe = os.path.join(str(tmp_path), "vstore_sq_plan_check")
    subprocess.check_call([shutil.which("g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-ffp-contract=off", os.path.join(ROOT, "tests", "c", "vstore_sq_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"vstore_sq_plan_check ok: (\d+) components consumed once, (\d+) shapes", r.stdout)
    assert m and int(m.group(1)) > 1000000 and int(m.group(2)) > 600, r.stdout[-2000:]
