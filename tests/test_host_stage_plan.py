"""tests/c/host_stage_check.cpp (its own main) on csrc/host_stage.h, built with ASan and UBSan, run as an ordinary child process."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_counts_span_and_compaction_under_the_sanitizers(tmp_path):
    exe = os.path.join(str(tmp_path), "host_stage_check")
    subprocess.check_call([shutil.which("g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "c", "host_stage_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    m = re.search(r"host_stage_check ok: (\d+) cases", r.stdout)
    assert m and int(m.group(1)) > sum(7 ** n for n in range(1, 9)), r.stdout[-2000:]   # every layout, and the other three checks
