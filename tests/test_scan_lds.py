"""The four-wave scan kernels' LDS layout, on the CPU under the sanitizers.

tests/c/scan_lds_check.cpp is a stand-alone program with its own main: it includes csrc/scan_layouts.h only -- FwLds / FwTail / SqLds, the
byte offsets carve_lds and sq_kernel fill their pointers from and the plan's scan_lds_bytes / sq_lds_bytes / lb_lds_bytes take their ends
from -- sweeps the shapes, widths, capacities and forms, and checks that the regions are ordered, disjoint and aligned, that the short-row
scratch and the parking buffers lie where the kernels use them, and that every end is the figure the plan reported before the layout
existed (the old formulas are kept in the program, verbatim).  It then feeds its own region check two wrong layouts and requires both to
be reported.  Built with AddressSanitizer and UndefinedBehaviorSanitizer and run as an ordinary child process: nothing is preloaded,
nothing is loaded into Python."""
import glob
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ivfadc.jl_amd", "csrc")


def test_regions_ends_and_planted_errors_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed for the scan LDS check"
    exe = os.path.join(str(tmp_path), "scan_lds_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",      # (the runtimes are in the program)
                           os.path.join(ROOT, "tests", "c", "scan_lds_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"scan_lds_check ok: (\d+) layouts, (\d+) sq layouts, (\d+) lb layouts, (\d+) planted errors reported", r.stdout)
    assert m, r.stdout[-2000:]
    shapes = 7 * 6      # every (m, dsub) of the sweep has m dsub <= 1024
    # 3 widths x 6 K x small / list_major / stripe on and off; 3 kc x inside on and off; the eight LB instantiations;
    # the parking buffers based 128 dwords behind the probes at m = 8 and 16, the tail without its round-up at three widths
    assert [int(g) for g in m.groups()] == [shapes * 3 * 6 * 8, shapes * 3 * 2, 8, 2 + 3]


def test_the_layout_is_written_once():
    """scan_layouts.h names no HIP type (it compiles with g++ above, under -Wall -Wextra -Werror); the kernels carve no region by a bare
    number, the host sums none up, and the words per slot of the shared bounds are defined in one place."""
    hdr = open(os.path.join(CSRC, "scan_layouts.h")).read()
    for word in ("hip/hip_runtime", "hipStream", "hipError", "__global__", "__device__", "__shared__", "ivfadc_index"):
        assert word not in hdr, word
    for word in ("struct FwTail", "struct FwLds", "struct SqLds", "struct LbCfg", "constexpr size_t scan_lds_bytes(", "constexpr size_t sq_lds_bytes(",
                 "constexpr size_t lb_lds_bytes("):
        assert hdr.count(word) == 1, word
    for name in ("kernels.hip.h", "smallq.hip.h", "maskset.hip.h"):
        src = open(os.path.join(CSRC, name)).read()
        for word in ("+ 192 +", "s_list + 160", "s_list + 168", "s_list + 170", "(extra_bytes >> 2)"):
            assert word not in src, (name, word)
    kern = open(os.path.join(CSRC, "kernels.hip.h")).read()
    # the carve takes its sizes and the tail's offsets from the header: in carve_lds, in the LB branch of qscan_body, for the probe
    # area and for the parking buffers; sq_kernel takes its own from SqLds
    for word in ("fw_tab_floats(m, QG)", "fw_resid_floats(d, QG)", "fw_selbuf_keys(NSEL, cap)"):
        assert kern.count(word) == 1, word
    assert kern.count("constexpr FwTail T = fw_tail(0, QG);") == 3 and kern.count("constexpr FwTail T = fw_tail(0, PG);") == 1
    assert kern.count("L.scnt = (int *)(smem_raw + C::END);") == 1
    assert "constexpr SqLds S = sq_tail(0, 0);" in open(os.path.join(CSRC, "smallq.hip.h")).read()
    host = open(os.path.join(CSRC, "ivfadc_hip.hip")).read()
    assert not re.search(r"scan_lds_bytes\([^;\n]*\) \+ 64 \+ \(", host) and "+ 64 + (" not in host
    assert "PG * STHR_WORDS * 8 + 768" not in host
    assert host.count("sq_lds_bytes(h->m, h->d, ") == 2
    defs = {os.path.basename(p): open(p).read().count("constexpr int STHR_WORDS") for p in glob.glob(os.path.join(CSRC, "*"))
            if p.endswith((".h", ".hip"))}
    assert {k: v for k, v in defs.items() if v} == {"scan_layouts.h": 1}
