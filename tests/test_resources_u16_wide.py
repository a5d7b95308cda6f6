"""Register / scratch / LDS figures of the two entries of the UInt16 list scan (csrc/u16scan.hip.h), read from the code object inside the
built library in the manner of tests/test_resources.py.  u16_scan_kernel (K <= 64, the kernel every 16-bit handle runs by default) shares
its body with u16_wide_scan_kernel (64 < K, table mode 10) through a template: it must keep its three waves per SIMD (165 VGPRs before the
template) and stay free of scratch memory.  The wide entry must exist, own its whole LDS allocation dynamically, and fit one workgroup's
160 KB at every reach the header documents.  No GPU needed."""
import os
import re
import subprocess
import tempfile

import pytest

from test_resources import LLVM

SMALL, WIDE = "15u16_scan_kernelE", "20u16_wide_scan_kernelE"
LDS_MAX = 160 << 10
KEYS = "name|vgpr_count|sgpr_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size"


@pytest.fixture(scope="module")
def kernels(native):
    import ivfadc_jl_amd as pkg
    so = os.path.join(os.path.dirname(pkg._native.__file__), "csrc", "libivfadc_hip.so")
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(so)):
        pytest.skip("LLVM tools or the built library are not available")
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, so])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    res, cur = {}, None
    for line in notes.splitlines():
        if re.match(r"^  - \.\w+:", line):
            cur = {}
            line = "    " + line[4:]
        if cur is None:
            continue
        m = re.match(r"^    \.(%s):\s+(\S+)" % KEYS, line)
        if m and m.group(1) == "name":
            res[m.group(2)] = cur
        elif m:
            cur[m.group(1)] = int(m.group(2))
    return res


def _one(kernels, frag):
    hits = {k: v for k, v in kernels.items() if frag in k and not k.endswith(".kd")}
    assert len(hits) == 1, "%s: %r" % (frag, sorted(hits))
    return next(iter(hits.items()))


def test_small_entry_keeps_its_registers(kernels):
    name, r = _one(kernels, SMALL)
    assert r["vgpr_count"] <= 165, "%s uses %d VGPRs (165 before the template: three waves per SIMD)" % (name, r["vgpr_count"])
    assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, "%s uses scratch memory: %r" % (name, r)
    assert r.get("group_segment_fixed_size", 0) == 0, "%s carries static LDS" % name


def test_wide_entry_compiles_and_fits_a_cu(kernels):
    name, r = _one(kernels, WIDE)
    assert r["vgpr_count"] <= 256 and r.get("vgpr_spill_count", 0) == 0, "%s: %r (two waves per SIMD need <= 256 VGPRs)" % (name, r)
    assert r.get("group_segment_fixed_size", 0) == 0, "%s carries static LDS" % name
    # u16_wide_lds_bytes with the constants of the source, at the reaches the header documents: m dsp + qg cap <= 4091
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ivfadc.jl_amd", "csrc", "scan_layouts.h")).read()   # (u16scan.hip.h includes it)
    P = int(re.search(r"constexpr int U16_P = (\d+);", src).group(1))
    TF = int(re.search(r"constexpr int U16_TAB_FLOATS = (\d+);", src).group(1))

    def lds(mdsp, qg, cap):
        return P * mdsp * 4 + TF * 4 + 4 * P * 4 + 16 + 4 * qg * cap * 8

    for mdsp, k in ((2040, 1984), (3064, 960), (3576, 448), (3832, 192)):
        cap = max(128, 1 << (k + 64 - 1).bit_length())
        assert cap == k + 64
        assert lds(mdsp, 1, cap) <= LDS_MAX < lds(mdsp + 4, 1, cap), (mdsp, k)
        assert lds(mdsp, 1, 2 * cap) > LDS_MAX                    # K + 1 doubles cap
        assert (mdsp + cap <= 4091) and (mdsp + 4 + cap > 4091)
    assert lds(4, 1, 4096) > LDS_MAX                              # cap = 4096 (K >= 1985) never fits
    assert lds(128, 8, 256) <= LDS_MAX and lds(128, 1, 2048) <= LDS_MAX   # d = 128 / m = 8: K <= 192 at qg = 8, K <= 1984 at qg = 1
