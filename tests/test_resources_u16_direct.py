"""Register / scratch / LDS figures of the two table-free entries of the UInt16 list scan (csrc/u16scan.hip.h), read from the code object
inside the built library in the manner of tests/test_resources_u16_wide.py.  u16_direct_scan_kernel (K <= 64) and
u16_direct_wide_scan_kernel (64 < K) share u16_scan_body with the table entries through one more template parameter: both must exist
exactly once, stay free of scratch memory and static LDS, and keep the registers they were built with -- 177 VGPRs (two waves per SIMD,
i.e. two workgroups of four waves per CU; three would need <= 168) and 217 (two waves per SIMD; <= 256).  Their LDS functions must fit
one workgroup's 160 KB at every reach the header documents and fail just beyond it.  The two table entries must still satisfy the
existing test's bounds.  No GPU needed."""
import os
import re

from test_resources_u16_wide import LDS_MAX, SMALL, WIDE, _one, kernels  # noqa: F401  (kernels: the module-scoped fixture)

DIRECT, DIRECT_WIDE = "22u16_direct_scan_kernelE", "27u16_direct_wide_scan_kernelE"


def _src():   # the kernel header and the sizes it includes (scan_layouts.h: shared with the plan)
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ivfadc.jl_amd", "csrc")
    return open(os.path.join(csrc, "u16scan.hip.h")).read() + open(os.path.join(csrc, "scan_layouts.h")).read()


def _no_scratch_no_static_lds(name, r):
    assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, "%s uses scratch memory: %r" % (name, r)
    assert r.get("group_segment_fixed_size", 0) == 0, "%s carries static LDS" % name


def test_direct_entry(kernels):
    name, r = _one(kernels, DIRECT)
    _no_scratch_no_static_lds(name, r)
    assert r["vgpr_count"] <= 177, "%s uses %d VGPRs (177 when it was measured: two waves per SIMD)" % (name, r["vgpr_count"])
    assert 512 // r["vgpr_count"] >= 2


def test_direct_wide_entry(kernels):
    name, r = _one(kernels, DIRECT_WIDE)
    _no_scratch_no_static_lds(name, r)
    assert r["vgpr_count"] <= 217, "%s uses %d VGPRs (217 when it was measured: two waves per SIMD)" % (name, r["vgpr_count"])
    assert 512 // r["vgpr_count"] >= 2


def test_table_entries_are_what_they_were(kernels):
    name, r = _one(kernels, SMALL)
    assert r["vgpr_count"] <= 165, (name, r)
    _no_scratch_no_static_lds(name, r)
    name, r = _one(kernels, WIDE)
    assert r["vgpr_count"] <= 256, (name, r)
    _no_scratch_no_static_lds(name, r)


def test_lds_functions_fit_a_cu_at_the_documented_reach():
    src = _src()
    P = int(re.search(r"constexpr int U16_P = (\d+);", src).group(1))
    assert re.search(r"constexpr int U16_XCH_FLOATS = 4 \* U16_P \* 64 \* 2;", src)
    assert "u16_direct_lds_bytes" in src and "u16_direct_wide_lds_bytes" in src
    xch = 4 * P * 64 * 8                                              # 4 waves x P pairs x 64 keys

    def small(mdsp):
        return P * mdsp * 4 + xch + 4 * P * 4 + 16

    def wide(mdsp, qg, cap):
        return P * mdsp * 4 + 4 * qg * cap * 8 + 4 * P * 4 + 16

    assert xch == 16384 and small(32) == 8 * 32 * 4 + 16384 + 144
    # K <= 64: 32 m dsp + 16 528 B <= 160 KB, i.e. m dsp <= 4600 (the table form: 4088)
    assert small(4600) <= LDS_MAX < small(4604)
    # 64 < K: m dsp + qg cap <= 5115
    for mdsp, k in ((3064, 1984), (4088, 960), (4600, 448), (4856, 192)):
        cap = max(128, 1 << (k + 64 - 1).bit_length())
        assert cap == k + 64
        assert wide(mdsp, 1, cap) <= LDS_MAX < wide(mdsp + 4, 1, cap), (mdsp, k)
        assert wide(mdsp, 1, 2 * cap) > LDS_MAX                      # K + 1 doubles cap
        assert (mdsp + cap <= 5115) and (mdsp + 4 + cap > 5115)
    assert wide(4, 1, 8192) > LDS_MAX and wide(1016, 1, 4096) <= LDS_MAX < wide(1020, 1, 4096)
    assert wide(128, 8, 512) <= LDS_MAX and wide(128, 1, 2048) <= LDS_MAX   # d = 128 / m = 8: K <= 448 at qg = 8, K <= 1984 at qg = 1
    for frag in ("m dsp + qg cap <= 5115", "K <= 1984 where m dsp <= 3064", "K <= 960 up to 4088", "K <= 448 up to 4600", "K <= 192 up to 4856", "cap = 4096 fits where m dsp <= 1016"):
        assert frag in src, frag
