"""Register / LDS budgets of the eight-wave list-major kernel at sixteen sub-quantizers (csrc/wg8scan.hip.h, wg8_m16_scan_kernel<NQ, DS>:
m = 16, d = 128 and 64), read from the code object inside the built library with the helpers of tests/test_resources.py.  Sixteen waves
per CU need <= 128 VGPRs; a step holds 16-byte code sets and their rotated copies -- with four points per lane sixteen registers more than
at m = 8 -- and none of them may be spilled inside the scan loop: the block with the step's table gathers stays free of scratch accesses.
The four-query form scans 256 points per step (four per lane, sixteen lookups each: 64 gathers); the eight-query form did not fit 128
registers that way and scans 128 (two per lane: 32 gathers).  The kernels own the whole LDS allocation (absolute addresses): no static LDS.  And the m = 8 kernels are
looked up by name fragments that must keep finding them alone.  No GPU needed."""
import os

import pytest

from test_resources import LLVM, _kernel_blocks, _kernel_resources

FORMS = {4: "ds_read_b64", 8: "ds_read_b128"}        # queries per code stream -> the gather of a table entry
STEP_GATHERS = {4: 64, 8: 32}                        # ... -> gathers of a step: sixteen lookups x points per lane (4, 2)
WIDTHS = (4, 8)                                      # d = 64, 128
OTHERS = ("wg8_scan_kernel", "wg8_wide_scan_kernel")


def _frag(nq, ds):
    return "wg8_m16_scan_kernelILi%dELi%dEE" % (nq, ds)


@pytest.fixture(scope="module")
def so(native):
    import ivfadc_jl_amd as pkg
    path = os.path.join(os.path.dirname(pkg._native.__file__), "csrc", "libivfadc_hip.so")
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(path)):
        pytest.skip("LLVM tools or the built library are not available")
    return path


def test_m16_kernels_budgets(so):
    res = {k: v for k, v in _kernel_resources(so).items() if not k.endswith(".kd")}
    m16 = {k: v for k, v in res.items() if "wg8_m16_scan_kernel" in k}
    assert len(m16) == len(FORMS) * len(WIDTHS), sorted(m16)
    for nq in FORMS:
        for ds in WIDTHS:
            hits = {k: v for k, v in m16.items() if _frag(nq, ds) in k}
            assert len(hits) == 1, "wg8_m16_scan_kernel<%d, %d>: %r" % (nq, ds, sorted(hits))
            (name, r), = hits.items()
            assert r.get("vgpr_count", 0) <= 128, "%s uses %d VGPRs (budget 128)" % (name, r.get("vgpr_count", 0))
            assert r.get("group_segment_fixed_size", 0) == 0, "%s carries static LDS" % name
    # what looks the m = 8 kernels up by name finds what it always found: eight narrow, eight wide
    for name in m16:
        assert not any(f in name for f in OTHERS), name
    assert len([k for k in res if "wg8_scan_kernel" in k]) == 8
    assert len([k for k in res if "wg8_wide_scan_kernel" in k]) == 8


@pytest.mark.parametrize("ds", WIDTHS)
@pytest.mark.parametrize("nq", sorted(FORMS))
def test_m16_kernels_scan_loop(so, nq, ds):
    """ONE block holds the step's gathers -- no more, no fewer -- and it touches no scratch memory."""
    want = STEP_GATHERS[nq]
    hot = [b for b in _kernel_blocks(so, _frag(nq, ds)) if sum(FORMS[nq] in x for x in b) >= want]
    assert len(hot) == 1, "wg8_m16_scan_kernel<%d, %d>: expected ONE block with the step's %d table gathers, found %d" % (nq, ds, want, len(hot))
    assert sum(FORMS[nq] in x for x in hot[0]) == want, "wg8_m16_scan_kernel<%d, %d>: the step's block holds %d gathers, not %d" % (
        nq, ds, sum(FORMS[nq] in x for x in hot[0]), want)
    assert not any("scratch_" in x for x in hot[0]), "the scan loop of wg8_m16_scan_kernel<%d, %d> touches scratch memory" % (nq, ds)
