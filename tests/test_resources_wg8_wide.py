"""Register / LDS budgets of the eight-wave list-major kernel's wide-pool form (csrc/wg8scan.hip.h, wg8_wide_scan_kernel<NQ, DS>: K <= 128),
read from the code object inside the built library with the helpers of tests/test_resources.py.  Sixteen waves per CU need <= 128 VGPRs;
the wide pool's second snapshot register pair lives in the cold paths (offers, hand-over) and must not reach the scan loop -- the block
with the step's 32 table gathers stays free of scratch accesses, as the narrow kernels' does.  The kernels own the whole LDS allocation
(absolute addresses): no static LDS.  And the narrow kernels are looked up by name fragments that must keep finding them alone.  No GPU
needed."""
import os

import pytest

from test_resources import LLVM, _kernel_blocks, _kernel_resources

FORMS = {4: "ds_read_b64", 8: "ds_read_b128"}        # queries per code stream -> the gather of a table entry
WIDTHS = (4, 8, 12, 16)
NARROW = ("wg8_scan_kernelILi4EE", "wg8_scan_kernelILi8EE")


def _frag(nq, ds):
    return "wg8_wide_scan_kernelILi%dELi%dEE" % (nq, ds)


@pytest.fixture(scope="module")
def so(native):
    import ivfadc_jl_amd as pkg
    path = os.path.join(os.path.dirname(pkg._native.__file__), "csrc", "libivfadc_hip.so")
    if not (os.path.exists(os.path.join(LLVM, "llvm-readelf")) and os.path.exists(path)):
        pytest.skip("LLVM tools or the built library are not available")
    return path


def test_wide_pool_kernels_budgets(so):
    res = {k: v for k, v in _kernel_resources(so).items() if not k.endswith(".kd")}
    wide = {k: v for k, v in res.items() if "wg8_wide_scan_kernel" in k}
    assert len(wide) == len(FORMS) * len(WIDTHS), sorted(wide)
    for nq in FORMS:
        for ds in WIDTHS:
            hits = {k: v for k, v in wide.items() if _frag(nq, ds) in k}
            assert len(hits) == 1, "wg8_wide_scan_kernel<%d, %d>: %r" % (nq, ds, sorted(hits))
            (name, r), = hits.items()
            assert r.get("vgpr_count", 0) <= 128, "%s uses %d VGPRs (budget 128)" % (name, r.get("vgpr_count", 0))
            assert r.get("group_segment_fixed_size", 0) == 0, "%s carries static LDS" % name
    # what tests/test_resources.py looks the narrow kernels up by finds them alone
    for name in wide:
        assert not any(f in name for f in NARROW), name
    for f in NARROW:
        assert len([k for k in res if f in k]) == 1, f


@pytest.mark.parametrize("ds", WIDTHS)
@pytest.mark.parametrize("nq", sorted(FORMS))
def test_wide_pool_kernels_scan_loop(so, nq, ds):
    """ONE block holds the step's 32 gathers, and it touches no scratch memory."""
    hot = [b for b in _kernel_blocks(so, _frag(nq, ds)) if sum(FORMS[nq] in x for x in b) >= 32]
    assert len(hot) == 1, "wg8_wide_scan_kernel<%d, %d>: expected ONE block with the step's 32 table gathers, found %d" % (nq, ds, len(hot))
    assert not any("scratch_" in x for x in hot[0]), "the scan loop of wg8_wide_scan_kernel<%d, %d> touches scratch memory" % (nq, ds)
