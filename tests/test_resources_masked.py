"""Register / scratch / LDS figures of the kernels of the masked search (csrc/maskset.hip.h), read from the code object inside the built
library in the manner of tests/test_resources_subset.py: the six masked_scan_kernel instantiations (groups of 1 / 2 / 4, register / LDS
selectors) and maskset_build_kernel each exist exactly once, use no scratch memory and spill nothing.  The scan instantiations stay at or
below 256 VGPRs -- two waves per SIMD (waves by registers = floor(512 / allocation)), which is what the plan's 80 KB LDS budget of two
workgroups per CU assumes -- and own their whole LDS allocation dynamically (the host refuses a scan kernel with static LDS).  The build
kernel stays at or below 64 VGPRs.  The existing resource tests pass unchanged: no existing kernel's code moved.  No GPU needed."""
import pytest

from test_resources_u16_wide import _one, kernels  # noqa: F401  (kernels: the module-scoped fixture)

BUILD = "20maskset_build_kernelE"
INGEST = "21maskset_ingest_kernelE"


def _no_scratch(name, r):
    assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, "%s uses scratch memory: %r" % (name, r)


@pytest.mark.parametrize("small", [1, 0])
@pytest.mark.parametrize("qg", [1, 2, 4])
def test_scan_instantiation(kernels, qg, small):
    name, r = _one(kernels, "18masked_scan_kernelILi%dELb%dEE" % (qg, small))
    _no_scratch(name, r)
    assert r["vgpr_count"] <= 256, "%s uses %d VGPRs: fewer than two waves per SIMD" % (name, r["vgpr_count"])
    assert r.get("group_segment_fixed_size", 0) == 0, "%s carries static LDS" % name


def test_there_are_exactly_six_scan_instantiations(kernels):
    hits = [k for k in kernels if "18masked_scan_kernelI" in k and not k.endswith(".kd")]
    assert len(hits) == 6, sorted(hits)


def test_build_kernel(kernels):
    name, r = _one(kernels, BUILD)
    _no_scratch(name, r)
    assert r["vgpr_count"] <= 64, "%s uses %d VGPRs" % (name, r["vgpr_count"])
    assert r.get("group_segment_fixed_size", 0) == 0, "%s: the rounds go out by whole words, nothing is shared through LDS" % name


def test_ingest_kernel(kernels):
    name, r = _one(kernels, INGEST)
    _no_scratch(name, r)
