"""Register / scratch / LDS figures of the masked range search's kernels (csrc/range.hip.h), read from the code object inside the built
library in the manner of tests/test_resources_range.py: range_masked_count_kernel, range_masked_fill_kernel, range_u16_count_kernel and
range_u16_fill_kernel -- four more instantiations of range_scan_item<FILL, U16, MASKED> -- each exist exactly once, use no scratch memory,
spill nothing, carry no static LDS (residual, tables and the item's counter are dynamic) and stay at or below 256 VGPRs.  The figures are
printed; DESIGN.md 4.6.5 records them.  No GPU needed."""
import pytest

from test_resources_u16_wide import _one, kernels  # noqa: F401  (kernels: the module-scoped fixture)

NEW = ("25range_masked_count_kernelEN", "24range_masked_fill_kernelEN", "22range_u16_count_kernelEN", "21range_u16_fill_kernelEN")


@pytest.mark.parametrize("mangled", NEW)
def test_scan_kernel(kernels, mangled):
    name, r = _one(kernels, mangled)
    assert r.get("vgpr_spill_count", 0) == 0 and r.get("sgpr_spill_count", 0) == 0, "%s spills: %r" % (name, r)
    assert r.get("private_segment_fixed_size", 0) == 0, "%s uses scratch memory: %r" % (name, r)
    assert r["vgpr_count"] <= 256, "%s uses %d VGPRs: fewer than two waves per SIMD" % (name, r["vgpr_count"])
    assert r.get("group_segment_fixed_size", 0) == 0, "%s carries static LDS" % name
    print("%s: %d VGPRs, %d SGPRs" % (name, r["vgpr_count"], r.get("sgpr_count", -1)))


def test_each_kernel_exists_exactly_once(kernels):
    for part in ("range_masked_count_kernel", "range_masked_fill_kernel", "range_u16_count_kernel", "range_u16_fill_kernel"):
        hits = [k for k in kernels if part in k and not k.endswith(".kd")]
        assert len(hits) == 1, (part, sorted(hits))
    # and the plain kernels' names still match one kernel each (tests/test_resources_range.py's pin)
    for part in ("range_count_kernel", "range_fill_kernel"):
        assert len([k for k in kernels if part in k and not k.endswith(".kd")]) == 1, part
