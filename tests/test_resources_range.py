"""Register / scratch / LDS figures of the range search's kernels (csrc/range.hip.h), read from the code object inside the built library in
the manner of tests/test_resources_masked.py: range_count_kernel, range_fill_kernel (the two instantiations of range_scan_item<FILL>) and
range_emit_kernel each exist exactly once, use no scratch memory, spill nothing and carry no static LDS (the scan kernels' tables and the
item's counter are dynamic: the host refuses a scan kernel with static LDS).  The two scan kernels stay at or below 256 VGPRs -- two waves
per SIMD by registers -- which is all their LDS leaves room for at m = 48 (52 KB a workgroup).  No GPU needed."""
import pytest

from test_resources_u16_wide import _one, kernels  # noqa: F401  (kernels: the module-scoped fixture)

SCAN = ("18range_count_kernelEN", "17range_fill_kernelEN")
EMIT = "17range_emit_kernelE"
OFFSETS = "20range_offsets_kernelE"


def _no_scratch(name, r):
    assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, "%s uses scratch memory: %r" % (name, r)


@pytest.mark.parametrize("mangled", SCAN)
def test_scan_kernel(kernels, mangled):
    name, r = _one(kernels, mangled)
    _no_scratch(name, r)
    assert r["vgpr_count"] <= 256, "%s uses %d VGPRs: fewer than two waves per SIMD" % (name, r["vgpr_count"])
    assert r.get("group_segment_fixed_size", 0) == 0, "%s carries static LDS" % name
    print("%s: %d VGPRs, %d SGPRs" % (name, r["vgpr_count"], r.get("sgpr_count", -1)))


def test_emit_kernel(kernels):
    name, r = _one(kernels, EMIT)
    _no_scratch(name, r)
    assert r["vgpr_count"] <= 64, "%s uses %d VGPRs" % (name, r["vgpr_count"])
    assert r.get("group_segment_fixed_size", 0) == 0, "%s carries static LDS" % name


def test_offsets_kernel(kernels):
    name, r = _one(kernels, OFFSETS)
    _no_scratch(name, r)


def test_each_kernel_exists_exactly_once(kernels):
    for part in ("range_count_kernel", "range_fill_kernel", "range_emit_kernel", "range_offsets_kernel"):
        hits = [k for k in kernels if part in k and not k.endswith(".kd")]
        assert len(hits) == 1, (part, sorted(hits))
