"""Register / scratch / LDS figures of the two kernels of the subset views (csrc/subset.hip.h), read from the code object inside the
built library in the manner of tests/test_resources_u16_wide.py: each exists exactly once, uses no scratch memory, and carries no static
LDS beyond the four wave totals (16 bytes).  The register bounds are the figures DESIGN.md 4.6.2 states (10 and 30 VGPRs), with room
for a compiler's mood: what matters is that both stay far below the 64 that would cost a wave of occupancy.  No GPU needed."""
from test_resources_u16_wide import _one, kernels  # noqa: F401  (kernels: the module-scoped fixture)

COUNT, SCATTER = "19subset_count_kernelE", "21subset_scatter_kernelE"


def _lean(name, r, vgprs):
    assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, "%s uses scratch memory: %r" % (name, r)
    assert r.get("group_segment_fixed_size", 0) == 16, "%s: static LDS is %s bytes, the four wave totals are 16" % (name, r.get("group_segment_fixed_size"))
    assert r["vgpr_count"] <= vgprs, "%s uses %d VGPRs" % (name, r["vgpr_count"])


def test_count_kernel(kernels):
    _lean(*_one(kernels, COUNT), 32)


def test_scatter_kernel(kernels):
    _lean(*_one(kernels, SCATTER), 64)
