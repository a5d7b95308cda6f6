"""Register / scratch / LDS figures of score_pairs_kernel (csrc/score.hip.h), read from the code object inside the built library in the
manner of tests/test_resources_range.py: the kernel exists exactly once (written once for both code widths, no instantiation per shape),
uses no scratch memory and spills nothing (m and dsub are run-time values and no per-lane array is indexed dynamically), carries no
static LDS (the query is dynamic: d floats), and stays at or below 128 VGPRs -- at least four waves per SIMD, for a kernel whose lanes
wait on gathered rows.  No GPU needed."""
from test_resources_u16_wide import _one, kernels  # noqa: F401  (kernels: the module-scoped fixture)

PAIRS = "18score_pairs_kernelE"


def test_pair_kernel(kernels):
    name, r = _one(kernels, PAIRS)
    assert r.get("vgpr_spill_count", 0) == 0 and r.get("private_segment_fixed_size", 0) == 0, "%s uses scratch memory: %r" % (name, r)
    assert r.get("group_segment_fixed_size", 0) == 0, "%s carries static LDS" % name
    assert r["vgpr_count"] <= 128, "%s uses %d VGPRs: fewer than four waves per SIMD" % (name, r["vgpr_count"])
    print("%s: %d VGPRs, %d SGPRs" % (name, r["vgpr_count"], r.get("sgpr_count", -1)))


def test_kernel_exists_exactly_once(kernels):
    hits = [k for k in kernels if "score_pairs_kernel" in k and not k.endswith(".kd")]
    assert len(hits) == 1, sorted(hits)
