"""The eight-wave kernel's integer filter at SIXTEEN terms (csrc/wg8scan.hip.h, m = 16), restated in numpy.  (CPU only.)

float32 operation for operation, as the kernel evaluates it:

  inv  = 2047 / (largest entry of the query's sixteen tables)                    [table build, step (3)]
  q    = min(2047, floor(t * inv))                                               [an entry's 16-bit field]
  x    = ((thr * (1 + 2^-18) - dc) * inv) * (1 + 2^-18)                          [w8_bias, as qf_targets]
  T    = 0 if x < 0, floor(x) + 2 if x < 32000, else 0x7FFF                      [the budget of a point's integer sum]

and a point is a candidate iff the sum of its sixteen fields is <= T.  The header's argument says that no point whose reference-order
float sum S = ((dc + t0) + t1) + ... + t15 is at or below the bound thr is ever refused, and that a sum never reaches 0x8000 (16 x 2047 =
32 752), so the biased 16-bit fields of the scan loop never carry.  Both are asserted here on twelve random m = 16 tables (d = 64 and
128, the widths the kernel is instantiated for) and on the extremes of test_eight_wave_kernel_filter_extremes -- outlier codewords, zero
codebooks, tiny and huge scale, the coarse distance dominating -- for thresholds drawn AT the sums themselves (the boundary), one float
below and above them, and far out on both sides.  Every input holds the point whose code picks the largest entry of every sub-quantizer.

Teeth: the m = 8 constants (cap 4095) applied to the same sixteen terms overflow the field -- asserted on the same inputs."""
import numpy as np
import pytest

import helpers

f32 = np.float32
M = 16
C18 = f32(1.0000038146972656)     # 1 + 2^-18
RANDOM = [(seed, 128 if seed % 2 else 64) for seed in range(1, 13)]
EXTREMES = ["outlier_codewords", "zero_codebooks", "tiny_scale", "huge_scale", "dc_dominates_300", "dc_dominates_5000", "dc_zero_huge_entries"]


def tables(seed, d, case=None):
    """(dc, tab[16][256]) of one query against one list, in the reference's order (helpers.ref_coarse / ref_table)."""
    kc = 4
    cent, cbs, labels = helpers.make_quantizers(seed, d, kc, M, 256)
    rng = np.random.default_rng(seed + 77)
    q = rng.random(d, dtype=f32)
    if case == "outlier_codewords":
        cbs[:, 7, :] *= f32(1000.0)
    elif case == "zero_codebooks":
        cbs[:] = 0
        q = cent[0].copy()
    elif case == "tiny_scale":
        cbs *= f32(1e-21); cent *= f32(1e-21); q *= f32(1e-21)
    elif case == "huge_scale":
        cbs *= f32(1e15); cent *= f32(1e15); q *= f32(1e15)
    elif case in ("dc_dominates_300", "dc_dominates_5000"):
        cent += f32(300.0 if case.endswith("300") else 5000.0)
        cbs *= f32(1e-3)
    elif case == "dc_zero_huge_entries":
        cbs *= f32(1e3)
        q = cent[0].copy()

    class O:
        pass
    o = O()
    o.kc, o.d, o.m, o.ksub, o.dsub, o.centroids, o.codebooks = kc, d, M, 256, d // M, cent, cbs
    with np.errstate(over="ignore", under="ignore"):
        dc = helpers.ref_coarse(o, q)[0]
        r = q - cent[0]
        tab = np.stack([helpers.ref_table(o, i, r) for i in range(M)])
    return f32(dc), tab.astype(f32)


def points(tab, seed, n=3000):
    """Random codes, plus the codes of the largest and of the smallest entry of every sub-quantizer and their one-off neighbours."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (n, M))
    hi, lo = tab.argmax(1), tab.argmin(1)
    extra = [hi, lo]
    for i in range(M):
        a = hi.copy(); a[i] = lo[i]; extra.append(a)
        b = lo.copy(); b[i] = hi[i]; extra.append(b)
    return np.concatenate([codes, np.stack(extra)])


def quantise(tab, cap):
    """The fields, and inv.  (u32)floorf(x) of the device: NaN -> 0, values past the range saturate (the cap takes them)."""
    mx = tab.max()
    with np.errstate(all="ignore"):
        inv = f32(cap) / mx if mx > 0 else f32(0)
        v = np.floor(tab * f32(inv))
    v = np.where(np.isnan(v), 0.0, np.clip(v, 0.0, float(cap)))
    return v.astype(np.int64), f32(inv)


def budget(thr, dc, inv):
    with np.errstate(all="ignore"):
        x = f32(f32(f32(f32(thr * C18) - dc) * inv) * C18)
    if x < 0:
        return 0
    return int(np.floor(x)) + 2 if x < f32(32000.0) else 0x7FFF


def ref_sums(dc, tab, codes):
    with np.errstate(over="ignore"):
        return helpers.ref_adc(dc, [tab[ii, codes[:, ii]] for ii in range(M)])


def thresholds(S, seed):
    rng = np.random.default_rng(seed)
    fin = np.sort(S[np.isfinite(S)])
    picks = [fin[0], fin[-1]] if fin.size else []
    if fin.size:
        picks += list(fin[rng.integers(0, fin.size, 24)])
        picks += list(fin[: 8])
    out = []
    for t in picks:
        out += [f32(t), np.nextafter(f32(t), f32(-np.inf)), np.nextafter(f32(t), f32(np.inf))]
    out += [f32(0), f32(1e-38), f32(3e38), f32(1e-45)]
    return [t for t in out if np.isfinite(t) and t >= 0]


INPUTS = [("random", s, d) for s, d in RANDOM] + [(c, 100 + i, 128) for i, c in enumerate(EXTREMES)] + [(c, 200 + i, 64) for i, c in enumerate(EXTREMES)]


@pytest.mark.parametrize("case,seed,d", INPUTS)
def test_sixteen_term_filter_refuses_no_candidate(case, seed, d):
    dc, tab = tables(seed, d, None if case == "random" else case)
    assert (tab >= 0).all()
    codes = points(tab, seed)
    S = ref_sums(dc, tab, codes)
    q, inv = quantise(tab, 2047)
    Q = sum(q[ii, codes[:, ii]] for ii in range(M))
    assert Q.max() < 0x8000, "an integer sum reaches the bias bit"
    assert 0x8000 + Q.max() < 0x10000, "a biased field carries"
    for thr in thresholds(S, seed):
        T = budget(thr, dc, inv)
        assert 0 <= T <= 0x7FFF
        true = S <= thr
        refused = true & (Q > T)
        assert not refused.any(), "%s d=%d thr=%r: %d true candidates refused (sum %d > budget %d)" % (
            case, d, thr, refused.sum(), Q[refused].min(), T)


def test_eight_term_constants_overflow_at_sixteen_terms():
    """Cap 4095 on sixteen terms: 16 x 4095 = 65 520.  The point that takes every sub-quantizer's largest entry is past 0x7FFF on the random
    tables (the sub-quantizers' maxima lie within a factor of two of each other), so its field would run into the neighbour's."""
    over = 0
    for case, seed, d in INPUTS:
        dc, tab = tables(seed, d, None if case == "random" else case)
        codes = points(tab, seed)
        q, _ = quantise(tab, 4095)
        Q = sum(q[ii, codes[:, ii]] for ii in range(M))
        over += int(Q.max() >= 0x8000)
    assert over >= 1, "the m = 8 constants never overflow on these inputs: the test has no teeth"
    assert over >= len(RANDOM), over
