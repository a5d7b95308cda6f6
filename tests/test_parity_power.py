"""Can the suite tell right from almost right?  (CPU only.)

helpers.assert_same_results compares distance BITS.  This file keeps it that way: a numpy restatement of knn_search (helpers.numpy_knn)
is mutated in the ways a kernel goes subtly wrong, and every mutant must be REJECTED by the helper against the C oracle, on every shape
of test_gpu_parity.SHAPES and on every rounding-hostile input of tests/test_gpu_bitwise.py -- while the unmutated restatement must be
accepted.  A helper loosened to a tolerance again fails here: the mutants' relative errors are below 1e-6.

Variants (VARIANTS):
  fma              coarse and table sums with the multiply-add contracted (one rounding: emulated through float64)
  adc_reversed     dc + t(m-1) + ... + t0
  adc_rotated      dc + t1 + ... + t(m-1) + t0 (what the striped filter computes)
  adc_pairwise     dc + tree(t0 .. t(m-1))
  dc_last          (t0 + ... + t(m-1)) + dc
  table_f64        table entries from the f32 operands in float64, rounded once
  coarse_expanded  coarse distance as ||c||^2 - 2 q.c + ||q||^2 (float32)

Measured on the CPU with the query caps below, pooled over the 12 SHAPES rows (418 queries; 387 for the re-orderings, which leave the
m = 1 row out) / over the 25 (kind, shape) stress inputs (300 queries): the share of queries whose ids change and the share whose result
bits change (ids or distance bits; what the helper rejects):

                     SHAPES           stress inputs
  variant            ids     bits     ids     bits
  fma                0.0 %  61.2 %   2.0 %   83.3 %
  adc_reversed       0.0 %  91.0 %   3.7 %   99.7 %
  adc_rotated        0.0 %  88.6 %   2.7 %   95.7 %
  adc_pairwise       0.0 %  93.3 %   3.7 %  100.0 %
  dc_last            0.0 %  48.1 %   3.7 %   99.7 %
  table_f64          0.0 %  66.3 %   2.0 %   88.7 %
  coarse_expanded    0.2 %  49.8 %  12.3 %   97.3 %

Per shape the share of queries whose bits change is printed by `python tests/test_parity_power.py`; the smallest over all pairs that
are not identities is 1 query of 33 (dc_last on the README toy shape with w = 1; the next are 1 of 19 and 2 of 10), so every pair is
rejected.  The assertion this file replaces (ids exact, distances within 1e-4 relative) accepted every mutant query on the SHAPES rows
but one (417 to 418 of 418) and 289 to 294 of the 300 stress queries (198 for coarse_expanded): it failed only where ids moved.
"""
import numpy as np
import pytest

import helpers
from test_gpu_parity import SHAPES

f32, f64 = np.float32, np.float64
QUERY_CAP = 48            # queries per SHAPES row (fewer where the row has fewer)
STRESS_QUERIES = 12       # queries per stress input


def _fma(a, b, c):
    """fl32(a * b + c): the product of two float32 is exact in float64."""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def coarse_fma(oidx, q):
    acc = np.zeros(oidx.kc, f32)
    for i in range(oidx.d):
        t = oidx.centroids[:, i] - q[i]
        acc = _fma(t, t, acc)
    return acc


def table_fma(oidx, i, r):
    s = np.zeros(oidx.ksub, f32)
    for t_ in range(oidx.dsub):
        df = oidx.codebooks[i, :, t_] - r[i * oidx.dsub + t_]
        s = _fma(df, df, s)
    return s


def table_f64(oidx, i, r):
    sl = slice(i * oidx.dsub, (i + 1) * oidx.dsub)
    df = oidx.codebooks[i].astype(f64) - r[sl].astype(f64)[None, :]
    return (df * df).sum(1).astype(f32)


def coarse_expanded(oidx, q):
    cc = np.zeros(oidx.kc, f32)
    qc = np.zeros(oidx.kc, f32)
    qq = f32(0)
    for i in range(oidx.d):
        cc = cc + oidx.centroids[:, i] * oidx.centroids[:, i]
        qc = qc + oidx.centroids[:, i] * q[i]
        qq = f32(qq + q[i] * q[i])
    return (cc - f32(2) * qc) + qq


def _adc_in_order(order):
    def adc(dc, terms):
        dd = np.full(terms[0].shape[0], dc, f32)
        for ii in order(len(terms)):
            dd = dd + terms[ii]
        return dd
    return adc


def adc_pairwise(dc, terms):
    lvl = list(terms)
    while len(lvl) > 1:
        lvl = [lvl[i] + lvl[i + 1] if i + 1 < len(lvl) else lvl[i] for i in range(0, len(lvl), 2)]
    return f32(dc) + lvl[0]


def adc_dc_last(dc, terms):
    s = terms[0]
    for t in terms[1:]:
        s = s + t
    return s + f32(dc)


VARIANTS = {
    "fma": dict(coarse=coarse_fma, table=table_fma),
    "adc_reversed": dict(adc=_adc_in_order(lambda m: range(m - 1, -1, -1))),
    "adc_rotated": dict(adc=_adc_in_order(lambda m: list(range(1, m)) + [0])),
    "adc_pairwise": dict(adc=adc_pairwise),
    "dc_last": dict(adc=adc_dc_last),
    "table_f64": dict(table=table_f64),
    "coarse_expanded": dict(coarse=coarse_expanded),
}
REORDERINGS = ("adc_reversed", "adc_rotated", "adc_pairwise", "dc_last")


def is_identity(variant, m):
    """The ONLY pairs left out of the must-be-rejected assertion: mutations that are algebraically the identity for the shape.
    With m = 1 there is one term: every re-ordering of the ADC sum is dc + t0 (float addition commutes), bit for bit.  (The fma
    variant is never an identity here: with dsub = 1 its table sums are, its coarse sums -- d > 1 in every shape -- are not.)"""
    return variant in REORDERINGS and m == 1


def shape_input(row):
    seed, n, d, kc, m, ksub, K, w, nq = row
    oidx, data = helpers.build_index(seed, n, d, kc, m, ksub, label_perm=(seed % 2 == 0))
    rng = np.random.default_rng(seed)
    qs = np.concatenate([rng.random((nq - 3, d), dtype=f32), data[:3]])       # the queries of test_search_matches_oracle
    return oidx, qs[-QUERY_CAP:], K, w


def stress_input(kind, shape):
    seed, n, d, kc, m, ksub, K, w = helpers.BITWISE_SHAPES[shape]
    oidx, qs = helpers.build_stress_index(kind, seed, n, d, kc, m, ksub, nq=STRESS_QUERIES, label_perm=(shape == "m10"))
    return oidx, qs, K, w


INPUTS = [("shape%d" % row[0], (lambda row=row: shape_input(row))) for row in SHAPES] + \
         [("%s-%s" % (kind, shape), (lambda kind=kind, shape=shape: stress_input(kind, shape)))
          for kind in helpers.STRESS_KINDS for shape in helpers.BITWISE_SHAPES]


def _changed(got, exp):
    """Per query: (ids or counts differ, anything the helper compares differs)."""
    ids, bits = [], []
    for r in range(exp[2].shape[0]):
        c = int(exp[2][r])
        di = got[2][r] != c or not np.array_equal(got[0][r, :c], exp[0][r, :c])
        ids.append(di)
        bits.append(di or not np.array_equal(got[1][r, :c].view(np.uint32), exp[1][r, :c].view(np.uint32)))
    return np.array(ids), np.array(bits)


@pytest.mark.parametrize("name,make", INPUTS, ids=[n for n, _ in INPUTS])
def test_oracle_equals_reference_and_every_mutant_is_rejected(name, make):
    oidx, qs, K, w = make()
    exp = oidx.knn_search(qs, K, w)
    helpers.assert_same_results(helpers.numpy_knn_batch(oidx, qs, K, w), exp, what="reference restatement, " + name)
    for variant, sums in VARIANTS.items():
        got = helpers.numpy_knn_batch(oidx, qs, K, w, **sums)
        if is_identity(variant, oidx.m):
            helpers.assert_same_results(got, exp, what="%s is the identity at m = 1, %s" % (variant, name))
            continue
        with pytest.raises(AssertionError):
            helpers.assert_same_results(got, exp, what="%s, %s" % (variant, name))


def test_helper_rejects_one_ulp_and_says_where():
    """The deliberately wrong input: the rotated-order sum (what a leaked striped-filter sum would be) and a single distance moved by
    one ulp; the message names query, slot, both values in hex and the ulp distance.  Wrong dtypes are refused, not cast."""
    oidx, qs, K, w = shape_input(SHAPES[4])
    exp = oidx.knn_search(qs, K, w)
    rot = helpers.numpy_knn_batch(oidx, qs, K, w, **VARIANTS["adc_rotated"])
    assert all(np.allclose(rot[1][r], exp[1][r], rtol=1e-6, atol=0) for r in range(qs.shape[0]))     # invisible to a tolerance
    with pytest.raises(AssertionError, match=r"distance bits differ at query \d+, slot \d+ .*0x1\.[0-9a-f]+p[+-]\d+.* ulp apart"):
        helpers.assert_same_results(rot, exp, what="rotated")
    one = (exp[0].copy(), exp[1].copy(), exp[2].copy())
    one[1][7, 2] = np.nextafter(one[1][7, 2], f32(np.inf))
    with pytest.raises(AssertionError, match=r"query 7, slot 2 .* 1 ulp apart"):
        helpers.assert_same_results(one, exp)
    beyond = (exp[0].copy(), exp[1].copy(), exp[2].copy())
    beyond[1][:, K - 1] += f32(1.0)                    # slots past `count` are not compared, slots below it are
    with pytest.raises(AssertionError):
        helpers.assert_same_results(beyond, exp)
    short = (exp[0], exp[1], np.minimum(exp[2], K - 1).astype(np.int32))
    helpers.assert_same_results((beyond[0], beyond[1], short[2]), short)
    with pytest.raises(AssertionError, match="float32"):
        helpers.assert_same_results((exp[0], exp[1].astype(np.float64), exp[2]), exp)
    with pytest.raises(AssertionError, match="float32"):
        helpers.assert_same_results(exp, (exp[0], exp[1].astype(np.float64), exp[2]))
    with pytest.raises(AssertionError, match="counts differ"):
        helpers.assert_same_results((exp[0], exp[1], exp[2] - 1), exp)
    neg = (exp[0], exp[1].copy(), exp[2])
    neg[1][0, 0] = f32(-0.0)
    zero = (exp[0], exp[1].copy(), exp[2])
    zero[1][0, 0] = f32(0.0)
    with pytest.raises(AssertionError, match="1 ulp apart|0 ulp apart"):      # -0.0 and +0.0 are different bits
        helpers.assert_same_results(neg, zero)


def measure():
    """The docstring's figures."""
    pooled = {v: {"SHAPES": [0, 0, 0, 0], "stress": [0, 0, 0, 0]} for v in VARIANTS}
    smallest = (2.0, "")
    for name, make in INPUTS:
        oidx, qs, K, w = make()
        exp = oidx.knn_search(qs, K, w)
        line = []
        for variant, sums in VARIANTS.items():
            got = helpers.numpy_knn_batch(oidx, qs, K, w, **sums)
            ids, bits = _changed(got, exp)
            old_ok = sum(1 for r in range(qs.shape[0]) if not ids[r] and np.allclose(got[1][r, :exp[2][r]], exp[1][r, :exp[2][r]], rtol=1e-4, atol=0))
            p = pooled[variant]["SHAPES" if name.startswith("shape") else "stress"]
            if not is_identity(variant, oidx.m):
                p[0] += int(ids.sum()); p[1] += int(bits.sum()); p[2] += len(bits); p[3] += old_ok
                smallest = min(smallest, (bits.mean(), "%s %s" % (name, variant)))
            line.append("%s %d/%d" % (variant, bits.sum(), len(bits)))
        print("%-28s %s" % (name, "  ".join(line)), flush=True)
    for v, p in pooled.items():
        a, b = p["SHAPES"], p["stress"]
        print("  %-18s %5.1f %%  %5.1f %%   %5.1f %%  %5.1f %%   (n = %d, %d; old assertion accepted %d, %d)" % (
            v, 100.0 * a[0] / a[2], 100.0 * a[1] / a[2], 100.0 * b[0] / b[2], 100.0 * b[1] / b[2], a[2], b[2], a[3], b[3]))
    print("smallest share of changed queries over non-identity pairs: %.3f (%s)" % smallest)


if __name__ == "__main__":
    measure()
