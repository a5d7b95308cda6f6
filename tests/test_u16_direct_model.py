"""The bit-exact assertions of tests/test_gpu_u16_direct.py have teeth on the inputs they use.  A numpy restatement of three orders in which
a table-free scan could form a point's distance (no GPU needed):

  contract    per sub-space an accumulator of its own from zero, sum = sum + df * df in ascending t, then acc = acc + sum -- the table
              entry's expression: what u16_direct_scan_kernel computes;
  folded      the terms added straight into the running sum, acc = acc + df * df;
  contracted  the contract's order with every multiply-add rounded once (an fma), what the compiler would emit without -ffp-contract=off.

The contract must reproduce tests/u16_ref.py on every query; each of the two natural mistakes must change the returned bytes of at least
half of the queries at K = 64, so a kernel that made one would fail the GPU comparisons."""
import numpy as np
import pytest

import u16_ref

f32 = np.float32


def knn_variant(ix, q, K, w, variant):
    q = np.asarray(q, f32)
    order, acc = u16_ref.coarse(ix, q, w)
    cand_d, cand_id = [], []
    for cl in order:
        lo, hi = int(ix.offsets[cl]), int(ix.offsets[cl + 1])
        dd = np.full(hi - lo, acc[cl], f32)
        r = q - ix.centroids[cl]
        for ii in range(ix.m):
            cw = ix.codebooks[ii, ix.inv[ii, ix.codes[lo:hi, ii]]]            # (len, dsub): the gathered codewords
            s = np.zeros(hi - lo, f32)
            for t in range(ix.dsub):
                df = cw[:, t] - r[ii * ix.dsub + t]
                if variant == "contract":
                    s = s + df * df
                elif variant == "folded":
                    dd = dd + df * df
                else:                                                         # the f64 product of two f32 is exact: one rounding of a*b + c
                    s = (df.astype(np.float64) * df.astype(np.float64) + s.astype(np.float64)).astype(f32)
            if variant != "folded":
                dd = dd + s
        cand_d.append(dd)
        cand_id.append(ix.ids[lo:hi])
    cd, ci = np.concatenate(cand_d), np.concatenate(cand_id)
    sel = np.lexsort((np.arange(cd.shape[0]), cd))[:K]
    return ci[sel], cd[sel]


def differing(ix, Q, K, w, variant):
    n = 0
    for q in Q:
        ei, ed = u16_ref.knn_one(ix, q, K, w)
        gi, gd = knn_variant(ix, q, K, w, variant)
        n += not (np.array_equal(ei, gi) and ed.tobytes() == gd.tobytes())
    return n


CASES = {
    "gpu_test_1": lambda: u16_ref.make_index(4242, 40000, 32, 4, 4, 1024, perm_labels=True, ndistinct=5000),
    "d32_m4_k1024": lambda: u16_ref.make_index(11, 6000, 32, 6, 4, 1024),
    "d20_m4_k300": lambda: u16_ref.make_index(12, 6000, 20, 6, 4, 300),
    "d64_m2_k257": lambda: u16_ref.make_index(13, 6000, 64, 6, 2, 257),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_contract_is_exact_and_the_mistakes_are_caught(case):
    ix = CASES[case]()
    Q = np.random.default_rng(9).random((8, ix.d), dtype=f32)
    w = 3
    for K in (1, 10, 64):
        assert differing(ix, Q, K, w, "contract") == 0, "the contract differs from the reference at K=%d" % K
    folded = differing(ix, Q, 64, w, "folded")
    contracted = differing(ix, Q, 64, w, "contracted")
    print("%s: K=64 folded differs on %d / 8, contracted on %d / 8; K=10 folded %d, contracted %d"
          % (case, folded, contracted, differing(ix, Q, 10, w, "folded"), differing(ix, Q, 10, w, "contracted")))
    assert folded >= 4, "folding the terms into the running sum would go unnoticed: %d / 8 queries differ" % folded
    assert contracted >= 4, "a contracted multiply-add would go unnoticed: %d / 8 queries differ" % contracted
