"""The range search's definition, its case table and the teeth of that table, on the CPU (tests/range_ref.py; no GPU, no native library).

* range_reference (knn_search with K = every stored point, cut at d <= r) equals the second statement of the same thing (every probed
  entry with distance, probe rank and position; filter; sort) and the C oracle's knn_search, cut, on every row of the table.
* the table asserts its own preconditions: an empty result, a skipped probe, a boundary inside a cross-list tie run, a result spanning
  both chunks of the long list, a probed empty list, a boundary strictly inside a single list's tie run, a point whose distance is its probe's dc itself -- each occurs.
* every entry of range_ref.MUTANTS differs from the reference somewhere on the table; none is merely equivalent.
"""
import numpy as np
import pytest

import range_ref as rr


@pytest.mark.parametrize("stride", rr.STRIDES)
def test_reference_is_the_cut_knn_search(stride):
    ref, qs = rr.case(stride)
    for w in rr.WS:
        qis, radii, _ = rr.table(stride, w)
        exp = rr.expected(stride, w)
        assert rr.same(rr.model(stride, qis, radii, w), exp), (stride, w)
        oi, od, oc = ref.knn_search(qs, rr.N, w)                    # the C oracle, cut
        rows = [rr.cut(oi[qi, :oc[qi]], od[qi, :oc[qi]], r) for qi, r in zip(qis, radii)]
        assert rr.same(rr.pack(rows), exp), (stride, w)
    # range_reference itself, on one row of each kind
    qis, radii, kinds = rr.table(stride, 3)
    exp = rr.expected(stride, 3)
    for row in range(len(rr.KINDS)):
        i, d = rr.range_reference(ref, qs[qis[row]], radii[row], 3)
        assert np.array_equal(i, exp[1][exp[0][row]:exp[0][row + 1]]) and np.array_equal(d, exp[2][exp[0][row]:exp[0][row + 1]])


def test_radius_edge_values():
    """NaN keeps nothing in the float compare AND in the kernels' integer compare as range_plan.h guards it; -0.0 is 0"""
    ref, qs = rr.case("u8_m8")
    assert len(rr.range_reference(ref, qs[0], np.float32(np.nan), 3)[0]) == 0
    assert len(rr.range_reference(ref, qs[0], np.float32(-np.inf), 3)[0]) == 0
    everything = rr.range_reference(ref, qs[0], np.float32(np.inf), rr.KC)
    assert len(everything[0]) == rr.N

    def kernel_test(dbits, r):     # range.hip.h: radius_live(r) && bits(d) <= radius_bits(r)
        r = np.float32(r)
        if not (r >= 0):
            return False
        rb = 0 if r == 0 else int(r.view(np.uint32))
        return dbits <= rb
    for d in (0.0, 1e-30, 0.5, 3.0e38):
        db = int(np.float32(d).view(np.uint32))
        for r in (np.nan, -np.nan, -1.0, -0.0, 0.0, 0.5, np.inf, -np.inf, 1e-30):
            assert kernel_test(db, r) == bool(np.float32(d) <= np.float32(r)), (d, r)
    assert int(np.float32(np.nan).view(np.uint32)) > int(np.float32(3.0e38).view(np.uint32)), "without the guard a NaN radius would pass everything"


def test_table_meets_its_preconditions():
    seen = {k: 0 for k in ("empty", "skipped probe", "cross-list run", "both chunks", "empty list probed", "d == dc", "run cut whole",
                          "in-list run, j strictly inside")}
    for stride in rr.STRIDES:
        ref, _ = rr.case(stride)
        lens = np.diff(ref.offsets)
        for w in rr.WS:
            qis, radii, kinds = rr.table(stride, w)
            lims, ids, dd = rr.expected(stride, w)
            for row, (qi, r, kind) in enumerate(zip(qis, radii, kinds)):
                E = rr.entries(stride, int(qi))
                weff = min(w, rr.KC)
                cnt = int(lims[row + 1] - lims[row])
                got = ids[lims[row]:lims[row + 1]]
                seen["empty"] += cnt == 0
                seen["skipped probe"] += bool((E["dcs"][:weff] > r).any() and cnt > 0)
                seen["empty list probed"] += bool((lens[E["cells"][:weff]] == 0).any() and cnt > 0)
                take = E["rank"] < weff
                if kind == "in_run":
                    run = take & (E["d"] == r)
                    D = rr.full_sorted(stride, int(qi), w)[1]
                    at = np.nonzero(D == r)[0]
                    if len(np.unique(E["rank"][run])) == 1 and len(at) >= 3:      # one list's run, and rr.table picked a j with both neighbours in it
                        seen["in-list run, j strictly inside"] += 1
                        assert cnt == int(at[-1]) + 1 and set(E["id"][run]) <= set(got), "the run comes back whole"
                        assert int(lims[row + 2] - lims[row + 1]) == int(at[0]), "in_run- (the next row) ends in front of the run"
                if kind == "cross_run":
                    run = take & (E["d"] == r)
                    if len(np.unique(E["rank"][run])) > 1:
                        seen["cross-list run"] += 1
                        assert set(E["id"][run]) <= set(got), "the run comes back whole"
                        prev = rr.expected(stride, w)
                        seen["run cut whole"] += int(prev[0][row + 2] - prev[0][row + 1]) == cnt - int(run.sum())   # (the next row is cross_run-)
                hit = take & (E["lst"] == rr.HIT) & np.isin(E["id"], got)
                seen["both chunks"] += bool((E["pos"][hit] < rr.CHUNK).any() and (E["pos"][hit] >= rr.CHUNK).any())
                if kind == "dchit" and qi == rr.NQ - 1:
                    seen["d == dc"] += bool((E["d"][take & (E["lst"] == rr.HIT)] == r).any())
    for k, v in seen.items():
        assert v > 0, "the table never shows: %s" % k
    assert seen["d == dc"] >= len(rr.STRIDES), "every stride has the exact hit (at w = kc at least)"
    assert seen["in-list run, j strictly inside"] >= len(rr.STRIDES) and seen["cross-list run"] >= len(rr.STRIDES)


@pytest.mark.parametrize("name", sorted(rr.MUTANTS))
def test_mutant_is_told_from_the_reference(name):
    differs = 0
    for stride in rr.STRIDES:
        for w in rr.WS:
            qis, radii, _ = rr.table(stride, w)
            differs += not rr.same(rr.model(stride, qis, radii, w, **rr.MUTANTS[name]), rr.expected(stride, w))
    assert differs > 0, "mutant '%s' gives the reference's answer on every row of the table" % name
    assert name not in rr.EQUIVALENT


def test_no_mutant_is_only_equivalent():
    assert rr.EQUIVALENT == {} and len(rr.MUTANTS) == 9
