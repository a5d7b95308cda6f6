"""CPU side of the placement suite (tests/placement.py; the GPU side is tests/test_gpu_placement.py): the placements have teeth.

On the very lists and queries the GPU file searches, placement.model -- P parts with a selector each under a shared bound, then a merge --
returns the reference's K best at every K and every geometry while it is right, and every one of placement.MUTANTS, the ways this class
of bound goes wrong, changes the result of at least one (placement, K) pair at EVERY geometry: (64, 4), (256, 4), (256, 8) and one part
per chunk of 1024 and of 2048 points.  A mutant that no placement catches is a hole in the placements.

The `shuffled` lists are the control: what random placement alone sees.  Measured over all (K, geometry) pairs of the two shuffled lists
of m8_d32 (printed by test_what_the_shuffled_control_sees; nothing is asserted about it): each of the 6 mutants at SOME geometry, but
only 19 of the 30 (mutant, geometry) pairs, where the placements catch 30 of 30 -- a at (64, 4) alone; b at the three (granule, parts)
geometries and at neither chunk size; c everywhere but at the 1024-point chunks; d and e at (64, 4) and, through the short list that
is ONE chunk (a single part's bound is its own K-th key), at both chunk sizes, never at (256, 4) or (256, 8); f everywhere.

Two more ways are restated as placement.EQUIVALENT, not as mutants -- (g) a bound applied to the next probe's keys before their
visit-order base is added, (h) probe pruning with >= for > against the next probe's coarse distance: both differ from the right form
only at an exact tie of sums ACROSS probes, where the later probe's key loses by its visit order either way.
test_the_equivalent_forms_change_nothing runs them on the probe placement, where the model's probe pruning is shown to be live.
"""
import numpy as np
import pytest

import helpers
import placement as pl
import u16_ref
from oracle import oracle as ora

KINDS = list(pl.KINDS)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(np.ascontiguousarray(a[1]).view(np.uint32), np.ascontiguousarray(b[1]).view(np.uint32))


@pytest.fixture(scope="module")
def designer():
    """kind -> per list the sums of its designer query's probes, computed once"""
    cache = {}

    def get(kind):
        if kind not in cache:
            case = pl.placed_case(kind)
            cache[kind] = [[s for _, s in pl.probe_sums(case, case.designer(l))] for l in range(len(case.lists))]
        return cache[kind]
    return get


@pytest.mark.parametrize("kind", KINDS)
def test_geometry(kind):
    """Every list holds its ranks where its placement says, by the designer query's sums in the reference's order."""
    case = pl.placed_case(kind)
    ref = case.ref
    d, m, ksub, bits = pl.KINDS[kind]
    assert (ref.d, ref.m, ref.ksub) == (d, m, ksub) and case.u16 == (bits == 16)
    assert case.qs.shape == (len(case.lists) * pl.QPL, d) and int(ref.offsets[-1]) < 1_000_000
    assert sorted({L for _, L, _ in case.lists}) == [pl.LEN_SHORT, pl.LEN_LONG]
    assert all(L % g for L in (pl.LEN_SHORT, pl.LEN_LONG) for g in (64, 256, 1024, 2048, 4096))
    names = {name for name, _, _ in case.lists}
    for want in ("ascending", "descending", "split", "near_misses_first", "shuffled", "lane(0)", "stride(1024,37)", "block(2048,1)",
                 "tied(descending)"):
        assert want in names
    for l, (name, L, pi) in enumerate(case.lists):
        (cl, sums), = pl.probe_sums(case, case.designer(l))[:1]
        assert cl == l and len(sums) == L == int(ref.offsets[l + 1] - ref.offsets[l])
        by_rank = sums[pi]
        assert (np.diff(by_rank) >= 0).all(), name
        if name.startswith("tied"):
            assert (by_rank[:pl.NTIED] == by_rank[0]).all() and by_rank[pl.NTIED + 1] > by_rank[0], name
        else:
            assert (np.diff(by_rank[:256]) > 0).mean() > 0.95, name        # (random rows: hardly any exact tie)
        for i in range(1, 3):                                               # the designer query verbatim
            assert np.array_equal(case.qs[l * pl.QPL + i], case.qs[l * pl.QPL])
    # what the placements promise, on positions alone
    L = pl.LEN_LONG
    by = {name: pi for name, n, pi in case.lists if n == L}
    assert np.array_equal(by["ascending"][:5], [0, 1, 2, 3, 4]) and np.array_equal(by["descending"][:3], [L - 1, L - 2, L - 3])
    assert np.array_equal(by["split"][:4], [0, L - 1, 1, L - 2])
    assert np.array_equal(by["block(256,13)"][:256], 13 * 256 + np.arange(256))
    assert np.array_equal(by["lane(37)"][:90], 64 * np.arange(90) + 37)
    assert np.array_equal(by["stride(1024,37)"][:9], [37, 1061, 2085, 3109, 4133, 5157, 6181, 38, 1062])
    assert np.array_equal(by["near_misses_first"][128:256], 127 - np.arange(128)) and np.array_equal(by["near_misses_first"][:128], L - 128 + np.arange(128))


@pytest.mark.parametrize("kind", KINDS)
def test_the_sorted_reference_is_the_reference(kind):
    """placement.reference (one sort per query, a prefix per K) is helpers.numpy_knn_batch / u16_ref.knn: every query at the largest K,
    the designer query of every list at six K (a sort's prefix is the sort of fewer) -- and, 8-bit, the C oracle on every query at three K."""
    case = pl.placed_case(kind)
    knn = (lambda q, K: u16_ref.knn(case.ref, q, K, pl.W)) if case.u16 else (lambda q, K: helpers.numpy_knn_batch(case.ref, q, K, pl.W))
    assert _same(pl.reference(case, pl.KMAX), knn(case.qs, pl.KMAX)[:2])
    own = case.qs[::pl.QPL]
    for K in (1, 9, 17, 64, 73, 129):
        exp = knn(own, K)
        assert (exp[2] == K).all()
        got = pl.reference(case, K)
        assert _same((got[0][::pl.QPL], got[1][::pl.QPL]), exp[:2]), K
    if not case.u16:
        for K in (1, 17, 128):
            helpers.assert_same_results(pl.reference(case, K), case.ref.knn_search(case.qs, K, pl.W, nthreads=ora.max_threads()), what="K=%d" % K)


def _expected(case, probes, l, K):
    ids, dists, _ = pl.reference(case, K, slice(case.designer(l), case.designer(l) + 1))
    return ids[0], dists[0]


def _ids_of(case, l):
    ref = case.ref
    pr = [cl for cl, _ in pl.probe_sums(case, case.designer(l))]
    return np.concatenate([ref.ids[ref.offsets[cl]:ref.offsets[cl + 1]] for cl in pr])


@pytest.mark.parametrize("kind", KINDS)
def test_the_model_is_the_reference(designer, kind):
    """Unmutated, the model returns the reference's ids and distance bits on every placed list at every K: at every geometry for
    m8_d32 and u16, at one geometry per (list, K) -- all five in turn -- for the other kinds."""
    case = pl.placed_case(kind)
    full = kind in ("m8_d32", "u16")
    for l, probes in enumerate(designer(kind)):
        ids = _ids_of(case, l)
        for ki, K in enumerate(pl.K_ALL):
            exp = _expected(case, probes, l, K)
            geos = pl.GEOMETRIES if full else (pl.GEOMETRIES[(l + ki) % len(pl.GEOMETRIES)],)
            for geo in geos:
                order, dd = pl.model(probes, K, *geo)
                assert _same((ids[order], dd), exp), "%s, %s, K=%d, geometry %s" % (kind, case.what(case.designer(l)), K, geo)
            assert np.array_equal(pl.exhaustive(probes, K)[1].view(np.uint32), exp[1].view(np.uint32))


def _caught(case, probes_of_list, lists, geo, mutant, Ks=pl.K_ALL):
    """the first (list, K) at which the mutant's result differs from the model's own, or None"""
    for K in Ks:
        for l in lists:
            probes = probes_of_list[l]
            if not _same(pl.model(probes, K, *geo, mutant=mutant), pl.exhaustive(probes, K)):
                return l, K
    return None


@pytest.mark.parametrize("geo", pl.GEOMETRIES, ids=lambda g: "g%d_p%s" % g)
@pytest.mark.parametrize("kind", KINDS)
def test_every_mutant_is_caught_at_every_geometry(designer, kind, geo):
    case = pl.placed_case(kind)
    probes = designer(kind)
    lists = [l for l, (name, _, _) in enumerate(case.lists) if name != "shuffled"]
    missed = []
    for mutant, text in pl.MUTANTS.items():
        hit = _caught(case, probes, lists, geo, mutant)
        if hit is None:
            missed.append("(%s) %s" % (mutant, text))
        else:
            print("%s geometry %s mutant %s: caught first by %s at K=%d" % (kind, geo, mutant, case.lists[hit[0]][0], hit[1]))
    assert not missed, "%s, geometry %s: no placement catches %s -- a hole in the placements" % (kind, geo, "; ".join(missed))


def test_what_the_shuffled_control_sees(designer):
    """The record of what random placement alone would have seen (the module's docstring quotes it); nothing is asserted about it."""
    case = pl.placed_case("m8_d32")
    probes = designer("m8_d32")
    lists = [l for l, (name, _, _) in enumerate(case.lists) if name == "shuffled"]
    assert len(lists) == 2
    seen = {}
    for mutant in pl.MUTANTS:
        seen[mutant] = [geo for geo in pl.GEOMETRIES if _caught(case, probes, lists, geo, mutant) is not None]
    print("the shuffled control catches %d of %d mutants: %s" % (sum(1 for v in seen.values() if v), len(seen),
                                                                 {k: v for k, v in seen.items()}))


@pytest.mark.parametrize("mode", pl.PROBE_MODES)
def test_probe_placement_geometry(mode):
    """The all-zero code sits only where the mode says, beats every ordinary point of every probed list, and -- in the designer query's
    first probe -- lies below the second probe's coarse distance, while every ordinary point's sum lies above every coarse distance:
    K = 1 / 10 end below the next probe's coarse distance, K = 17 / 64 above."""
    import list_end as le
    cent, cbs, labels, zero, qs, order, dcs = pl._probe_base()
    assert len(set(order.tolist())) == max(pl.PROBE_WS) == 65 and (np.diff(dcs) >= 0).all()
    for w in pl.PROBE_WS:
        c = pl.probe_case(mode, w)
        ref = c.ref
        assert (ref.kc, ref.d, ref.m) == (pl.PROBE_KC, pl.PROBE_D, pl.PROBE_M) and c.qs.shape == (pl.PROBE_NQ, pl.PROBE_D)
        is_zero = (ref.codes == 0).all(1)
        per_list = np.add.reduceat(is_zero.astype(np.int64), ref.offsets[:-1])
        want = np.zeros(ref.kc, np.int64)
        want[{"first": order[:1], "last": order[w - 1:w], "each": order}[mode]] = 1 if mode == "each" else pl.PROBE_WINNERS
        assert np.array_equal(per_list, want), (mode, w)
        assert (np.diff(ref.offsets) == pl.PROBE_ORDINARY + want).all()
        if w not in (1, 25, 65):
            continue
        for r in (0, 5, 9):
            probes, pd = le.probes_of(cent, qs[r:r + 1], w)
            for j, cl in enumerate(probes[0]):
                rows = ref.codes[ref.offsets[cl]:ref.offsets[cl + 1]]
                s = le.row_sums(ref, qs[r], int(cl), pd[0, j], rows)
                z = (rows == 0).all(1)
                assert s[~z].min() > 10 * dcs[-1] and s[~z].min() > 10 * pd[0].max()        # ordinary: above every coarse distance
                if z.any():
                    assert s[z].max() < s[~z].min()
                    if r == 0 and j == 0:
                        assert s[z].max() < dcs[1]                                            # winners of probe 0: below the next one
        for K in (10, 17):
            helpers.assert_same_results(helpers.numpy_knn_batch(ref, qs, K, w), ref.knn_search(qs, K, w), what="%s w=%d K=%d" % (mode, w, K))


def test_the_equivalent_forms_change_nothing():
    """placement.EQUIVALENT on the probe placement (every mode, w on both sides of every edge, every K) with the model's probe pruning on:
    the reference's result, and -- winners in the first probe, K within them -- probes are in fact skipped."""
    import list_end as le
    for mode in pl.PROBE_MODES:
        for w in (2, 3, 25, 65):
            c = pl.probe_case(mode, w)
            ref = c.ref
            for r in (0, 9):
                probes, dcs = le.probes_of(ref.centroids, c.qs[r:r + 1], w)
                sums = [le.row_sums(ref, c.qs[r], int(cl), dcs[0, j], ref.codes[ref.offsets[cl]:ref.offsets[cl + 1]]) for j, cl in enumerate(probes[0])]
                for K in pl.PROBE_KS:
                    want = pl.exhaustive(sums, K)
                    for mutant in (None,) + tuple(pl.EQUIVALENT):
                        info = {}
                        got = pl.model(sums, K, 1024, None, mutant=mutant, dcs=dcs[0], info=info)     # (one part per list: its bound is its K-th key)
                        assert _same(got, want), (mode, w, r, K, mutant)
                        if mode == "first" and r == 0 and K <= 10:
                            assert info.get("skipped", 0) == w - 1, (mode, w, K, mutant, info)
                        if mode == "last" and r == 0:
                            assert info.get("skipped", 0) == 0, (mode, w, K, mutant, info)
