"""CPU side of the list-end suite (tests/list_end.py; the GPU side is tests/test_gpu_list_end.py): the test has teeth.

On the very index, queries and states the GPU file walks, every way of reading past a list's end that list_end restates -- a length
rounded up to 2, 4, 64, 128, 256 or 1024 points, one slot too many, and the bound tightened by what lies behind the end while only live
points are returned -- changes the exact result of at least one of the list's own queries, for EVERY list on which the restatement
differs from the reference at all.  helpers.assert_same_results, the comparison the GPU file uses, is what must fail.

Two kinds of list are exempt, both counted from the lengths alone and the counts asserted:
* the over-read range is empty (the length is a multiple of g);
* fresh state only: the list still holds r >= K live decoys.  The zero slack behind them has the decoys' own code, hence their sum to
  the bit, and a later visit order: it cannot enter a top-K that the live decoys fill.  So that the fresh state exempts nothing for
  that reason either, the over-read is also checked at K = 256, above every r (not the tightened bound: the shortest lists' queries
  see fewer than 256 candidates in all, and a bound that nothing reaches drops nothing).
"""
import numpy as np
import pytest

import list_end as le
import write_path as wp

CPU_STATES = le.STATES[:3]


@pytest.fixture(scope="module")
def walked():
    cache = {}

    def get(kind, state):
        if (kind, state) not in cache:
            case = le.hostile_case(kind)
            lists, model, removed = le.walk_states(case, state)
            cache[(kind, state)] = (case, lists, model, removed, le.Scan(case, model))
        return cache[(kind, state)]
    return get


def test_geometry():
    assert len(le.LENS) == 32 and len(set(le.LENS)) == 32
    total = sum(le.LENS) + sum(le.decoys_of(l) for l in range(32))
    assert 32000 < total < 36000
    assert [le.decoys_of(l) for l in range(9)] == [40, 1, 2, 3, 31, 32, 64, 200, 1]
    for kind, (d, m, ksub, bits) in le.KINDS.items():
        ref, qs, decoys = le.hostile_case(kind)
        assert (ref.d, ref.m, ref.ksub, ref.kc) == (d, m, ksub, 32) and qs.shape == (256, d)
        assert np.array_equal(np.diff(ref.offsets), [le.LENS[l] + le.decoys_of(l) for l in range(32)])
        assert [len(x) for x in decoys] == [le.decoys_of(l) for l in range(32)]
        assert wp.is_u16(ref) == (bits == 16)
        lens = np.diff(le.plain_lists(le.hostile_case(kind))[0])
        assert np.array_equal(lens, le.LENS)


@pytest.mark.parametrize("kind", list(le.KINDS))
def test_append_batch_goes_in_place_and_proves_the_old_capacity(kind):
    """The third state's batch fits the room the decoys left in every list, holds no live decoy, reaches most lists -- and at least one
    list takes more points than the spare capacity a re-layout after the deletion would have given it (max(32, len / 8)): that the
    device takes the batch in place shows that the deletion kept the old blocks, stale rows included."""
    case = le.hostile_case(kind)
    _, lst, codes, ids = le.append_batch(kind)
    cnt = np.bincount(lst, minlength=32)
    assert (cnt <= le.append_quota()).all() and (cnt[le.append_quota() > 0] > 0).sum() >= 20, cnt
    assert (codes != case.zero_labels[None, :]).all()
    lens = np.array(le.LENS)
    assert (cnt > np.maximum(32, lens // 8)).any(), cnt
    assert (cnt < np.array([le.decoys_of(l) for l in range(32)]))[cnt > 0].all()      # part of the freed room: stale rows remain


@pytest.mark.parametrize("state", CPU_STATES)
@pytest.mark.parametrize("kind", list(le.KINDS))
def test_reading_past_the_end_changes_the_result(walked, kind, state):
    case, lists, model, removed, scan = walked(kind, state)
    ref = wp.ref_with_lists(case.ref, *lists)
    assert np.array_equal(model.len, np.diff(lists[0]))
    if state != "fresh":
        assert removed[0] == sum(le.decoys_of(l) for l in range(32))
    # the restatement on the model's raw rows, reading to the length and no further, IS the reference
    for K in (1, 10, 64):
        exp = wp.ref_knn(ref, case.qs, K, le.W)
        assert wp.same_answer(scan.select(K, scan.reach_exact()), exp), (kind, state, K)
    assert le.ordering_holds(case, model), "a decoy must beat every live point (%s, %s)" % (kind, state)
    fresh = state == "fresh"
    if fresh:       # positive control: the decoys are live and they are what the reference returns
        for K in (1, 10, 64):
            ids, _, counts = wp.ref_knn(ref, case.qs, K, le.W)
            for l in range(32):
                want = case.decoys[l][:min(K, le.decoys_of(l))]
                for r in range(l * le.QPL, (l + 1) * le.QPL):
                    assert counts[r] >= len(want) and np.array_equal(ids[r, :len(want)], want), (kind, l, r, K)
    lens = np.array(model.len)
    rs = np.array([le.decoys_of(l) for l in range(32)])
    # the lengths of this state from LENS, the decoy counts and the batch alone: what the exemptions are counted from
    by_rule = np.array(le.LENS) + (rs if fresh else 0) + (np.bincount(le.append_batch(kind)[1], minlength=32) if state == "appended" else 0)
    assert np.array_equal(lens, by_rule)
    reaches = [("g=%d" % g, scan.reach_overread(g), g) for g in le.GRANULES] + [("len+1", scan.reach_one_more(), None)]
    exact = {K: scan.select(K, scan.reach_exact()) for K in (1, 10, 64, 256)}
    for name, reach, g in reaches:
        empty = reach == lens                                                   # the over-read range of the model ...
        assert (reach <= np.array(model.cap)).all() and (reach >= lens).all()
        for how, Ks in (("overread", (1, 10)), ("tightened", (10, 64))):
            for K in Ks + ((256,) if fresh and how == "overread" else ()):
                tied = (rs >= K) if fresh else np.zeros(32, bool)
                exempt = empty | tied
                want_exempt = sum(1 for l in range(32) if (g is not None and by_rule[l] % g == 0) or (fresh and rs[l] >= K))
                assert int(exempt.sum()) == want_exempt                         # ... is empty exactly where the lengths say
                print("%s %s %s %s K=%d: %d lists exempt (%d with an empty over-read range, %d behind r >= K live decoys)"
                      % (kind, state, how, name, K, exempt.sum(), empty.sum(), (tied & ~empty).sum()))
                for l in np.nonzero(~exempt)[0]:
                    own = le.own_queries(int(l))
                    bad = scan.select(K, reach, own, live_only=(how == "tightened"))
                    assert not wp.same_answer(bad, le.part(exact[K], own)), \
                        "%s %s: %s %s at K=%d leaves the result of every query of list %d (length %d) unchanged" % (
                            kind, state, how, name, K, l, lens[l])
                    if how == "tightened":      # the bound failure returns fewer or other neighbours, never what lies behind the end
                        assert (bad[2] < le.part(exact[K], own)[2]).any() or not np.array_equal(bad[0], le.part(exact[K], own)[0])
                        assert (bad[2] <= le.part(exact[K], own)[2]).all()
