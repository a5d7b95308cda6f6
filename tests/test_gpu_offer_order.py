"""The offer order of the query-major scan at one probe per round and of the stand-alone top-w at one wave per query (DESIGN.md 4.2 /
4.6; the CPU side is tests/test_offer_order_model.py).

Both offer each lane's smallest key to an empty register selector first.  What a selector ends with is the K smallest keys of the set it
was offered, so nothing a caller can see may move: every search here is compared byte for byte (counts, ids, distance bits) with the C
oracle and with the same search with pruning off, and scanned_points / pruned_points with a restatement of the round loop's pruning
rule on the oracle's sums (query_stats below) -- which the parent commit's kernels meet as well.

The index (d = 128, m = 8: the kernels of the flagship shape) has one list per (length, placement).  Lengths stand around the step
geometry -- a wave step is 256 points (64 lanes x 4 points: positions pb + {2 l, 2 l + 1, 128 + 2 l, 128 + 2 l + 1} of lane l), a
workgroup step 1024 --; on the placed lists the RANK of every row by the list's own query is prescribed by position (as in
tests/placement.py), so that the winners stand where an ordering bug shows:
  one_lane      ranks 0 .. in ONE lane's four points of a wave, then the same lane of the next wave, ...: ranks 1 .. 3 of the lane's sort
                carry winners
  reg3          winners only at register index 3 (position 128 + 2 l + 1 of a step)
  lone          one winner per lane, the lane's other three points are the list's WORST rows
  tied_*        the 130 best rows are copies of one row: equal sums inside a lane and across lanes, visit order decides
  descending    the best row is the list's last: the list ends inside a lane's four points with the winner in front of the end
Queries: one per list next to its centroid (probe 0 is the list; the later probes are pruned wherever a wave holds K keys) and one per
list half-way to another centroid (the second probe must be scanned)."""
import functools

import numpy as np
import pytest

import helpers
import list_end as le
import sequences as sq
import write_path as wp
from oracle import oracle as ora

pytestmark = pytest.mark.gpu
f32 = np.float32
D, M, KSUB = 128, 8, 256
KS = (1, 2, 4, 5, 10, 16, 17, 63, 64)
GEOMETRY = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
NTIED = 130
KEY_MAX = (1 << 64) - 1


def lane_points(wave, lane, step=0):
    """positions of the four register points of a lane in a wave's step (CodeRegs<8, 4>::point), register index 0 .. 3"""
    pb = (wave + 4 * step) * 256
    return [pb + 2 * lane, pb + 2 * lane + 1, pb + 128 + 2 * lane, pb + 128 + 2 * lane + 1]


def _rest(L, head, rng, tail=()):
    """ranks 0 .. at `head`, the worst ranks at `tail`, everything else shuffled between"""
    head, tail = [p for p in head if p < L], [p for p in tail if p < L]
    assert len(set(head) | set(tail)) == len(head) + len(tail)
    free = np.setdiff1d(np.arange(L), np.array(head + tail, np.int64))
    return np.concatenate([np.array(head, np.int64), rng.permutation(free), np.array(tail[::-1], np.int64)]).astype(np.int64)


def one_lane(L, rng):
    head = [p for wave in (1, 2, 3, 0) for step in (0, 1) for p in lane_points(wave, 7, step)]
    return _rest(L, head + [p for p in lane_points(1, 8)], rng)


def reg3(L, rng):
    return _rest(L, [lane_points(r % 4, (11 * (r // 4) + 3 * (r % 4)) % 64)[3] for r in range(80)], rng)


def lone(L, rng):
    lanes = [(r % 4, (5 * r + 2) % 64, r % 4) for r in range(64)]           # (wave, lane, register index) of rank r
    assert len({(wv, l) for wv, l, _ in lanes}) == 64
    head = [lane_points(wv, l)[r] for wv, l, r in lanes]
    tail = [p for wv, l, r in lanes for i, p in enumerate(lane_points(wv, l)) if i != r]
    return _rest(L, head, rng, tail)


def shuffled(L, rng):
    return rng.permutation(L)


def descending(L, rng):
    return L - 1 - np.arange(L)


# (name, length, placement, tied?)
LISTS = tuple(("len%d" % L, L, shuffled, False) for L in GEOMETRY) + (
    ("one_lane", 1025, one_lane, False), ("one_lane_short", 600, one_lane, False), ("reg3", 1025, reg3, False), ("lone", 1024, lone, False),
    ("tied_one_lane", 1025, one_lane, True), ("tied_shuffled", 1023, shuffled, True), ("tied_reg3", 257 + 768, reg3, True),
    ("descending1023", 1023, descending, False), ("descending257", 257, descending, False), ("descending66", 66, descending, False))


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case():
    """Built once, left unchanged.  qs[:kc]: the lists' own queries; qs[kc:]: the queries between two centroids."""
    kc = len(LISTS)
    rng = np.random.default_rng(6100)
    cent = rng.random((kc, D), dtype=f32)
    cbs = ((rng.random((M, KSUB, D // M), dtype=f32) - f32(0.5)) * f32(0.5)).astype(f32)
    labels = np.stack([rng.permutation(256)[:KSUB] for _ in range(M)]).astype(np.uint8)
    empty = ora.OracleIndex(cent, cbs, labels, np.zeros(kc + 1, np.int64), np.zeros((0, M), np.uint8), np.zeros(0, np.uint32))
    own = (cent + f32(0.05) * rng.standard_normal((kc, D)).astype(f32)).astype(f32)
    nxt = (np.arange(kc) + 1) % kc
    between = (f32(0.52) * cent + f32(0.48) * cent[nxt]).astype(f32)
    qs = np.ascontiguousarray(np.concatenate([own, between]), f32)
    probes, dcs = le.probes_of(cent, qs, kc)
    assert np.array_equal(probes[:kc, 0], np.arange(kc)) and np.array_equal(probes[kc:, 0], np.arange(kc)) and np.array_equal(probes[kc:, 1], nxt)
    codes = []
    for l, (name, L, fn, tied) in enumerate(LISTS):
        pool = np.stack([labels[i][rng.integers(0, KSUB, L)] for i in range(M)], 1).astype(np.uint8)
        sums = le.row_sums(empty, qs[l], l, dcs[l, 0], pool)
        by_rank = pool[np.lexsort((np.arange(L), sums))]
        if tied:
            by_rank[:NTIED] = by_rank[0]
        pi = np.asarray(fn(L, rng), np.int64)
        assert np.array_equal(np.sort(pi), np.arange(L)), name
        rows = np.zeros_like(by_rank)
        rows[pi] = by_rank
        codes.append(rows)
    offsets = np.zeros(kc + 1, np.int64)
    np.cumsum([L for _, L, _, _ in LISTS], out=offsets[1:])
    ids = rng.permutation(int(offsets[-1])).astype(np.uint32)
    c = Case()
    c.ref = ora.OracleIndex(cent, cbs, labels, offsets, np.ascontiguousarray(np.concatenate(codes)), ids)
    c.qs, c.kc, c.probes, c.dcs = qs, kc, probes, dcs
    c.lens = np.diff(offsets)
    c.sums = {}
    return c


def probe_keys(c, r, j):
    """the keys' high words (sum bits) of query r's probe of rank j, in position order"""
    if (r, j) not in c.sums:
        cl = int(c.probes[r, j])
        rows = c.ref.codes[c.ref.offsets[cl]:c.ref.offsets[cl + 1]]
        c.sums[(r, j)] = le.row_sums(c.ref, c.qs[r], cl, c.dcs[r, j], rows).view(np.uint32).astype(np.uint64)
    return c.sums[(r, j)]


def query_stats(c, r, K, w, pg, prune):
    """(probed points, pruned points, ranks scanned) of query r: the round loop of the query-major scan restated (kernels.hip.h,
    qscan_body).  The four waves of a workgroup take the 256-point steps of a list in turn, each with a selector of its own; the bound
    is the smallest K-th key any wave holds over what it has been offered so far (a wave's K smallest keys all pass: every published
    bound is some wave's K-th key of a subset of its points, so none lies below the smallest of the waves' true K-th keys).  Before a
    round the probes whose coarse distance bits exceed the bound's high word are dropped: the round's first ends the query, a later
    one is skipped alone.  Two probes per round: the first round takes probe 0 alone when dc[1] > 2 dc[0]."""
    lens = [int(c.lens[c.probes[r, j]]) for j in range(w)]
    dcb = [int(np.asarray(c.dcs[r, j], f32).view(np.uint32)) for j in range(w)]
    held = [[] for _ in range(4)]
    bound, pruned, scanned, base = KEY_MAX, 0, [], np.cumsum([0] + lens)

    def scan(j):
        nonlocal bound
        scanned.append(j)
        keys = (probe_keys(c, r, j) << np.uint64(32)) | (int(base[j]) + np.arange(lens[j])).astype(np.uint64)
        wave = (np.arange(lens[j]) // 256) % 4
        for v in range(4):
            held[v] = sorted(held[v] + keys[wave == v].tolist())[:K]
            if len(held[v]) >= K:
                bound = min(bound, held[v][K - 1])

    j0 = 0
    while j0 < w:
        step = pg
        js = [j for j in range(j0, min(w, j0 + pg))]
        live = {j: lens[j] for j in js}
        if prune:
            thi = bound >> 32
            if dcb[j0] > thi:
                pruned += sum(lens[j0:])
                break
            for j in js[1:]:
                if dcb[j] > thi and live[j]:
                    pruned += live[j]
                    live[j] = 0
            if pg == 2 and K <= 64 and j0 == 0 and w > 1 and live.get(1, 0) and c.dcs[r, 1] > f32(2.0) * c.dcs[r, 0]:
                live[1] = 0
                step = 1
        for j in js:
            if live[j]:
                scan(j)
        j0 += step
    return sum(lens), pruned, scanned


def pg_of(st):
    """probes per round of the latest query-major scan, from the LDS it was planned with"""
    for pg in (1, 2):
        if st["last_scan_lds"] == sq.scan_lds_bytes(M, D // M, KSUB, pg, 64, True, False, True):
            return pg
    raise AssertionError(st)


_STATE = {}


def handle(native):
    if "g" not in _STATE:
        c = case()
        g = wp.gpu_handle(native, c.ref)
        g.set_coarse_mode(1)
        g.set_tuning(-3, 0)          # query-major at every batch size, the stand-alone top-w (kc < 512: one wave per query)
        _STATE["g"] = g
        # the searches with pruning off run on a handle of their own: the plan's estimate of the pruned fraction (plan.h: PG1_MIN_PRUNED)
        # follows the scans of a handle, and one that prunes nothing would talk the first handle out of one probe per round
        off = wp.gpu_handle(native, c.ref)
        off.set_coarse_mode(1)
        off.set_tuning(-3, 0)
        off.set_pruning(0)
        _STATE["off"] = off
        _STATE["exp"] = {}
    return _STATE["g"]


def expected(K, w):
    c = case()
    if (K, w) not in _STATE["exp"]:
        _STATE["exp"][(K, w)] = c.ref.knn_search(c.qs, K, w, nthreads=ora.max_threads())
    return _STATE["exp"][(K, w)]


def checked_search(g, K, w, what):
    """one search with pruning on, one (on the second handle) with it off: the oracle's bytes both times, and the stats the restated round loop gives"""
    c = case()
    exp = expected(K, w)
    res, ran = {}, {}
    for prune in (1, 0):
        h = g if prune else _STATE["off"]
        h.reset_stats()
        res[prune] = h.search_raw(c.qs, K, w)
        st = h.get_stats()
        where = "%s, K=%d w=%d pruning %d" % (what, K, w, prune)
        assert st["last_qg"] == 0, (where, st)
        pg = pg_of(st)
        helpers.assert_same_results(res[prune], exp, what=where)
        model = [query_stats(c, r, K, w, pg, prune) for r in range(c.qs.shape[0])]
        print("%s: %d probes per round, scanned_points %d pruned_points %d" % (where, pg, st["scanned_points"], st["pruned_points"]))
        assert st["scanned_points"] == sum(m[0] for m in model), (where, st["scanned_points"], sum(m[0] for m in model))
        assert st["pruned_points"] == sum(m[1] for m in model), (where, st["pruned_points"], sum(m[1] for m in model))
        ran[prune] = (pg, model)
    assert all(np.array_equal(a, b) for a, b in zip(res[0], res[1])), what
    return ran[1]           # (probes per round, per-query model) of the search with pruning on


@pytest.mark.parametrize("K", KS)
def test_one_probe(native, K):
    """w = 1 plans one probe per round whatever the data: qscan_kernel<8, 16, 1>.  Lists of 1 and 63 points hold fewer than K = 64."""
    g = handle(native)
    pg, _ = checked_search(g, K, 1, "one probe")
    assert pg == 1


def test_later_probes_scanned_and_pruned(native):
    """w = 8.  One probe per round is planned once the handle has seen most probed points pruned (plan.h: PG1_MIN_PRUNED; the estimate
    follows the scans on the stream, every eighth): the batch is searched until the plan says so -- most of its probed points fall to
    pruning -- and then at every K.  The restated round loop must say that the queries between two centroids scan their second probe
    and that the lists' own queries lose theirs to pruning wherever the list gives a wave K points; the counters must be the model's."""
    c = case()
    g = handle(native)
    g.set_pruning(1)
    for K in KS:
        for i in range(64):
            g.search_raw(c.qs, 10, 8)
            if pg_of(g.get_stats()) == 1:
                break
        assert pg_of(g.get_stats()) == 1, "one probe per round was never planned: %s" % (g.get_stats(),)
        pg, model = checked_search(g, K, 8, "eight probes")
        assert pg == 1, "K=%d ran with two probes per round" % K
        own, between = model[:c.kc], model[c.kc:]
        assert all(1 in m[2] for m in between), "a query between two centroids must scan its second probe"
        if K <= 10:
            pruned_all = [m[2] == [0] for l, m in enumerate(own) if LISTS[l][1] >= 64]
            assert pruned_all and all(pruned_all), "a list's own query must lose its later probes to pruning"


def test_hinted_pair(native):
    """The index and a view of it, each search naming the next batch (ivfadc_set_next_queries): the scan carries the next batch's coarse
    tiles (qscan_coarse_kernel) and the hinted search starts from the finished rows, selected by the stand-alone top-w at one wave per
    query.  Stats as tests/test_gpu_parity.py::test_next_batch_coarse_rides_behind_the_scan expects them; the plain device entry first."""
    import torch
    c = case()
    g = handle(native)
    g.set_pruning(1)
    dev = torch.device("cuda:0")
    sets = [c.qs[:c.kc], c.qs[c.kc:]]
    qdev = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in sets]
    exp_of = {}

    def search(h, i, K, w, hint=None):
        nq = sets[i].shape[0]
        ids = torch.zeros(nq * K, dtype=torch.int32, device=dev)
        dist = torch.zeros(nq * K, dtype=torch.float32, device=dev)
        cnt = torch.zeros(nq, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        if hint is not None:
            h.set_next_queries(sets[hint].shape[0], qdev[hint].data_ptr(), 100 + hint)
        h.set_query_token(100 + i)
        h.search_device(nq, qdev[i].data_ptr(), K, w, ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
        torch.cuda.synchronize()
        st = h.get_stats()
        got = (ids.cpu().numpy().view(np.uint32).reshape(nq, K), dist.cpu().numpy().reshape(nq, K), cnt.cpu().numpy())
        if (i, K, w) not in exp_of:
            exp_of[(i, K, w)] = c.ref.knn_search(sets[i], K, w, nthreads=ora.max_threads())
        helpers.assert_same_results(got, exp_of[(i, K, w)], what="hinted pair: set %d K=%d w=%d hint=%s" % (i, K, w, hint))
        return st

    v = g.clone_view()
    v.set_coarse_mode(1)
    v.set_tuning(-3, 0)
    for h in (g, v):
        for K, w in ((10, 1), (64, 1), (1, 1), (10, 4), (17, 4)):
            st = search(h, 0, K, w)                                    # the plain device entry
            assert st["last_rider"] == 0 and st["coarse_prefetched"] == 0 and st["last_qg"] == 0, st
            st = search(h, 0, K, w, hint=1)
            assert st["last_rider"] == 1 and st["coarse_prefetched"] == 0, st
            st = search(h, 1, K, w, hint=0)                            # the hinted batch: its rows stand; it carries riders itself
            assert st["last_rider"] == 1 and st["coarse_prefetched"] == 1, st
            st = search(h, 0, K, w)
            assert st["last_rider"] == 0 and st["coarse_prefetched"] == 1, st
            if w == 1:
                assert pg_of(st) == 1, st
    del v


# ---- the stand-alone top-w -------------------------------------------------------------------------------------------------------------
TOPW_KC = (64, 65, 256, 1000, 1024, 1028)
TOPW_W = (1, 2, 8, 9, 32, 64)
TOPW_D = 16
LANE = 5                     # the lane whose share of a row holds the nearest centroids of the second query group


def lane_share(kc, lane=LANE):
    """the centroid numbers one lane of the wave holds of the first 1024 entries of a row read as float4s: u * 256 + 4 lane + e"""
    return [c for c in (u * 256 + 4 * lane + e for u in range(4) for e in range(4)) if c < kc]


@functools.lru_cache(maxsize=None)
def topw_case(kc, few_finite):
    """centroids and queries of one kc.  Query groups: random; next to a point P around which the centroids of ONE lane's share stand
    (the w nearest all in one lane where the share holds w); next to a centroid that exists four times (ties go to the lower id).
    few_finite: all but five centroids lie so far away that their distance overflows to +Inf: fewer than w finite entries."""
    rng = np.random.default_rng(6200 + kc + (1 if few_finite else 0))
    cent = rng.random((kc, TOPW_D), dtype=f32)
    P = (f32(3.0) + rng.random(TOPW_D, dtype=f32)).astype(f32)
    share = lane_share(kc)
    cent[share] = (P + f32(0.01) * rng.standard_normal((len(share), TOPW_D)).astype(f32)).astype(f32)
    dup = [i for i in (kc - 1, kc // 2 + 1, 9, 2) if i not in share]
    cent[dup] = cent[dup[0]]
    dup2 = [share[-1], share[0]]          # a tie inside the lane's share
    cent[dup2] = cent[dup2[0]]
    if few_finite:
        far = np.setdiff1d(np.arange(kc), np.array([1, kc // 3, share[0], kc - 2, kc - 1]))
        cent[far] = f32(3e19)
    return np.ascontiguousarray(cent), P, cent[dup[0]].copy()


def topw_queries(kc, few_finite, nq):
    cent, P, Q = topw_case(kc, few_finite)
    rng = np.random.default_rng(6300 + kc)
    qs = rng.random((nq, TOPW_D), dtype=f32)
    third = nq // 3
    qs[:third] = (P + f32(0.02) * rng.standard_normal((third, TOPW_D)).astype(f32)).astype(f32)
    qs[third:2 * third] = (Q + f32(0.001) * rng.standard_normal((third, TOPW_D)).astype(f32)).astype(f32)
    qs[0], qs[third] = P, Q
    return np.ascontiguousarray(qs, f32)


_TOPW = {}


@pytest.mark.parametrize("few_finite", [False, True])
@pytest.mark.parametrize("kc", TOPW_KC)
def test_topw(native, kc, few_finite):
    """ivfadc_coarse_search: the exact coarse kernel and topw_select_kernel, one wave per query below kc = 512 and, from 512 on, for
    batches of at least 32 queries per compute unit.  Cells and distance bits of the reference's stable top-w (ties to the lower cell)."""
    import torch
    cent, _, _ = topw_case(kc, few_finite)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    nq = 96 if kc < 512 else 32 * ncu
    qs = topw_queries(kc, few_finite, nq)
    cbs = np.zeros((2, 256, TOPW_D // 2), f32)
    labels = np.tile(np.arange(256, dtype=np.uint8), (2, 1))
    g = native.IVFADCIndex.from_arrays(cent, cbs, labels)
    g.set_coarse_mode(1)
    with np.errstate(over="ignore", invalid="ignore"):
        acc = le.coarse_sums(cent, qs)
    assert not np.isnan(acc).any()
    if few_finite:
        assert (np.isfinite(acc).sum(1) == 5).all()
    order = np.lexsort((np.broadcast_to(np.arange(kc), acc.shape), acc), axis=1)
    share = set(lane_share(kc))
    for w in TOPW_W:
        lists, dists = g.coarse_search_raw(qs, w)
        el = order[:, :w]
        ed = np.take_along_axis(acc, el, 1)
        what = "top-w kc=%d w=%d few_finite=%s" % (kc, w, few_finite)
        bad = np.nonzero((lists != el).any(1) | (np.ascontiguousarray(dists).view(np.uint32) != np.ascontiguousarray(ed).view(np.uint32)).any(1))[0]
        assert bad.size == 0, "%s: query %d: got %s %s, expected %s %s" % (what, bad[0], lists[bad[0]], dists[bad[0]], el[bad[0]], ed[bad[0]])
        if not few_finite and w <= len(share):
            assert set(el[0].tolist()) <= share, (what, "the w nearest of the first query must stand in one lane's share")
