"""Per-query filtered search on the device (ivfadc_maskset_create, ivfadc_search_masked; csrc/maskset.hip.h): one batch whose queries
carry different masks, tested inside the list scan.

The model is tests/masked.py (masked_reference: the reference over subset.filtered_lists per query); tests/test_masked_model.py shows on
the CPU that the read-back used here tells every wrong implementation of masked.MUTANTS from the right one.  A masked search is compared,
bit for bit, with the model, with the subset views of the same masks (a second oracle: ivfadc_clone_subset returns the same bytes by
contract) and, for the -1 rows, with the plain search.  The masked kernel (stats.last_striped == 8) and the masked generic path
(last_qg == -2) are two independent implementations of the same contract; both are held to it."""
import threading
import time

import numpy as np
import pytest

import helpers
import list_end as le
import masked as mk
import subset as sb
import u16_ref
import write_path as wp
from oracle import oracle as ora

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_STATE = 2, 4


def same(got, exp, what, u16=False):
    if u16:
        u16_ref.assert_exact(got, exp, what)
    else:
        helpers.assert_same_results(got, exp, what=what)


def rows(res, sel):
    return res[0][sel], res[1][sel], res[2][sel]


def refuses(call, code=ERR_STATE, match=None):
    from ivfadc_jl_amd import _native as nat
    with pytest.raises(nat.IVFADCError, match=match) as e:
        call()
    assert e.value.code == code, e.value


# ---- shared, built once and left unchanged -------------------------------------------------------------------------------------------
_G, _MODEL, _ORACLES = {}, {}, {}


def setup_of(native, stride):
    """(handle, mask set) of a case: the index with its 16 masks in ONE mask set"""
    if stride not in _G:
        g = wp.gpu_handle(native, mk.case(stride).ref)
        ms = g.maskset(masks=list(mk.masks(stride)))
        assert len(ms) == 16 and np.array_equal(ms.kept, mk.kept(stride)), (ms.kept, mk.kept(stride))
        _G[stride] = (g, ms)
    return _G[stride]


def model_of(stride, K, w=mk.KC):
    if (stride, K, w) not in _MODEL:
        _MODEL[(stride, K, w)] = mk.masked_reference(mk.case(stride), mk.masks(stride), mk.MASK_OF_QUERY, K, w)
    return _MODEL[(stride, K, w)]


def oracles_of(native, stride, K):
    """the second oracle: per query, the subset view of its mask (the plain search for -1), at the library's own plan"""
    if (stride, K) not in _ORACLES:
        c = mk.case(stride)
        g, _ = setup_of(native, stride)
        g.set_tuning(0, 0)
        out = []
        for qi, r in enumerate(mk.MASK_OF_QUERY):
            h = g if r < 0 else g.subset(mask=mk.masks(stride)[r])
            out.append(h.search_raw(c.qs[qi:qi + 1], K, mk.KC))
        _ORACLES[(stride, K)] = tuple(np.concatenate([o[i] for o in out]) for i in range(3))
    return _ORACLES[(stride, K)]


def check_all(native, stride, K, got, what):
    c = mk.case(stride)
    kept = mk.kept(stride)
    want = np.array([min(K, mk.N if r < 0 else kept[r]) for r in mk.MASK_OF_QUERY], np.int32)
    assert np.array_equal(got[2], want), "%s: counts %s, min(K, kept) %s" % (what, got[2], want)
    same(got, model_of(stride, K), what + ": the model", c.u16)
    same(got, oracles_of(native, stride, K), what + ": subset views (masked rows) and the plain search (-1 rows)", c.u16)


# ---- 1. read-back at the edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [mk.K_ALL, mk.K_REG])
@pytest.mark.parametrize("qg", [1, 2, 4])
@pytest.mark.parametrize("stride", mk.U8_STRIDES)
def test_read_back_at_the_edges(native, stride, qg, K):
    """w = kc, chunk 1024 (the 1025-point list makes two work items), every forced width: K = 1963 returns every selected entry of every
    mask through the LDS selectors, K = 64 through the register selectors."""
    t0 = time.time()
    c = mk.case(stride)
    g, ms = setup_of(native, stride)
    oracles_of(native, stride, K)                       # (before the tuning is forced)
    g.set_tuning(qg, 1024)
    try:
        got = g.search_masked_raw(c.qs, K, ms, mk.MASK_OF_QUERY, w=mk.KC)
        st = g.get_stats()
    finally:
        g.set_tuning(0, 0)
    what = "%s qg=%d K=%d" % (stride, qg, K)
    assert st["last_striped"] == 8 and st["last_qg"] == mk.forced_qg(stride, K, qg) and st["last_chunk"] == 1024, (what, st)
    check_all(native, stride, K, got, what)
    print("masked read-back %s: %.2f s" % (what, time.time() - t0))


# ---- 2. the generic path: the independent second implementation ----------------------------------------------------------------------
@pytest.mark.parametrize("how", ["K = 2500", "set_tuning(-2, 0)"])
@pytest.mark.parametrize("stride", mk.U8_STRIDES)
def test_generic_path_8bit(native, stride, how):
    c = mk.case(stride)
    g, ms = setup_of(native, stride)
    K = 2500 if how.startswith("K") else mk.K_REG
    oracles_of(native, stride, K)
    g.set_tuning(0 if how.startswith("K") else -2, 0)
    try:
        got = g.search_masked_raw(c.qs, K, ms, mk.MASK_OF_QUERY, w=mk.KC)
        st = g.get_stats()
    finally:
        g.set_tuning(0, 0)
    assert st["last_qg"] == -2, st
    check_all(native, stride, K, got, "%s generic (%s)" % (stride, how))


@pytest.mark.parametrize("K", [mk.K_ALL, mk.K_REG])
@pytest.mark.parametrize("stride", mk.U16_STRIDES)
def test_generic_path_u16(native, stride, K):
    """every UInt16 handle takes the masked generic path, whatever K"""
    c = mk.case(stride)
    g, ms = setup_of(native, stride)
    got = g.search_masked_raw(c.qs, K, ms, mk.MASK_OF_QUERY, w=mk.KC)
    assert g.get_stats()["last_qg"] == -2
    check_all(native, stride, K, got, "%s K=%d" % (stride, K))


# ---- 3. small K and exact pruning ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clustered(native):
    """Well separated cells (centroids x 4, points within 0.1 of theirs), queries next to stored points: the K-th best key of a query's own
    cell lies below the coarse distance of every other cell, so exact pruning skips them -- once the bound has been published.  4096
    queries x w = 3 are 12 288 work items at one query per code stream, several times what the chip holds at once: the items of the
    farther cells start after those of the closest ones have finished."""
    kc, n, d, m, nq = 40, 6000, 32, 8, 4096
    rng = np.random.default_rng(4711)
    cent, cbs, labels = helpers.make_quantizers(77, d, kc, m, 256, scale=0.05)
    cent = (cent * np.float32(4.0)).astype(np.float32)
    assign = rng.integers(0, kc, n)
    data = (cent[assign] + (rng.random((n, d), dtype=np.float32) - np.float32(0.5)) * np.float32(0.1)).astype(np.float32)
    tmp = ora.OracleIndex(cent, cbs, labels, np.zeros(kc + 1, np.int64), np.zeros((0, m), np.uint8), np.zeros(0, np.uint32))
    lst, codes = tmp.encode(data)
    order = np.argsort(lst, kind="stable")
    offsets = np.zeros(kc + 1, np.int64)
    np.cumsum(np.bincount(lst, minlength=kc), out=offsets[1:])
    oidx = ora.OracleIndex(cent, cbs, labels, offsets, np.ascontiguousarray(codes[order]), order.astype(np.uint32))
    qs = (data[rng.integers(0, n, nq)] + np.float32(0.01)).astype(np.float32)
    mrng = np.random.default_rng(12)
    masks = [mrng.random(n) < 0.5, mrng.random(n) < 0.9, np.arange(n) % 3 == 0]
    moq = (np.arange(nq) % 4 - 1).astype(np.int32)          # -1, 0, 1, 2, ...
    g = wp.gpu_handle(native, oidx)
    return oidx, qs, masks, moq, g, g.maskset(masks=masks)


def _oracle_masked(oidx, qs, masks, moq, K, w):
    """the C oracle over the filtered lists, one call per mask"""
    ids = np.zeros((len(qs), K), np.uint32)
    dists = np.full((len(qs), K), np.inf, np.float32)
    counts = np.zeros(len(qs), np.int32)
    for r in np.unique(moq):
        ref = oidx if r < 0 else wp.ref_with_lists(oidx, *sb.filtered_lists(oidx.offsets, oidx.codes, oidx.ids, masks[r]))
        sel = np.nonzero(moq == r)[0]
        i, dd, cc = ref.knn_search(qs[sel], K, w, nthreads=ora.max_threads())
        ids[sel], dists[sel], counts[sel] = i, dd, cc
    return ids, dists, counts


@pytest.mark.parametrize("K", [1, 10])
def test_small_k_and_pruning(native, clustered, K):
    oidx, qs, masks, moq, g, ms = clustered
    exp = _oracle_masked(oidx, qs, masks, moq, K, 3)
    res = {}
    for qg in (1, 4):
        for on in (1, 0):
            g.set_pruning(on)
            g.set_tuning(qg, 1024)
            g.reset_stats()
            try:
                res[(qg, on)] = g.search_masked_raw(qs, K, ms, moq, w=3)
                st = g.get_stats()
            finally:
                g.set_tuning(0, 0)
                g.set_pruning(1)
            what = "clustered K=%d qg=%d pruning=%d" % (K, qg, on)
            assert st["last_striped"] == 8 and st["last_qg"] == qg, (what, st)
            helpers.assert_same_results(res[(qg, on)], exp, what=what)
            if on == 0:
                assert st["pruned_points"] == 0, (what, st)
            elif qg == 1:           # rank-major items: the test cannot pass with pruning idle
                assert 0 < st["pruned_points"] < st["scanned_points"], (what, st)
        assert all(np.array_equal(x, y) for x, y in zip(res[(qg, 0)], res[(qg, 1)]))


# ---- 4. hostile spare capacity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutated", [True, False])
def test_hostile_spare_capacity(native, mutated):
    """tests/list_end.py's index: behind list_len lie decoys that would be every query's best candidate -- deleted in place and partly
    overwritten by an in-place append (mutated), or the zero slack of a never-mutated index.  A mask set made AFTER the mutations from an
    all-ones bitmap selects every stored id, the stale ones included: the bits behind list_len must be 0 all the same.  A decoy's sum is
    about 2 dc, far below every live point's: one that got through would be the first result and differ from the reference, which
    holds none."""
    from test_gpu_list_end import Walker
    wk = Walker(native, "m8_d32", mutated=mutated)
    g, qs = wk.g, wk.case.qs
    if mutated:
        # positive control, while the decoys are live: a masked search returns them first (a decoy that got through later would show)
        ms0 = g.maskset(masks=[np.ones(int(wk.lists[2].max()) + 1, bool)])
        first = g.search_masked_raw(qs, 1, ms0, None, w=le.W)[0][:, 0]
        assert all(first[r] in wk.case.decoys[r // le.QPL] for r in range(len(qs))), "the live decoys are every query's best candidate"
        wk.advance("appended")
        refuses(lambda: g.search_masked_raw(qs, 1, ms0, None, w=le.W), ERR_STATE, "changed")
    ids_now = wk.lists[2]         # (the deletion renumbered the ids, as delete_from_index! does: a decoy is told by its sum, not its id)
    top = int(ids_now.max()) + 1
    ms = g.maskset(masks=[np.ones(top, bool)])
    assert ms.kept[0] == len(ids_now) == len(g)
    for K in (1, 10, 64):
        for qg in (1, 4):
            g.set_tuning(0, 0)
            plain = g.search_raw(qs, K, le.W)
            g.set_tuning(qg, 1024)
            try:
                got = g.search_masked_raw(qs, K, ms, None, w=le.W)
                assert g.get_stats()["last_striped"] == 8
            finally:
                g.set_tuning(0, 0)
            what = "hostile (%s) K=%d qg=%d" % ("mutated" if mutated else "never mutated", K, qg)
            helpers.assert_same_results(got, plain, what=what)
            helpers.assert_same_results(got, wk.expected(K), what=what + ": the reference")
        g.set_tuning(-2, 0)
        try:
            helpers.assert_same_results(g.search_masked_raw(qs, K, ms, None, w=le.W), plain, what="hostile, generic K=%d" % K)
        finally:
            g.set_tuning(0, 0)


# ---- 5. device entries -----------------------------------------------------------------------------------------------------------------
def test_device_entries(native):
    """bitmaps, mask_of_query and outputs in device memory (torch); asynchronous, followed by ivfadc_sync; the host entries' bytes"""
    import torch
    stride, K = "u8_m10", mk.K_REG
    c = mk.case(stride)
    g, ms = setup_of(native, stride)
    nbits = max(len(x) for x in mk.masks(stride))
    bits = np.zeros((16, (nbits + 31) // 32), np.uint32)
    for r, x in enumerate(mk.masks(stride)):
        wds = sb.pack(x)
        bits[r, :len(wds)] = wds
    dev = "cuda:0"
    dbits = torch.from_numpy(bits.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    ms2 = g.maskset_device(dbits.data_ptr(), 16, nbits)
    assert np.array_equal(ms2.kept, ms.kept)
    host = g.search_masked_raw(c.qs, K, ms, mk.MASK_OF_QUERY, w=mk.KC)
    dq = torch.from_numpy(c.qs).to(dev)
    dm = torch.from_numpy(mk.MASK_OF_QUERY).to(dev)
    di = torch.zeros((mk.NQ, K), dtype=torch.int32, device=dev)
    dd = torch.zeros((mk.NQ, K), dtype=torch.float32, device=dev)
    dc = torch.zeros(mk.NQ, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for which, (set_, moq_ptr, exp) in {"device set": (ms2, dm.data_ptr(), host),
                                        "null mask_of_query": (ms2, 0, g.search_masked_raw(c.qs, K, ms, None, w=mk.KC))}.items():
        g.search_device_masked(set_, mk.NQ, dq.data_ptr(), K, mk.KC, moq_ptr, di.data_ptr(), dd.data_ptr(), dc.data_ptr())
        g.sync()
        got = (di.cpu().numpy().view(np.uint32), dd.cpu().numpy(), dc.cpu().numpy())
        helpers.assert_same_results(got, exp, what="device entry, " + which)
    # a violated precondition is clamped into [-1, nmasks): nothing outside the set is read, in-range rows are untouched
    bad = mk.MASK_OF_QUERY.copy()
    bad[0], bad[1] = 1000, -1000
    dm2 = torch.from_numpy(bad).to(dev)
    torch.cuda.synchronize()
    g.search_device_masked(ms2, mk.NQ, dq.data_ptr(), K, mk.KC, dm2.data_ptr(), di.data_ptr(), dd.data_ptr(), dc.data_ptr())
    g.sync()
    got = (di.cpu().numpy().view(np.uint32), dd.cpu().numpy(), dc.cpu().numpy())
    helpers.assert_same_results(rows(got, slice(2, None)), rows(host, slice(2, None)), what="device entry, clamped rows aside")
    clamped = mk.MASK_OF_QUERY.copy()
    clamped[0], clamped[1] = 15, -1
    helpers.assert_same_results(got, g.search_masked_raw(c.qs, K, ms, clamped, w=mk.KC), what="device entry, clamped")


# ---- 6. sub-batches --------------------------------------------------------------------------------------------------------------------
def test_sub_batches_advance_the_mask_numbers(native):
    """The planner never cuts a sub-batch below 64 queries, so the 20 queries are dealt ten times over: 200 queries under a 1 MB workspace
    at K = 1963 run as 64 + 64 + 64 + 8.  Query q of every round must see ITS mask: the mask numbers advance with the sub-batch."""
    stride, K, reps = "u8_m8", mk.K_ALL, 10
    c = mk.case(stride)
    g, ms = setup_of(native, stride)
    qs = np.tile(c.qs, (reps, 1))
    moq = np.tile(mk.MASK_OF_QUERY, reps)
    m = model_of(stride, K)
    exp = tuple(np.concatenate([x] * reps) for x in m)
    g.set_workspace_limit(1 << 20)
    g.set_profiling(1)
    g.reset_stats()
    try:
        got = g.search_masked_raw(qs, K, ms, moq, w=mk.KC)
        st = g.get_stats()
    finally:
        g.set_profiling(0)
        g.set_workspace_limit(8 << 30)
    assert st["last_striped"] == 8 and st["scan_launches"] >= 3, st
    helpers.assert_same_results(got, exp, what="sub-batched")


def test_generic_path_batches_and_sort_groups_advance_the_mask_numbers(native):
    """The masked generic path cut twice over.  Under the smallest workspace (1 MB) a stage-A batch holds 2^20 / (kc * 20 + w * 12 + 64) =
    2340 queries at kc = w = 12, and a sort group 2^20 keys -- 536 queries of 1956 probed points each (a rejected point still leaves a
    key).  2400 queries run as two stage-A batches (2340 + 60), the first in five sort groups: the dump, and with it the mask numbers,
    start at queries 536, 1072, 1608, 2144 and 2340.  The queries are drawn, not tiled, so that no cut falls on a period of the mask
    numbers: a slice that forgot to advance them would filter by another query's mask."""
    stride, K, nq = "u8_m8", mk.K_REG, 2400
    c = mk.case(stride)
    g, ms = setup_of(native, stride)
    pick = np.random.default_rng(536).integers(0, mk.NQ, nq)
    for cut in (536, 1072, 1608, 2144, 2340):
        assert mk.MASK_OF_QUERY[pick[cut]] != mk.MASK_OF_QUERY[pick[0]] and not np.array_equal(pick[cut:cut + 60], pick[:60]), cut
    exp = tuple(x[pick] for x in model_of(stride, K))
    g.set_workspace_limit(1 << 20)
    g.set_tuning(-2, 0)
    try:
        got = g.search_masked_raw(c.qs[pick], K, ms, mk.MASK_OF_QUERY[pick], w=mk.KC)
        st = g.get_stats()
    finally:
        g.set_tuning(0, 0)
        g.set_workspace_limit(8 << 30)
    assert st["last_qg"] == -2, st
    helpers.assert_same_results(got, exp, what="masked generic path, stage-A batches and sort groups")


# ---- 7. life cycle ---------------------------------------------------------------------------------------------------------------------
def test_life_cycle(native):
    """what each call on a mask set must do (include/ivfadc_hip.h, "h and s")"""
    from ivfadc_jl_amd import index as ix
    stride, K = "u8_m3", mk.K_REG
    c = mk.case(stride)
    g = wp.gpu_handle(native, c.ref)                      # an index of this test's own: it is mutated below
    ms = g.maskset(masks=list(mk.masks(stride)))
    exp = model_of(stride, K)
    search = lambda h, s=ms, moq=mk.MASK_OF_QUERY, k=K, w=mk.KC: h.search_masked_raw(c.qs, k, s, moq, w=w)
    helpers.assert_same_results(search(g), exp, what="the index itself")
    # a plain view of the index: served -- and two handles search with ONE set at the same time
    v = g.clone_view()
    helpers.assert_same_results(search(v), exp, what="a plain view")
    out = {}
    th = [threading.Thread(target=lambda h=h, n=n: out.__setitem__(n, [search(h) for _ in range(4)])) for n, h in (("g", g), ("v", v))]
    [t.start() for t in th]
    [t.join() for t in th]
    for n in ("g", "v"):
        for r in out[n]:
            helpers.assert_same_results(r, exp, what="concurrent searches with one set, handle " + n)
    # w > kc is clamped as ivfadc_search clamps it; K < 1 and w < 1 are the reference's assertions
    helpers.assert_same_results(search(g, w=mk.KC + 5), exp, what="w > kc")
    with pytest.raises(AssertionError, match="k >= 1"):
        search(g, k=0)
    with pytest.raises(AssertionError, match="w >= 1"):
        search(g, w=0)
    assert ix.knn_search_masked(g, c.qs[0], 5, ms, int(mk.MASK_OF_QUERY[0]), w=mk.KC)[0].tolist() == exp[0][0, :min(5, exp[2][0])].tolist()
    # mask numbers outside [-1, nmasks): refused before any launch, naming the query
    bad = mk.MASK_OF_QUERY.copy()
    bad[7] = 16
    refuses(lambda: search(g, moq=bad), ERR_INVALID, "query 7")
    bad[7] = -2
    refuses(lambda: search(g, moq=bad), ERR_INVALID, "query 7")
    # a subset view has lists of its own; a mask set is made from the index itself
    sv = g.subset(mask=mk.masks(stride)[4])
    refuses(lambda: search(sv), ERR_STATE, "subset view")
    refuses(lambda: v.maskset(masks=[np.ones(4, bool)]), ERR_STATE, "take it from the index itself")
    refuses(lambda: sv.maskset(masks=[np.ones(4, bool)]), ERR_STATE, "take it from the index itself")
    # another index, even one with the same lists
    other = wp.gpu_handle(native, c.ref)
    refuses(lambda: search(other), ERR_STATE, "another index")
    helpers.assert_same_results(search(other, s=other.maskset(masks=list(mk.masks(stride)))), exp, what="the other index with a set of its own")
    # a list partition
    g.set_list_partition(2, 0)
    try:
        refuses(lambda: search(g), ERR_STATE, "list partition")
    finally:
        g.set_list_partition(1, 0)
    helpers.assert_same_results(search(g), exp, what="after the partition is lifted")
    # the empty mask (nbits == 0, no bitmap) and a mask by ids
    empty = g.maskset(ids=[np.zeros(0, np.int64), c.ref.ids[:5]])
    assert empty.kept.tolist() == [0, 5]
    r0 = search(g, s=empty, moq=np.zeros(mk.NQ, np.int32))
    assert (r0[2] == 0).all()
    r1 = search(g, s=empty, moq=np.ones(mk.NQ, np.int32))
    assert (r1[2] == 5).all() and all(sorted(r1[0][q, :5].tolist()) == sorted(c.ref.ids[:5].tolist()) for q in range(mk.NQ))
    # any mutator: the set refuses from then on (on the index and on a view taken afterwards); a new one serves
    g._append(c.qs[:1], np.array([mk.N + 100], np.uint32))
    refuses(lambda: search(g), ERR_STATE, "changed")
    v2 = g.clone_view()
    refuses(lambda: search(v2), ERR_STATE, "changed")
    ms_new = g.maskset(masks=[np.ones(mk.N + 101, bool)])
    assert ms_new.kept[0] == mk.N + 1 == len(g)
    helpers.assert_same_results(search(g, s=ms_new, moq=None), g.search_raw(c.qs, K, mk.KC), what="a new set after the mutation")
    # destroying in either order
    del ms, empty
    del g


def test_device_synthesised_lists(native):
    """ids are positions where the lists were synthesised on the device: the build reads none, and the id is what a search returns"""
    c = mk.case("u8_m8")
    g = wp.gpu_handle(native, c.ref, with_lists=False)
    g.synth_lists(c.ref.offsets, 99)
    K = 40
    plain = g.search_raw(c.qs, K, mk.KC)
    ones = g.maskset(masks=[np.ones(1 << 16, bool)])     # (positions count the spare capacity in front of them)
    assert ones.kept[0] == mk.N
    helpers.assert_same_results(g.search_masked_raw(c.qs, K, ones, None, w=mk.KC), plain, what="synthesised lists, all ones")
    # keep exactly what the plain search of query 0 returned, minus its best: the best of the rest comes first
    keep = plain[0][0, 1:plain[2][0]]
    ms = g.maskset(ids=[keep])
    got = g.search_masked_raw(c.qs[:1], K, ms, None, w=mk.KC)
    assert got[2][0] == len(keep) and np.array_equal(got[0][0, :len(keep)], keep)
    assert np.array_equal(got[1][0, :len(keep)].view(np.uint32), plain[1][0, 1:plain[2][0]].view(np.uint32))
