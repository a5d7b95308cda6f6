"""Masked range search on the device (ivfadc_range_search_masked; csrc/range.hip.h): every stored point of the w probed lists with d <= r
that the query's mask selects, on handles with 8-bit and with UInt16 codes.

The model is tests/range_masked_ref.py (per query masked._knn over subset.filtered_lists with K = every stored point, cut at the radius);
tests/test_range_masked_model.py shows on the CPU that the table used here tells every wrong implementation of its MUTANTS from the right
one.  Every comparison is exact: lims, ids and distance BITS, no tolerance, no row left out.  The indexes hold 1956 points (a few thousand
in the shape tests); wall time per test is printed."""
import os
import threading
import time

import numpy as np
import pytest

import helpers
import masked as mk
import range_masked_ref as rm
import range_ref as rr
import subset as sb
import u16_ref
import write_path as wp

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_STATE = 2, 4
INF = np.float32(np.inf)
_G = {}


def setup_of(native, stride):
    """(handle, mask set) of the table's index: built once, never changed (tunings are set back by every test)"""
    if stride not in _G:
        c, _, _ = rm.case(stride)
        g = wp.gpu_handle(native, c.ref)
        ms = g.maskset(masks=list(rm.masks(stride)))
        assert len(ms) == 16
        _G[stride] = (g, ms)
    return _G[stride]


def assert_same(got, exp, what):
    assert np.array_equal(got[0], exp[0]), "%s: lims differ\n%s\n%s" % (what, got[0], exp[0])
    assert np.array_equal(got[1], exp[1]), "%s: ids differ (first at %d)" % (what, int(np.nonzero(got[1] != exp[1])[0][0]))
    gb, eb = np.asarray(got[2], np.float32).view(np.uint32), np.asarray(exp[2], np.float32).view(np.uint32)
    assert np.array_equal(gb, eb), "%s: distance bits differ (first at %d)" % (what, int(np.nonzero(gb != eb)[0][0]))


def refuses(call, code=ERR_STATE, match=None):
    from ivfadc_jl_amd import _native as nat
    with pytest.raises(nat.IVFADCError, match=match) as e:
        call()
    assert e.value.code == code, e.value


def ref_cut(ref, u16, qs, radii, w, n=None):
    """the definition over a reference index: its knn_search with K = every stored point, cut"""
    n = max(1, int(ref.offsets[-1])) if n is None else n
    knn = u16_ref.knn_one if u16 else helpers.numpy_knn
    return rr.pack([rr.cut(*knn(ref, qs[q], n, w), radii[q]) for q in range(qs.shape[0])])


# ---- 1. the case table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 64, 1024])
@pytest.mark.parametrize("stride", rm.STRIDES)
def test_case_table(native, stride, chunk):
    """every row of the table at every w: the default chunk, the smallest forced chunk (set_tuning(0, 1) is rounded up to 64: the
    1025-point list is 17 items) and 1024 (two items)"""
    t0 = time.time()
    g, ms = setup_of(native, stride)
    g.set_tuning(0, 1 if chunk == 64 else chunk)
    try:
        for w in rm.WS:
            qs, radii, moq = rm.queries(stride, w)
            assert_same(g.range_search_masked_raw(qs, radii, ms, moq, w), rm.expected(stride, w), "%s chunk=%d w=%d" % (stride, chunk, w))
    finally:
        g.set_tuning(0, 0)
    print("masked range table %s chunk=%d: %.2f s" % (stride, chunk, time.time() - t0))


# ---- 2. against the library itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["planned", "generic"])
@pytest.mark.parametrize("stride", rm.STRIDES)
def test_equals_the_masked_search_cut_on_the_host(native, stride, how):
    """search_masked_raw with K = N + 7, cut on the host: the generic path for UInt16 handles (whatever is asked), the masked list scan
    (planned) or set_tuning(-2, 0) (generic) for 8-bit ones"""
    g, ms = setup_of(native, stride)
    w = rm.KC
    qs, radii, moq = rm.queries(stride, w)
    c, own, _ = rm.case(stride)
    g.set_tuning(-2 if how == "generic" else 0, 0)
    try:
        ids, dd, cnt = g.search_masked_raw(c.qs, mk.K_ALL, ms, own, w=w)
    finally:
        g.set_tuning(0, 0)
    qis, _, _ = rm.table(stride, w)
    exp = rr.pack([rr.cut(ids[qi, :cnt[qi]], dd[qi, :cnt[qi]], r) for qi, r in zip(qis, radii)])
    assert_same(g.range_search_masked_raw(qs, radii, ms, moq, w), exp, "%s against search_masked_raw (%s)" % (stride, how))


@pytest.mark.parametrize("stride", rm.U8_STRIDES)
def test_equals_the_range_search_of_a_subset_view(native, stride):
    g, ms = setup_of(native, stride)
    c, _, _ = rm.case(stride)
    r = 12                                                # random_half, max_plus_1
    assert mk.MASKS[r][0] == "random_half"
    v = g.subset(mask=rm.masks(stride)[r])
    for w in (3, rm.KC):
        D = [rm.full_sorted(stride, qi, w, r)[1] for qi in range(rm.NQ)]
        radii = np.array([d[len(d) // 2] if len(d) else 1.0 for d in D], np.float32)
        radii[::5] = INF
        got = g.range_search_masked_raw(c.qs, radii, ms, np.full(rm.NQ, r, np.int32), w)
        assert got[0][-1] > 0
        assert_same(got, v.range_search_raw(c.qs, radii, w), "%s subset view w=%d" % (stride, w))


# ---- 3. maskset=None -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", rm.STRIDES)
def test_without_a_set(native, stride):
    """8-bit handles: byte-equal to range_search_raw; UInt16 handles: the reference, cut"""
    g, _ = setup_of(native, stride)
    c, _, _ = rm.case(stride)
    for w in (1, 3, rm.KC + 5):
        qs, radii, _ = rm.queries(stride, w)
        got = g.range_search_masked_raw(qs, radii, None, None, w)
        if c.u16:
            assert_same(got, rm.reference(stride, rm.table(stride, w)[0], radii, w, np.full(len(radii), -1)), "%s no set w=%d" % (stride, w))
        else:
            assert_same(got, g.range_search_raw(qs, radii, w), "%s no set w=%d" % (stride, w))
    refuses(lambda: g.range_search_masked_raw(qs, radii, None, np.zeros(len(radii), np.int32), 3), ERR_INVALID, "without a mask set")


@pytest.mark.parametrize("stride", rm.U16_STRIDES)
def test_u16_subset_view_without_a_set(native, stride):
    g, ms = setup_of(native, stride)
    c, _, _ = rm.case(stride)
    r = 12
    v = g.subset(mask=rm.masks(stride)[r])
    w = rm.KC
    radii = np.array([rm.full_sorted(stride, qi, w, r)[1][10] for qi in range(rm.NQ)], np.float32)
    radii[3] = INF
    exp = rm.reference(stride, np.arange(rm.NQ), radii, w, np.full(rm.NQ, r))
    assert_same(v.range_search_masked_raw(c.qs, radii, None, None, w), exp, "%s subset view, no set" % stride)
    refuses(lambda: v.range_search_masked_raw(c.qs, radii, ms, None, w), ERR_STATE, "subset view")


# ---- 4. UInt16 shapes the strides miss -------------------------------------------------------------------------------------------------
SHAPES = {   # seed, n, d, kc, m, ksub, permuted labels
    "dsub6_ksub300": (9401, 3000, 18, 6, 3, 300, True),          # the single-float gather
    "dsub1": (9402, 3000, 4, 6, 4, 300, True),
    "ksub65536": (9403, 3000, 8, 6, 2, 65536, True),
    "ksub200_perm": (9404, 3000, 32, 6, 8, 200, True),           # ksub <= 256 stored as UInt16, 16-bit labels
    "m48_d768": (9405, 2000, 768, 4, 48, 300, False),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_u16_shapes(native, shape):
    t0 = time.time()
    seed, n, d, kc, m, ksub, perm = SHAPES[shape]
    ref = u16_ref.make_index(seed, n, d, kc, m, ksub, perm_labels=perm, ndistinct=50)
    qs = np.random.default_rng(seed + 5).random((4, d), dtype=np.float32)
    g = wp.gpu_handle(native, ref)
    mask = np.random.default_rng(seed + 6).random(n) < 0.5
    fref = wp.ref_with_lists(ref, *sb.filtered_lists(ref.offsets, ref.codes, ref.ids, mask))
    ms = g.maskset(masks=[mask])
    w = 2
    for which, rf, moq in (("unmasked", ref, None), ("masked", fref, np.array([0, -1, 0, 0], np.int32))):
        rows, radii = [], []
        for q in range(4):
            use = ref if (moq is not None and moq[q] < 0) else rf
            i, D = u16_ref.knn_one(use, qs[q], n, w)
            r = INF if q == 3 else D[len(D) // 3]
            radii.append(r)
            rows.append(rr.cut(i, D, r))
        radii = np.array(radii, np.float32)
        for chunk in (0, 256):
            g.set_tuning(0, chunk)
            try:
                got = g.range_search_masked_raw(qs, radii, ms if moq is not None else None, moq, w)
            finally:
                g.set_tuning(0, 0)
            assert_same(got, rr.pack(rows), "%s %s chunk=%d" % (shape, which, chunk))
    print("u16 shape %s: %.2f s" % (shape, time.time() - t0))


# ---- 5. sub-batches and sort groups ------------------------------------------------------------------------------------------------------
WS_MIN = 1 << 20                 # set_workspace_limit(1): the limit's minimum


def plan_splits(tot, w, chunk):
    """csrc/range_plan.h restated for the table's index under the 1 MiB workspace: the sub-batches [a0, a1) of a masked batch whose queries
    hold tot[q] keys (make_plan: per_query_bytes, nb) and the sort groups [g0, g1) of each, relative to a0 (next_group: cap_keys)."""
    items = w * -(-max(mk.LENS) // chunk)
    per_query = rm.KC * 20 + w * 12 + items * 8 + 64 + 4
    nb = max(1, min(WS_MIN // per_query, ((1 << 31) - 1) // rm.KC, 65535, len(tot)))
    cap = max(WS_MIN // 24, 1 << 20)
    out = []
    for a0 in range(0, len(tot), nb):
        t = tot[a0:a0 + nb]
        groups, g0 = [], 0
        while g0 < len(t):
            g1, keys = g0, 0
            while g1 < len(t) and g1 - g0 < 65535 and (g1 == g0 or keys + t[g1] <= cap) and keys + t[g1] < (1 << 32):
                keys += t[g1]
                g1 += 1
            groups.append((g0, g1))
            g0 = g1
        out.append((a0, a0 + len(t), groups))
    return out


@pytest.mark.parametrize("stride", ["u8_m8", "u16_m8"])
def test_sub_batches_and_sort_groups_advance_the_mask_numbers(native, stride):
    """The table tiled x8 under set_workspace_limit at its minimum (1 MiB).  Leg 1, the smallest chunk: several sub-batches (a0 > 0).
    Leg 2, r = +inf at chunk 1024: a sub-batch holds more than cap_keys = 2^20 keys, so it is cut into several sort groups (g0 > 0 inside
    a sub-batch with a0 > 0 as well).  The plan's arithmetic is restated above and both splits are asserted, not assumed.  Rows are dealt
    so that neighbouring queries carry different mask numbers, across every sub-batch and sort-group boundary too: a launch that read
    its mask numbers from the batch's or the sub-batch's start would give other rows."""
    t0 = time.time()
    g, ms = setup_of(native, stride)
    w = rm.KC
    qs, radii, moq = rm.queries(stride, w)
    reps = 12
    # kind-major instead of query-major, the four unfiltered queries (3, 17, 18, 19) dealt between the others: every row's neighbours
    # are other queries with other mask numbers, also from one tile to the next
    qorder = np.array([17, 0, 18, 1, 19, 2] + [q for q in range(rm.NQ) if q not in (17, 0, 18, 1, 19, 2)])
    nk = len(rm.KINDS)
    perm = (qorder[None, :] * nk + np.arange(nk)[:, None]).ravel()
    assert sorted(perm.tolist()) == list(range(len(radii)))
    qs, radii, moq = qs[perm], radii[perm], moq[perm]
    Q, R, M = np.tile(qs, (reps, 1)), np.tile(radii, reps), np.tile(moq, reps)
    e = rm.expected(stride, w)
    rows = [(e[1][e[0][q]:e[0][q + 1]], e[2][e[0][q]:e[0][q + 1]]) for q in perm] * reps
    qis = np.tile(rm.table(stride, w)[0][perm], reps)
    assert len(np.unique(moq)) == 17 and (np.diff(M) != 0).all(), "no two neighbouring rows carry the same mask number"
    # leg 2's mask numbers: every second row unfiltered (1956 keys: enough keys), the others (all >= 0) their own mask moved on by 0, 5
    # or 10 from one block of 22 rows to the next, so that the sequence does not repeat with the table's period and neighbours differ
    shift = (np.arange(len(M)) // rm.NQ % 3) * 5
    M2 = np.where(np.arange(len(M)) % 2 == 0, -1, (M + shift) % 16).astype(np.int32)
    assert (M[1::2] >= 0).all() and (np.diff(M2) != 0).all()
    everything = [rm.full_sorted(stride, int(qi), w, int(r)) for qi, r in zip(qis, M2)]

    def differs_across(masks, at, base, what):
        """rows at - 1 and at carry different mask numbers, and the rows from `at` on are not the rows from `base` on: a launch that
        started reading its mask numbers at `base` would filter other points"""
        assert masks[at - 1] != masks[at] and not np.array_equal(masks[at:at + 8], masks[base:base + 8]), (what, at, base)

    split1 = plan_splits([len(i) for i, _ in rows], w, 64)
    assert len(split1) >= 2, "leg 1: the batch must not fit one sub-batch"
    for a0, _, _ in split1[1:]:
        differs_across(M, a0, 0, "sub-batch boundary")
    split2 = plan_splits([len(i) for i, _ in everything], w, 1024)
    cut = [(a0, groups) for a0, _, groups in split2 if len(groups) >= 2]
    assert cut and any(a0 > 0 for a0, _ in cut), "leg 2: a sub-batch behind the first must hold several sort groups: %s" % split2
    for a0, groups in cut:
        for g0, _ in groups[1:]:
            differs_across(M2, a0 + g0, a0, "sort-group boundary: + g0 dropped")
            if a0 > 0:
                differs_across(M2, a0 + g0, g0, "sort-group boundary: + a0 dropped")
            differs_across(M2, a0 + g0, 0, "sort-group boundary: both dropped")
    g.set_workspace_limit(1)
    try:
        g.set_tuning(0, 1)
        g.reset_stats()
        assert_same(g.range_search_masked_raw(Q, R, ms, M, w), rr.pack(rows), "sub-batched")
        assert g.get_stats()["scanned_points"] == Q.shape[0] * rm.N, "every probed point counts once, selected or not, whatever the passes"
        g.set_tuning(0, 1024)
        assert_same(g.range_search_masked_raw(Q, np.full(len(R), INF, np.float32), ms, M2, w), rr.pack(everything), "several sort groups")
    finally:
        g.set_tuning(0, 0)
        g.set_workspace_limit(8 << 30)
    print("masked range sub-batches %s: %d sub-batches; +inf leg: %s groups per sub-batch; %.2f s"
          % (stride, len(split1), [len(gr) for _, _, gr in split2], time.time() - t0))


# ---- 6. states -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", ["u8_m10", "u16_m5"])
def test_views_threads_and_refusals(native, stride):
    from ivfadc_jl_amd import index as ix
    c, own, _ = rm.case(stride)
    g = wp.gpu_handle(native, c.ref)                      # an index of this test's own: a partition is set below
    ms = g.maskset(masks=list(rm.masks(stride)))
    w = 3
    qs, radii, moq = rm.queries(stride, w)
    exp = rm.expected(stride, w)
    search = lambda h, s=ms, m=moq: h.range_search_masked_raw(qs, radii, s, m, w)
    assert_same(search(g), exp, "the index itself")
    v, v2 = g.clone_view(), g.clone_view()
    assert_same(search(v), exp, "a plain view with the index's set")
    out = {}
    th = [threading.Thread(target=lambda h=h, n=n: out.__setitem__(n, [search(h) for _ in range(3)])) for n, h in (("a", v), ("b", v2))]
    [t.start() for t in th]
    [t.join() for t in th]
    for n in ("a", "b"):
        assert len(out[n]) == 3
        for r in out[n]:
            assert_same(r, exp, "two threads on two views with one set, view " + n)
    # mask_of_query == None with a set: mask 0 for every query
    assert_same(search(g, m=None), search(g, m=np.zeros(len(radii), np.int32)), "None is mask 0")
    i0, d0 = ix.range_search_masked(g, qs[30], float(radii[30]), ms, int(moq[30]), w=w)
    assert i0.dtype == g.index_type and np.array_equal(i0, exp[1][exp[0][30]:exp[0][31]].astype(g.index_type)) and d0.dtype == np.float32
    # max_total
    total = int(exp[0][-1])
    assert total > 1
    assert_same(g.range_search_masked_raw(qs, radii, ms, moq, w, max_total=total), exp, "max_total == total")
    refuses(lambda: g.range_search_masked_raw(qs, radii, ms, moq, w, max_total=total - 1), ERR_INVALID, r"\b%d\b" % total)
    assert_same(search(g), exp, "the call after the refusal")
    # NaN and mask numbers outside [-1, nmasks) at the host entry: named, before any launch
    nan = radii.copy()
    nan[7] = np.nan
    refuses(lambda: g.range_search_masked_raw(qs, nan, ms, moq, w), ERR_INVALID, "query 7")
    bad = moq.copy()
    bad[9] = 16
    refuses(lambda: search(g, m=bad), ERR_INVALID, "query 9")
    bad[9] = -2
    refuses(lambda: search(g, m=bad), ERR_INVALID, "query 9")
    with pytest.raises(AssertionError, match="w >= 1"):
        ix.range_search_masked(g, qs[0], 1.0, ms, 0, w=0)
    lims, ids, dd = g.range_search_masked_raw(qs[:0], radii[:0], ms, moq[:0], w)
    assert lims.tolist() == [0] and len(ids) == 0 and len(dd) == 0
    # the refusals
    sv = g.subset(mask=rm.masks(stride)[4])
    refuses(lambda: search(sv), ERR_STATE, "subset view")
    other = wp.gpu_handle(native, c.ref)
    refuses(lambda: search(other), ERR_STATE, "another index")
    if not c.u16:                                          # (the list-partitioned mode serves UInt8 codes only)
        g.set_list_partition(2, 0)
        try:
            refuses(lambda: search(g), ERR_STATE, "list partition")
            refuses(lambda: search(g, s=None, m=None), ERR_STATE, "list partition")
        finally:
            g.set_list_partition(1, 0)
        assert_same(search(g), exp, "after the partition is lifted")
    # a mutator: the old set refuses on the index and on a view taken afterwards, the view taken before is stale; a new set serves
    g._append(c.qs[:1], np.array([mk.N + 100], np.uint32))
    refuses(lambda: search(g), ERR_STATE, "changed")
    refuses(lambda: search(g.clone_view()), ERR_STATE, "changed")
    refuses(lambda: search(v), ERR_STATE)
    ms_new = g.maskset(masks=[np.ones(mk.N + 101, bool)])
    got = g.range_search_masked_raw(c.qs, np.full(rm.NQ, INF, np.float32), ms_new, None, rm.KC)
    assert (np.diff(got[0]) == mk.N + 1).all()
    if not c.u16:
        assert_same(got, g.range_search_raw(c.qs, np.full(rm.NQ, INF, np.float32), rm.KC), "a new set after the mutation")


@pytest.mark.parametrize("state", ["appended", "lists_emptied"])
def test_after_push_and_delete_with_hostile_spare_capacity(native, state):
    """list_end's index: what lies behind list_len (stale rows a delete left, the zero slack) would be the best candidate of the list's own
    queries.  The set made before the change is refused; a new set answers as the reference over the new lists, filtered"""
    import list_end as le
    from test_gpu_list_end import Walker
    t0 = time.time()
    wk = Walker(native, "m8_d32")
    old = wk.g.maskset(masks=[np.ones(int(wk.lists[2].max()) + 1, bool)])
    wk.advance(state)
    n = int(wk.lists[0][-1])
    qs = np.ascontiguousarray(wk.case.qs[::le.QPL // 2])              # two queries per list
    refuses(lambda: wk.g.range_search_masked_raw(qs, np.ones(len(qs), np.float32), old, None, le.W), ERR_STATE, "changed")
    ids_now = wk.lists[2]
    top = int(ids_now.max()) + 1 if len(ids_now) else 1
    masks = [np.ones(top, bool), np.arange(top) % 2 == 0]
    ms = wk.g.maskset(masks=masks)
    frefs = [wp.ref_with_lists(wk.ref, *sb.filtered_lists(*wk.lists, mk_)) for mk_ in masks]
    moq = (np.arange(len(qs)) % 3 - 1).astype(np.int32)              # -1, 0, 1, ...
    rows, radii = [], []
    for q in range(qs.shape[0]):
        ref = wk.ref if moq[q] < 0 else frefs[moq[q]]
        i, D = helpers.numpy_knn(ref, qs[q], max(1, n), le.W)
        r = INF if q % 2 == 0 or len(D) == 0 else D[len(D) // 2]
        radii.append(r)
        rows.append(rr.cut(i, D, r))
    radii = np.array(radii, np.float32)
    for chunk in (0, 1):
        wk.g.set_tuning(0, chunk)
        try:
            assert_same(wk.g.range_search_masked_raw(qs, radii, ms, moq, le.W), rr.pack(rows), "%s chunk=%d" % (state, chunk))
        finally:
            wk.g.set_tuning(0, 0)
    print("masked range after %s: %.2f s" % (state, time.time() - t0))


def test_on_a_file_loaded_opq_index(native):
    """a search never reads the rotation: the :opq fixture (UInt16 ids, 8-bit codes) answers as its own masked search, cut"""
    idx = native.load_ivfadc_index(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "persistency_hand_f32_u16_opq.bin"))
    assert idx.rotated
    qs = np.random.default_rng(77).random((5, idx.d), dtype=np.float32)
    _, _, ids = idx._lists()
    mask = np.zeros(int(ids.max()) + 1, bool)
    mask[ids[::2]] = True
    ms = idx.maskset(masks=[mask])
    moq = np.array([0, 0, -1, 0, 0], np.int32)
    K = max(1, len(idx))
    full = idx.search_masked_raw(qs, K, ms, moq, w=idx.kc)
    radii = np.array([full[1][q, full[2][q] // 2] if full[2][q] else 1.0 for q in range(5)], np.float32)
    radii[-1] = INF
    exp = rr.pack([rr.cut(full[0][q, :full[2][q]], full[1][q, :full[2][q]], radii[q]) for q in range(5)])
    got = idx.range_search_masked_raw(qs, radii, ms, moq, idx.kc)
    assert_same(got, exp, "opq fixture")
    assert got[0][-1] - got[0][-2] == int(ms.kept[0]) > 0


def test_device_entry_and_result_life_cycle(native):
    import torch
    from ivfadc_jl_amd import index as ix
    stride = "u16_m8"
    g, ms = setup_of(native, stride)
    w = 3
    qs, radii, moq = rm.queries(stride, w)
    exp = rm.expected(stride, w)
    dq, dr, dm = torch.from_numpy(qs).cuda(), torch.from_numpy(radii).cuda(), torch.from_numpy(moq).cuda()
    torch.cuda.synchronize()
    nq = qs.shape[0]
    res = g.range_search_device_masked(nq, dq.data_ptr(), dr.data_ptr(), ms, dm.data_ptr(), w)
    res0 = g.range_search_device_masked(nq, dq.data_ptr(), dr.data_ptr(), ms, 0, w)           # null mask numbers: mask 0; two results alive
    g.search_raw(qs[:4], 10, 3)                                                              # a later search does not touch them
    assert ix.range_result_sizes(res) == (nq, int(exp[0][-1]))
    assert_same(ix.range_result_copy(res), exp, "device entry")
    assert_same(ix.range_result_copy(res0), g.range_search_masked_raw(qs, radii, ms, np.zeros(nq, np.int32), w), "device entry, null mask numbers")
    ix.range_result_destroy(res)
    ix.range_result_destroy(res0)
    # no set: the plain range search of a UInt16 handle, on device pointers
    res = g.range_search_device_masked(nq, dq.data_ptr(), dr.data_ptr(), None, 0, w)
    assert_same(ix.range_result_copy(res), g.range_search_masked_raw(qs, radii, None, None, w), "device entry, no set")
    ix.range_result_destroy(res)
    refuses(lambda: g.range_search_device_masked(nq, dq.data_ptr(), dr.data_ptr(), None, dm.data_ptr(), w), ERR_INVALID, "without a mask set")
    # a NaN radius at the device entry (a violated precondition): that query has no results, the others are untouched
    bad = radii.copy()
    bad[5] = np.nan
    dbad = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    res = g.range_search_device_masked(nq, dq.data_ptr(), dbad.data_ptr(), ms, dm.data_ptr(), w)
    lims, ids, dd = ix.range_result_copy(res)
    ix.range_result_destroy(res)
    assert lims[6] == lims[5]
    others = [(exp[1][exp[0][q]:exp[0][q + 1]], exp[2][exp[0][q]:exp[0][q + 1]]) if q != 5 else (exp[1][:0], exp[2][:0]) for q in range(nq)]
    assert_same((lims, ids, dd), rr.pack(others), "device entry, a NaN radius: that query empty, the others untouched")
    # mask numbers outside [-1, nmasks) are clamped: nothing outside the set is read, in-range rows are untouched
    wild = moq.copy()
    wild[0], wild[1] = 1000, -1000
    clamped = moq.copy()
    clamped[0], clamped[1] = 15, -1
    dw = torch.from_numpy(wild).cuda()
    torch.cuda.synchronize()
    res = g.range_search_device_masked(nq, dq.data_ptr(), dr.data_ptr(), ms, dw.data_ptr(), w)
    assert_same(ix.range_result_copy(res), g.range_search_masked_raw(qs, radii, ms, clamped, w), "device entry, clamped")
    ix.range_result_destroy(res)
    # a result outlives its handle and its set
    c, _, _ = rm.case(stride)
    g2 = wp.gpu_handle(native, c.ref)
    ms2 = g2.maskset(masks=list(rm.masks(stride)))
    res = g2.range_search_device_masked(nq, dq.data_ptr(), dr.data_ptr(), ms2, dm.data_ptr(), w)
    del ms2
    del g2
    assert_same(ix.range_result_copy(res), exp, "after the handle and the set are gone")
    ix.range_result_destroy(res)


# ---- 7. sequences ------------------------------------------------------------------------------------------------------------------------
def test_between_a_masked_search_and_a_plain_range_search(native):
    """one handle: masked top-K search (the masked list scan), masked range search, plain range search, masked top-K again.  The last_*
    stats still describe the top-K search; only scanned_points and queries move"""
    stride = "u8_m8"
    g, ms = setup_of(native, stride)
    c, own, _ = rm.case(stride)
    w = rm.KC
    qs, radii, moq = rm.queries(stride, w)
    g.set_tuning(4, 1024)
    try:
        top = g.search_masked_raw(c.qs, mk.K_REG, ms, own, w=w)
        before = g.get_stats()
        assert before["last_striped"] == 8 and before["last_qg"] == 4 and before["last_chunk"] == 1024, before
        got = g.range_search_masked_raw(qs, radii, ms, moq, w)
        after = g.get_stats()
        assert_same(got, rm.expected(stride, w), "masked range search behind a masked search")
        for key in ("last_qg", "last_chunk", "last_striped", "last_nf", "last_lb", "last_scan_lds", "last_scan_grid", "scan_launches"):
            assert after[key] == before[key], "a masked range search leaves %s as the last search set it" % key
        assert after["scanned_points"] - before["scanned_points"] == len(radii) * rm.N and after["queries"] - before["queries"] == len(radii)
        none = np.full(len(radii), -1, np.int32)
        plain = g.range_search_raw(qs, radii, w)
        assert_same(g.range_search_masked_raw(qs, radii, ms, none, w), plain, "-1 for every query is the plain range search")
        again = g.search_masked_raw(c.qs, mk.K_REG, ms, own, w=w)
        assert all(np.array_equal(x, y) for x, y in zip(top, again)), "the masked search behind the range searches"
        assert g.get_stats()["last_striped"] == 8
    finally:
        g.set_tuning(0, 0)
