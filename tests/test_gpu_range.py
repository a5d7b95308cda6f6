"""Range search on the device (ivfadc_range_search; csrc/range.hip.h): every stored point of the w probed lists with d <= r.

The model is tests/range_ref.py (range_reference: knn_search with K = every stored point, cut at the radius); tests/test_range_model.py
shows on the CPU that the table used here tells every wrong implementation of range_ref.MUTANTS from the right one.  Every comparison is
exact: lims, ids and distance BITS, no tolerance, no row left out.  Wall time per test is printed."""
import os
import time

import numpy as np
import pytest

import helpers
import masked as mk
import range_ref as rr
import subset as sb
import write_path as wp

pytestmark = pytest.mark.gpu
ERR_INVALID, ERR_STATE = 2, 4
INF = np.float32(np.inf)
_G = {}


def handle(native, stride):
    """the table's index on the device: built once, never changed (tunings are set back by every test)"""
    if stride not in _G:
        ref, _ = rr.case(stride)
        _G[stride] = wp.gpu_handle(native, ref)
    return _G[stride]


def assert_same(got, exp, what):
    assert np.array_equal(got[0], exp[0]), "%s: lims differ\n%s\n%s" % (what, got[0], exp[0])
    assert np.array_equal(got[1], exp[1]), "%s: ids differ (first at %d)" % (what, int(np.nonzero(got[1] != exp[1])[0][0]))
    gb, eb = np.asarray(got[2], np.float32).view(np.uint32), np.asarray(exp[2], np.float32).view(np.uint32)
    assert np.array_equal(gb, eb), "%s: distance bits differ (first at %d)" % (what, int(np.nonzero(gb != eb)[0][0]))


def cut_of_search(g, qs, radii, w):
    """the definition, through the library's own knn_search: search_raw with K = every stored point, cut at d <= r"""
    K = max(1, len(g))
    ids, dd, cnt = g.search_raw(qs, K, w)
    return rr.pack([rr.cut(ids[q, :cnt[q]], dd[q, :cnt[q]], radii[q]) for q in range(qs.shape[0])])


# ---- 1. the case table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 64, 1024])
@pytest.mark.parametrize("stride", rr.STRIDES)
def test_case_table(native, stride, chunk):
    """every row of the table at every w: the default chunk (one work item per list), the smallest forced chunk (set_tuning(0, 1) is
    rounded up to 64: the 1025-point list is 17 items) and the table's own 1024 (two items)"""
    t0 = time.time()
    g = handle(native, stride)
    g.set_tuning(0, 1 if chunk == 64 else chunk)
    try:
        for w in rr.WS:
            qs, radii = rr.queries(stride, w)
            assert_same(g.range_search_raw(qs, radii, w), rr.expected(stride, w), "%s chunk=%d w=%d" % (stride, chunk, w))
    finally:
        g.set_tuning(0, 0)
    print("range table %s chunk=%d: %.2f s" % (stride, chunk, time.time() - t0))


@pytest.mark.parametrize("stride", rr.STRIDES)
def test_equals_knn_search_at_the_tenth_neighbour(native, stride):
    """r = D[9]: the result is search_raw(K = count) -- ids bit-exact, distances bit-identical, ties at D[9] included"""
    g = handle(native, stride)
    _, qs = rr.case(stride)
    w = 3
    radii = np.array([rr.full_sorted(stride, qi, w)[1][9] for qi in range(rr.NQ)], np.float32)
    lims, ids, dd = g.range_search_raw(qs, radii, w)
    for qi in range(rr.NQ):
        cnt = int(lims[qi + 1] - lims[qi])
        assert cnt >= 10
        ki, kd, kc = g.search_raw(qs[qi:qi + 1], cnt, w)
        assert kc[0] == cnt and np.array_equal(ki[0], ids[lims[qi]:lims[qi + 1]])
        assert np.array_equal(kd[0].view(np.uint32), dd[lims[qi]:lims[qi + 1]].view(np.uint32))
        if cnt < len(rr.full_sorted(stride, qi, w)[1]):
            assert rr.full_sorted(stride, qi, w)[1][cnt] > radii[qi]


# ---- 2. index states ---------------------------------------------------------------------------------------------------------------------
def test_on_a_clone_view(native):
    g = handle(native, "u8_m8")
    v = g.clone_view()
    qs, radii = rr.queries("u8_m8", rr.KC)
    assert_same(v.range_search_raw(qs, radii, rr.KC), rr.expected("u8_m8", rr.KC), "clone_view")
    assert_same(g.range_search_raw(qs, radii, rr.KC), rr.expected("u8_m8", rr.KC), "the index, its view alive")


@pytest.mark.parametrize("kind", ["every_other", "random_half", "last_only"])
def test_on_a_subset_view(native, kind):
    """against the reference over the FILTERED lists (subset.filtered_lists)"""
    stride = "u8_m10"
    g = handle(native, stride)
    ref, qs = rr.case(stride)
    mask, _ = mk.case(stride).mask(kind, "max_plus_1")
    fref = wp.ref_with_lists(ref, *sb.filtered_lists(ref.offsets, ref.codes, ref.ids, mask))
    v = g.subset(mask=mask)
    for w in (3, rr.KC):
        rows, radii = [], []
        for qi in range(rr.NQ):
            D = helpers.numpy_knn(fref, qs[qi], rr.N, w)[1]
            for r in ((D[len(D) // 2], INF) if len(D) else (np.float32(1.0), INF)):
                radii.append(r)
                rows.append(rr.range_reference(fref, qs[qi], r, w))
        radii = np.array(radii, np.float32)
        assert_same(v.range_search_raw(np.repeat(qs, 2, axis=0), radii, w), rr.pack(rows), "subset view %s w=%d" % (kind, w))


@pytest.mark.parametrize("state", ["appended", "lists_emptied"])
def test_after_push_and_delete_with_hostile_spare_capacity(native, state):
    """list_end's index: what lies behind list_len (stale rows a delete left, the zero slack) would be the best candidate of the list's own
    queries; at r = +inf every probed point comes back and nothing else, at a finite radius the prefix"""
    import list_end as le
    from test_gpu_list_end import walker
    t0 = time.time()
    wk = walker(native, "m8_d32", state)
    n = int(wk.lists[0][-1])
    qs = np.ascontiguousarray(wk.case.qs[::le.QPL // 2])              # two queries per list
    rows, radii = [], []
    for q in range(qs.shape[0]):
        i, D = helpers.numpy_knn(wk.ref, qs[q], n, le.W)
        r = INF if q % 2 == 0 or len(D) == 0 else D[len(D) // 2]
        radii.append(r)
        rows.append(rr.cut(i, D, r))
    radii = np.array(radii, np.float32)
    for chunk in (0, 1024):
        wk.g.set_tuning(0, chunk)
        try:
            assert_same(wk.g.range_search_raw(qs, radii, le.W), rr.pack(rows), "%s chunk=%d" % (state, chunk))
        finally:
            wk.g.set_tuning(0, 0)
    print("range after %s: %.2f s" % (state, time.time() - t0))


def test_on_a_file_loaded_opq_index(native):
    """a search never reads the rotation: the :opq fixture answers as its own knn_search, cut"""
    idx = native.load_ivfadc_index(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "persistency_hand_f32_u16_opq.bin"))
    assert idx.rotated
    qs = np.random.default_rng(77).random((5, idx.d), dtype=np.float32)
    full = idx.search_raw(qs, max(1, len(idx)), idx.kc)
    radii = np.array([full[1][q, full[2][q] // 2] if full[2][q] else 1.0 for q in range(5)], np.float32)
    radii[-1] = INF
    got = idx.range_search_raw(qs, radii, idx.kc)
    assert_same(got, cut_of_search(idx, qs, radii, idx.kc), "opq fixture")
    assert got[0][-1] - got[0][-2] == len(idx) > 0
    i, d = native.range_search(idx, qs[0], float(radii[0]), w=idx.kc)
    assert i.dtype == idx.index_type and np.array_equal(i, got[1][:got[0][1]].astype(idx.index_type)) and d.dtype == np.float32


# ---- 3. shapes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9301, 3000, 16, 4, 1), (9302, 2000, 768, 4, 48)], ids=["m1", "m48_d768"])
def test_shape_extremes(native, shape):
    seed, n, d, kc, m = shape
    ref, _ = helpers.build_index(seed, n, d, kc, m, mode="random", ndistinct=50)
    qs = np.random.default_rng(seed + 5).random((4, d), dtype=np.float32)
    g = wp.gpu_handle(native, ref)
    w = 2
    oi, od, oc = ref.knn_search(qs, n, w)
    radii = np.array([od[q, oc[q] // 3] for q in range(4)], np.float32)
    radii[3] = INF
    exp = rr.pack([rr.cut(oi[q, :oc[q]], od[q, :oc[q]], radii[q]) for q in range(4)])
    for chunk in (0, 256):
        g.set_tuning(0, chunk)
        assert_same(g.range_search_raw(qs, radii, w), exp, "m=%d chunk=%d" % (m, chunk))
    g.set_tuning(0, 0)


# ---- 4. entry forms, result life cycle, max_total, refusals ------------------------------------------------------------------------------
def test_device_entry_and_result_life_cycle(native):
    import torch
    from ivfadc_jl_amd import index as ix
    stride = "u8_m3"
    g = handle(native, stride)
    exp = {w: rr.expected(stride, w) for w in (3, rr.KC)}
    dev = {}
    for w in exp:
        qs, radii = rr.queries(stride, w)
        dev[w] = (torch.from_numpy(qs).cuda(), torch.from_numpy(radii).cuda())
    torch.cuda.synchronize()
    for order in ((3, rr.KC), (rr.KC, 3)):
        res = {w: g.range_search_device(dev[w][0].shape[0], dev[w][0].data_ptr(), dev[w][1].data_ptr(), w) for w in exp}   # two alive at once
        g.search_raw(rr.case(stride)[1], 10, 3)                                # a later search on the handle does not touch them
        for w in order:
            assert ix.range_result_sizes(res[w]) == (len(exp[w][0]) - 1, int(exp[w][0][-1]))
            assert_same(ix.range_result_copy(res[w]), exp[w], "device entry w=%d" % w)
            d_lims, d_ids, d_dists = ix.range_result_device(res[w])
            assert d_lims and d_ids and d_dists
            ix.range_result_destroy(res[w])
    # a NaN radius at the device entry (a violated precondition): that query has no results, the others are untouched
    qs, radii = rr.queries(stride, 3)
    bad = radii.copy()
    bad[5] = np.nan
    dbad = torch.from_numpy(bad).cuda()                                        # (kept in a variable until the call has returned)
    torch.cuda.synchronize()
    res = g.range_search_device(qs.shape[0], dev[3][0].data_ptr(), dbad.data_ptr(), 3)
    del dbad
    lims, ids, dd = ix.range_result_copy(res)
    ix.range_result_destroy(res)
    e = exp[3]
    assert lims[6] == lims[5] and np.array_equal(np.diff(lims)[np.arange(len(bad)) != 5], np.diff(e[0])[np.arange(len(bad)) != 5])
    # a result outlives its handle
    ref, _ = rr.case(stride)
    g2 = wp.gpu_handle(native, ref)
    res = g2.range_search_device(qs.shape[0], dev[3][0].data_ptr(), dev[3][1].data_ptr(), 3)
    del g2
    assert_same(ix.range_result_copy(res), e, "after the handle is gone")
    ix.range_result_destroy(res)


def test_max_total_and_refusals(native):
    from ivfadc_jl_amd import _native as nat
    stride = "u8_m8"
    g = handle(native, stride)
    qs, radii = rr.queries(stride, 3)
    exp = rr.expected(stride, 3)
    total = int(exp[0][-1])
    assert total > 1
    assert_same(g.range_search_raw(qs, radii, 3, max_total=total), exp, "max_total == total")
    with pytest.raises(nat.IVFADCError, match=r"\b%d\b" % total) as e:
        g.range_search_raw(qs, radii, 3, max_total=total - 1)
    assert e.value.code == ERR_INVALID
    assert_same(g.range_search_raw(qs, radii, 3), exp, "the call after the refusal")
    nan = radii.copy()
    nan[7] = np.nan
    with pytest.raises(nat.IVFADCError, match="query 7") as e:
        g.range_search_raw(qs, nan, 3)
    assert e.value.code == ERR_INVALID
    with pytest.raises(AssertionError, match="w >= 1"):
        g.range_search_raw(qs, radii, 0)
    lims, ids, dd = g.range_search_raw(qs[:0], radii[:0], 3)                   # an empty batch: an empty result
    assert lims.tolist() == [0] and len(ids) == 0 and len(dd) == 0
    u16 = wp.gpu_handle(native, mk.case("u16_m5").ref)
    with pytest.raises(nat.IVFADCError, match="UInt16") as e:
        u16.range_search_raw(mk.case("u16_m5").qs[:2], np.ones(2, np.float32), 3)
    assert e.value.code == ERR_STATE


# ---- 5. sub-batching ---------------------------------------------------------------------------------------------------------------------
def test_sub_batches_and_sort_groups_do_not_change_the_answer(native):
    """set_workspace_limit at its minimum (1 MiB) with the smallest chunk: the queries split into several sub-batches (the plan's
    arithmetic restated below), and at r = +inf, w = kc the keys split into several sort groups (more than 2^20 keys)"""
    t0 = time.time()
    stride = "u8_m8"
    g = handle(native, stride)
    w = rr.KC
    qs, radii = rr.queries(stride, w)
    reps = 8
    Q, R = np.tile(qs, (reps, 1)), np.tile(radii, reps)
    e = rr.expected(stride, w)
    rows = [(e[1][e[0][q]:e[0][q + 1]], e[2][e[0][q]:e[0][q + 1]]) for q in range(len(radii))] * reps
    items = w * -(-max(mk.LENS) // 64)
    per_query = rr.KC * 20 + w * 12 + items * 8 + 64
    assert (1 << 20) // per_query < Q.shape[0], "the batch must not fit one sub-batch"
    g.set_workspace_limit(1)
    g.set_tuning(0, 1)
    try:
        g.reset_stats()
        assert_same(g.range_search_raw(Q, R, w), rr.pack(rows), "sub-batched")
        assert g.get_stats()["scanned_points"] == Q.shape[0] * rr.N, "every probed point counts once, whatever the passes"
        everything = [rr.full_sorted(stride, int(qi), w) for qi in rr.table(stride, w)[0]] * reps
        assert sum(len(i) for i, _ in everything) > (1 << 20)
        assert_same(g.range_search_raw(Q, np.full(len(R), INF, np.float32), w), rr.pack(everything), "several sort groups")
    finally:
        g.set_tuning(0, 0)
        g.set_workspace_limit(8 << 30)
    print("range sub-batches: %.2f s" % (time.time() - t0))


# ---- 6. sequences ------------------------------------------------------------------------------------------------------------------------
def test_range_search_between_the_scan_forms(native):
    """One leg in the spirit of tests/sequences.py, on the shape where every 8-bit form exists (m = 8, dsub = 16, ksub = 256: the m8_d128 index
    of tests/test_gpu_sequences.py, 14 lists of ~2 100 points): ONE handle walks  R f1 R f2 R ... fn R,  R a range search and f every form
    of test_gpu_sequences.forms_8bit -- query-major with and without the stand-alone top-w, the small-batch launch, the generic path by
    request and by K, list-major at 1 / 2 / 4 on reference tables, the striped tables, the eight-wave forms q4 / q8 (one and several chunks,
    pruning off), the wide pools, the LDS selectors, the narrow-field form and the two list partitions -- then the masked list scan, the
    pre-assigned entry and ivfadc_search_batches, so that every form runs directly behind a range search and directly in front of one.
    Every form is run by test_gpu_sequences.run_form: it names its stats beforehand and asserts them through get_stats(); where
    sequences.expected_form specifies the form, the table's expectation is checked against it first.  Range search shares the key and
    offset buffers of the generic path, the probe arrays, the counter block and the query staging with these forms: every answer on both
    sides is compared exactly."""
    import sequences as sq
    import test_gpu_sequences as tgs
    t0 = time.time()
    kind = tgs.kind_of("m8_d128")
    ix, qs = kind.ix, kind.qs
    nq, w = qs.shape[0], tgs.W
    n = int(ix.offsets[-1])
    shape = dict(m=kind.m, dsub=kind.dsub, ksub=256, kc=kind.kc, n=n, u16=False)
    assert sq.nf_shape(kind.m, kind.dsub) and sq.filt_shape(kind.m, kind.dsub)
    forms = kind.forms()
    names = " | ".join(f["name"] for f in forms)
    for need in ("query-major", "stand-alone top-w", "small-batch", "generic (forced)", "generic by K", "qg=1 reference", "qg=2 reference",
                 "qg=4 reference", "automatic tables", "eight-wave q4", "eight-wave q8", "several chunks", "wide pool q4", "wide pool q8",
                 "LDS selectors", "pruning off", "list partition", "narrow-field"):
        assert need in names, need
    for f in forms:               # the table's stats are the plan's rules (sequences.expected_form), wherever those specify the form
        want = sq.expected_form(shape, dict(table=f["table"], qg=f["qg"], part_n=max(1, f["parts"])), f["K"], f["w"], f["nq"] or nq)
        if want is not None:
            for key, val in want.items():
                assert f["expect"].get(key, val) == val, (f["name"], key, f["expect"], want)
    # the range searches: radius D[50] of each query, every seventh query +inf (all ~6 400 probed points)
    rows, radii = [], []
    for qi in range(nq):
        i, D = helpers.numpy_knn(ix, qs[qi], n, w)
        r = INF if qi % 7 == 0 else D[50]
        radii.append(r)
        rows.append(rr.cut(i, D, r))
    radii = np.array(radii, np.float32)
    exp_r = rr.pack(rows)
    g = kind.make(native)
    io = tgs.DeviceIO(qs)
    count = [0]

    def range_step(behind):
        g.set_list_partition(1, 0)
        g.set_tuning(0, (0, 1024, 1)[count[0] % 3])                            # the default chunk, 1024, the smallest
        count[0] += 1
        before = g.get_stats()
        assert_same(g.range_search_raw(qs, radii, w), exp_r, "range search behind [%s]" % behind)
        after = g.get_stats()
        for key in ("last_qg", "last_chunk", "last_striped", "last_nf", "last_lb", "last_scan_lds"):
            assert after[key] == before[key], "a range search leaves %s as the last search set it" % key

    range_step("a new handle")
    for f in forms:
        tgs.run_form(kind, [g], f, "[%s] behind a range search" % f["name"], io)
        range_step(f["name"])
    # the masked list scan (last_striped == 8): even ids selected for every second query, -1 for the rest
    plain = dict(name="plain", K=10, w=w, nq=None)
    mask = np.arange(int(ix.ids.max()) + 1) % 2 == 0
    fref = wp.ref_with_lists(ix, *sb.filtered_lists(ix.offsets, ix.codes, ix.ids, mask))
    moq = np.where(np.arange(nq) % 2 == 0, 0, -1).astype(np.int32)
    em, ep = fref.knn_search(qs, 10, w), kind.expected(plain)
    exp_m = tuple(np.where((moq == 0).reshape((-1,) + (1,) * (a.ndim - 1)), a, b) for a, b in zip(em, ep))
    ms = g.maskset(masks=[mask])
    g.set_tuning(4, 1024)
    g.set_table_mode(0)
    got = g.search_masked_raw(qs, 10, ms, moq, w=w)
    tgs.ran(g, dict(last_striped=8, last_qg=4, last_chunk=1024), "masked list scan behind a range search")
    helpers.assert_same_results(got, exp_m, what="masked list scan behind a range search")
    range_step("masked list scan")
    # the pre-assigned entry, on the list-major reference-table form
    st = dict(table=1, qg=4)
    want = {k: v for k, v in sq.expected_form(shape, st, 10, w, nq).items() if k != "last_scan_lds"}
    g.set_tuning(4, 1024)
    g.set_table_mode(1)
    lists, cd = g.coarse_search_raw(qs, w)
    range_step("coarse_search")
    g.set_tuning(4, 1024)
    got = g.search_preassigned_raw(qs, 10, lists, cd)
    tgs.ran(g, dict(want, last_chunk=1024), "pre-assigned search behind a range search")
    helpers.assert_same_results(got, ep, what="pre-assigned search behind a range search")
    range_step("pre-assigned search")
    # ivfadc_search_batches: three ragged batches, the odd one on the internal view
    sizes = [20, 25, nq - 45]
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    g.set_tuning(4, 1024)
    parts = g.search_batches_raw([qs[cuts[i]:cuts[i + 1]] for i in range(3)], 10, w)
    tgs.ran(g, {k: v for k, v in sq.expected_form(shape, st, 10, w, sq.index_lane_batch(sizes)).items() if k != "last_scan_lds"}, "search_batches behind a range search")
    helpers.assert_same_results(tuple(np.concatenate([p[i] for p in parts]) for i in range(3)), ep, what="search_batches behind a range search")
    range_step("search_batches")
    assert count[0] == len(forms) + 5
    print("range sequences: %d forms + masked, pre-assigned, batched; %d range searches; %.2f s" % (len(forms), count[0], time.time() - t0))
