"""Searches with caller-supplied probes (ivfadc_coarse_search*, ivfadc_search*_preassigned) on the GPU.  Every comparison is exact:
counts equal, ids equal, distance bits identical.  The references are the CPU oracle's coarse_search, the handle's own plain search
(a preassigned search fed with the coarse result must return its bytes on every scan form) and pre_knn, the numpy restatement of
index.jl:220-257 for ANY probes (tests/test_preassigned_abi.py, which also shows on the CPU that the inputs used here tell "skip a
list above the bound" from "stop at the first one")."""
import numpy as np
import pytest

import helpers
import sequences as sq
import u16_ref
from test_preassigned_abi import pre_knn_batch, teeth_input, true_coarse

pytestmark = pytest.mark.gpu
f32 = np.float32
same = helpers.assert_same_results


def gpu_index(native, oidx):
    return native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)


def u16_index(native, ix):
    return native.IVFADCIndex.from_arrays(ix.centroids, ix.codebooks, ix.labels.astype(np.uint16), ix.offsets, ix.codes.astype(np.uint16), ix.ids)


def ran(g, expect, what):
    st = g.get_stats()
    for key, val in expect.items():
        assert st[key] == val, "%s did not run as the form it names: %s = %s, expected %s (%s)" % (what, key, st[key], val, st)


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def oracle_coarse(oidx, qs, w):
    def make():
        lists = np.zeros((qs.shape[0], w), np.int32)
        dists = np.zeros((qs.shape[0], w), f32)
        for r in range(qs.shape[0]):
            lists[r], dists[r] = oidx.coarse_search(qs[r], w)
        return lists, dists
    return cached(("coarse", id(oidx), id(qs), w), make)


def same_coarse(got, exp, what):
    assert got[0].dtype == np.int32 and got[1].dtype == f32 and got[0].shape == exp[0].shape, what
    bad = np.nonzero((got[0] != exp[0]).any(axis=1) | (got[1].view(np.uint32) != exp[1].view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, "%s: query %d: lists %s vs %s, dists %s vs %s" % (what, bad[0], got[0][bad[0]], exp[0][bad[0]], got[1][bad[0]], exp[1][bad[0]])


# ---- 1. coarse search -------------------------------------------------------------------------------------------------------------------
def coarse_fixture():
    """kc = 384 (the matrix-core filter and the two-level search both exist from 128 cells on), d = 32, two pairs of identical centroids,
    queries that sit on centroids (distance +0, exact ties between the twins) and uniform ones."""
    def make():
        oidx, _ = helpers.build_index(31, 3000, 32, 384, 8, mode="random")
        oidx.centroids[200] = oidx.centroids[5]
        oidx.centroids[18] = oidx.centroids[17]
        rng = np.random.default_rng(32)
        qs = rng.random((1500, 32), dtype=f32)
        qs[:6] = oidx.centroids[[5, 200, 17, 18, 0, 383]]
        return oidx, qs
    return cached("coarse_fixture", make)


@pytest.mark.parametrize("mode,expect", [(0, {}), (1, {"coarse_mfma": 0, "last_twolevel": 0}), (2, {"coarse_mfma": 1}), (6, {"last_twolevel": 1})])
def test_coarse_search_equals_the_oracle_in_every_coarse_mode(native, mode, expect):
    oidx, qs = coarse_fixture()
    g = gpu_index(native, oidx)
    g.set_coarse_mode(mode)
    for nq, w in ((70, 8), (70, 1), (9, 48), (300, 8)):
        got = g.coarse_search_raw(qs[:nq], w)
        ran(g, expect, "coarse mode %d, nq = %d, w = %d" % (mode, nq, w))
        same_coarse(got, tuple(a[:nq] for a in oracle_coarse(oidx, qs, w)), "coarse mode %d, nq = %d, w = %d" % (mode, nq, w))
    # ties go to the lower cell: the twins, in index order, at the same distance
    l, d = g.coarse_search_raw(qs[:4], 2)
    assert l.tolist() == [[5, 200], [5, 200], [17, 18], [17, 18]] and (d == 0).all(), (l, d)
    # beyond the register selectors and the filters (w > 64), and every cell
    for w in (100, 384):
        same_coarse(g.coarse_search_raw(qs[:20], w), tuple(a[:20] for a in oracle_coarse(oidx, qs, w)), "coarse mode %d, w = %d" % (mode, w))
    # the module-level function of the reference's name: one point, and a list of points
    l1, d1 = native.coarse_search(g, qs[7], 3)
    assert l1.shape == (3,) and np.array_equal(l1, oracle_coarse(oidx, qs, 3)[0][7]) and np.array_equal(d1, oracle_coarse(oidx, qs, 3)[1][7])
    l2, _ = native.coarse_search(g, [qs[7], qs[8]], 3)
    assert l2.shape == (2, 3) and np.array_equal(l2[0], l1)


def test_coarse_search_small_quantizer_and_sub_batches(native):
    oidx, _ = cached("kc100", lambda: helpers.build_index(33, 2000, 16, 100, 4, mode="random"))
    qs = cached("kc100q", lambda: np.random.default_rng(34).random((40, 16), dtype=f32))
    g = gpu_index(native, oidx)
    for w in (1, 100):
        same_coarse(g.coarse_search_raw(qs, w), oracle_coarse(oidx, qs, w), "kc = 100, w = %d" % w)
    from ivfadc_jl_amd import _native as nat
    with pytest.raises(nat.IVFADCError, match="exceeds the 100 cells") as e:
        g.coarse_search_raw(qs, 101)
    assert e.value.code == 2
    with pytest.raises(AssertionError, match="w >= 1"):
        g.coarse_search_raw(qs, 0)
    assert g.coarse_search_raw(qs[:0], 3)[0].shape == (0, 3)
    # a small workspace limit: 1500 queries x (4 kc + 4 w + 64) bytes = 2.4 MB against 1 MB -- three sub-batches
    oidx, qs = coarse_fixture()
    g = gpu_index(native, oidx)
    g.set_workspace_limit(sq.WS_SMALL)
    same_coarse(g.coarse_search_raw(qs, 8), oracle_coarse(oidx, qs, 8), "sub-batched coarse search")


# ---- 2. round trip: search_preassigned(coarse_search) == search, on every scan form -----------------------------------------------------
def roundtrip_kind(name):
    def make():
        if name == "u16":
            ix = u16_ref.make_index(4242, 40000, 32, 4, 4, 1024, perm_labels=True, ndistinct=5000)
            return ix, np.random.default_rng(9).random((96, 32), dtype=f32)
        if name == "m16_d96":
            ix, _ = helpers.build_index(9102, 20000, 96, 24, 16, 256, mode="random")
            return ix, np.random.default_rng(10).random((70, 96), dtype=f32)
        d = {"m8_d32": 32, "m8_d128": 128}[name]
        ix, _ = helpers.build_index(2500 + d, 30000, d, 14, 8, 256, mode="random")
        return ix, np.random.default_rng(177 + d).random((200, d), dtype=f32)
    return cached(("kind", name), make)


def _f(name, kind, qg=0, chunk=0, table=0, K=10, w=3, nq=61, prune=1, ws=sq.WS_DEFAULT, **expect):
    return pytest.param(dict(kind=kind, qg=qg, chunk=chunk, table=table, K=K, w=w, nq=nq, prune=prune, ws=ws, expect=expect), id=name)


ROUNDTRIP = [
    _f("query-major", "m8_d32", -1, last_qg=0, last_lb=0),
    _f("query-major, pruning off", "m8_d32", -1, prune=0, last_qg=0, pruned_points=0),
    _f("query-major, w = 8, K = 100", "m8_d32", -1, K=100, w=8, last_qg=0),
    _f("query-major, w = 14 > 8 probes per LDS row", "m8_d32", -3, w=14, last_qg=0),
    _f("default plan", "m8_d32", 0, nq=200, w=8),
    _f("latency-path batch, nq = 1", "m8_d32", 0, nq=1, w=8),
    _f("latency-path batch, nq = 8", "m8_d32", 0, nq=8, w=3),
    _f("list-major qg = 1", "m8_d32", 1, 1024, table=1, last_qg=1, last_striped=0, last_nf=0),
    _f("list-major qg = 2", "m8_d32", 2, 1024, table=1, last_qg=2, last_striped=0, last_nf=0),
    _f("list-major qg = 4", "m8_d32", 4, 1024, table=1, last_qg=4, last_striped=0, last_nf=0),
    _f("list-major qg = 4, three sub-batches", "m8_d32", 4, 1024, table=1, K=64, w=8, nq=200, ws=sq.WS_SMALL, last_qg=4),
    _f("narrow-field qg = 8", "m8_d128", 8, last_qg=8, last_nf=1),
    _f("eight-wave q4 (table mode 6)", "m8_d32", 4, table=6, last_qg=4, last_striped=2),
    _f("eight-wave q8 (table mode 7)", "m8_d32", 4, table=7, last_qg=8, last_striped=3),
    _f("wide pool K = 100 (table mode 8)", "m8_d32", 4, table=8, K=100, last_qg=4, last_striped=4),
    _f("lower-bound rounds (table mode 2)", "m16_d96", -1, table=2, w=6, nq=70, last_qg=0, last_lb=1),
    _f("lower-bound rounds, pruning off", "m16_d96", -3, table=2, w=6, nq=70, prune=0, last_qg=0, last_lb=1),
    _f("generic (forced)", "m8_d32", -2, last_qg=-2),
    _f("generic by K", "m8_d32", 0, K=2500, nq=8, last_qg=-2),
    _f("u16 K = 10", "u16", 0, nq=96, last_striped=0),
    _f("u16 K = 100, mode 0 (generic)", "u16", 4, K=100, nq=96, last_qg=-2),
    _f("u16 K = 100, mode 10", "u16", 4, table=10, K=100, nq=96, last_qg=4),
]


@pytest.mark.parametrize("f", ROUNDTRIP)
def test_round_trip_returns_the_bytes_of_a_plain_search(native, f):
    ix, qs = roundtrip_kind(f["kind"])
    g = u16_index(native, ix) if f["kind"] == "u16" else gpu_index(native, ix)
    g.set_tuning(f["qg"], f["chunk"])
    g.set_table_mode(f["table"])
    g.set_pruning(f["prune"])
    g.set_workspace_limit(f["ws"])
    q, K, w = qs[:f["nq"]], f["K"], f["w"]
    plain = g.search_raw(q, K, w)
    lists, dists = g.coarse_search_raw(q, w)
    g.reset_stats()
    got = g.search_preassigned_raw(q, K, lists, dists)
    ran(g, f["expect"], "preassigned")
    st = g.get_stats()
    assert st["last_qg"] != -3 and st["queries"] == q.shape[0], st       # never the latency path: it has no seam
    same(got, plain, what="preassigned(coarse_search) vs search")
    # ... and through a view of the handle
    v = g.clone_view()
    same(v.search_preassigned_raw(q, K, lists, dists), plain, what="view: preassigned(coarse_search) vs search")
    ran(v, {k: x for k, x in f["expect"].items() if k != "pruned_points"}, "preassigned on a view")


def test_module_level_functions(native):
    ix, qs = roundtrip_kind("m8_d32")
    g = gpu_index(native, ix)
    cl, cd = native.coarse_search(g, qs[:5], 4)
    ids, dists = native.knn_search_preassigned(g, qs[:5], 7, cl, cd)
    eids, edists = native.knn_search(g, qs[:5], 7, w=4)
    for r in range(5):
        assert ids[r].dtype == eids[r].dtype and np.array_equal(ids[r], eids[r]) and np.array_equal(dists[r].view(np.uint32), edists[r].view(np.uint32))
    i1, d1 = native.knn_search_preassigned(g, qs[2], 7, cl[2], cd[2])
    assert np.array_equal(i1, eids[2]) and np.array_equal(d1, edists[2])
    with pytest.raises(AssertionError, match="k >= 1"):
        native.knn_search_preassigned(g, qs[:5], 0, cl, cd)
    with pytest.raises(AssertionError, match="k >= 1"):
        g.search_preassigned_raw(qs[:5], 0, cl, cd)          # the library's own text (index.jl:210)


# ---- 3. arbitrary probes against the restatement ----------------------------------------------------------------------------------------
def expected_pre(shape, K, tag, lists, dists):
    oidx, qs, _, _ = teeth_input(shape)
    return cached(("pre", shape, K, tag), lambda: pre_knn_batch(oidx, qs, K, lists, dists))


def arbitrary_probes(shape):
    """tag -> (lists, dists) over the teeth queries: the interleaved near / far probes with their true distances; shuffled ranks with
    made-up distances in [0, 4); the true probes in descending order; every cell in a random permutation."""
    def make():
        oidx, qs, tl, td = teeth_input(shape)
        rng = np.random.default_rng(77)
        out = {"interleaved": (tl, td)}
        sl = np.stack([rng.permutation(oidx.kc)[:8] for _ in range(qs.shape[0])]).astype(np.int32)
        out["made-up"] = (sl, (rng.random(sl.shape, dtype=f32) * f32(4)).astype(f32))
        cl, cd = true_coarse(oidx, qs, 8)
        out["descending"] = (np.ascontiguousarray(cl[:, ::-1]), np.ascontiguousarray(cd[:, ::-1]))
        al, ad = true_coarse(oidx, qs, oidx.kc)
        perms = np.stack([rng.permutation(oidx.kc) for _ in range(qs.shape[0])])
        out["w = kc"] = (np.take_along_axis(al, perms, 1), np.take_along_axis(ad, perms, 1))
        return out
    return cached(("probes", shape), make)


@pytest.mark.parametrize("prune", [1, 0])
@pytest.mark.parametrize("form", ["query-major", "query-major stand-alone", "lower-bound", "list-major", "generic"])
def test_arbitrary_probes_equal_the_restatement(native, form, prune):
    shape = "m16" if form == "lower-bound" else "m8"
    oidx, qs, _, _ = teeth_input(shape)
    g = gpu_index(native, oidx)
    g.set_tuning({"query-major": -1, "query-major stand-alone": -3, "lower-bound": -1, "list-major": 2, "generic": -2}[form], 0)
    g.set_table_mode(2 if form == "lower-bound" else 0)
    g.set_pruning(prune)
    probes = arbitrary_probes(shape)
    for tag, Ks in (("interleaved", (1, 3, 10, 65)), ("made-up", (3, 65)), ("descending", (1, 10)), ("w = kc", (10,))):
        lists, dists = probes[tag]
        for K in Ks:
            g.reset_stats()
            got = g.search_preassigned_raw(qs, K, lists, dists)
            what = "%s, pruning %d, %s probes, K = %d" % (form, prune, tag, K)
            st = g.get_stats()
            if form == "lower-bound":
                assert st["last_lb"] == (1 if K <= 64 and lists.shape[1] <= 32 else 0) and st["last_qg"] == 0, (what, st)
            elif form != "list-major":
                assert st["last_qg"] == (-2 if form == "generic" else 0), (what, st)
            else:
                assert st["last_qg"] == 2, (what, st)
            if form.startswith("query-major") or form == "lower-bound":
                if not prune:
                    assert st["pruned_points"] == 0, (what, st)
                elif tag == "interleaved" and K <= 10:
                    assert st["pruned_points"] > 0, (what, st)        # the rule fired: far lists were skipped, near ones behind them were not
            same(got, expected_pre(shape, K, tag, lists, dists), what=what)


def test_empty_lists_short_lists_and_no_queries(native):
    """Probes that include empty lists, probes whose lists are all empty (count 0), fewer than K points in the probed lists, nq = 0."""
    def make():
        base, qs, _, _ = teeth_input("m8")
        from oracle import oracle as ora
        off = base.offsets.copy()
        off[1:-1:2] = off[2::2]            # every odd list gives its points to the even list in front of it and is empty
        return ora.OracleIndex(base.centroids, base.codebooks, base.labels, off, base.codes, base.ids), qs
    oidx, qs = cached("holes", make)
    assert (np.diff(oidx.offsets)[1::2] == 0).all() and (np.diff(oidx.offsets)[0::2] > 0).all()
    rng = np.random.default_rng(78)
    mixed = np.stack([rng.permutation(32)[:8] for _ in range(40)]).astype(np.int32)
    empty = np.stack([2 * rng.permutation(16)[:8] + 1 for _ in range(40)]).astype(np.int32)
    one = np.stack([np.array([2 * int(rng.integers(0, 16)) + 1, 2 * int(rng.integers(0, 16))]) for _ in range(40)]).astype(np.int32)
    g = gpu_index(native, oidx)
    for qg in (-1, 2, -2):
        g.set_tuning(qg, 0)
        for tag, lists, K in (("mixed", mixed, 10), ("all empty", empty, 10), ("short", one, 1000)):
            dists = (rng.random(lists.shape, dtype=f32) * f32(2)).astype(f32)
            got = g.search_preassigned_raw(qs, K, lists, dists)
            exp = pre_knn_batch(oidx, qs, K, lists, dists)
            if tag == "all empty":
                assert (got[2] == 0).all()
            if tag == "short":
                assert (got[2] < K).all() and (got[2] > 0).all()
            same(got, exp, what="tuning %d, %s" % (qg, tag))
        i, d, c = g.search_preassigned_raw(qs[:0], 5, mixed[:0], mixed[:0].astype(f32))
        assert i.shape == (0, 5) and c.shape == (0,)


# ---- 4. the supplied rank breaks ties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qg", [-1, 1, -2])
def test_supplied_rank_breaks_ties(native, qg):
    """Two identical centroid rows whose lists hold identical codes: with equal supplied distances every point of one twin ties with
    its counterpart in the other, and the twin that was supplied FIRST comes first (visit order = supplied rank)."""
    from oracle import oracle as ora
    cent, cbs, labels = helpers.make_quantizers(41, 32, 4, 8, 256)
    cent[2] = cent[1]
    rng = np.random.default_rng(42)
    codes = rng.integers(0, 256, (6, 8)).astype(np.uint8)
    offsets = np.array([0, 3, 9, 15, 18], np.int64)
    allcodes = np.concatenate([rng.integers(0, 256, (3, 8)).astype(np.uint8), codes, codes, rng.integers(0, 256, (3, 8)).astype(np.uint8)])
    ids = np.arange(18, dtype=np.uint32) + 100
    oidx = ora.OracleIndex(cent, cbs, labels, offsets, allcodes, ids)
    qs = rng.random((5, 32), dtype=f32)
    g = gpu_index(native, oidx)
    g.set_tuning(qg, 0)
    dd = np.full((5, 2), 0.75, f32)
    ab = g.search_preassigned_raw(qs, 12, np.tile(np.array([1, 2], np.int32), (5, 1)), dd)
    ba = g.search_preassigned_raw(qs, 12, np.tile(np.array([2, 1], np.int32), (5, 1)), dd)
    same(ab, pre_knn_batch(oidx, qs, 12, np.tile([1, 2], (5, 1)), dd), what="twins, a first")
    same(ba, pre_knn_batch(oidx, qs, 12, np.tile([2, 1], (5, 1)), dd), what="twins, b first")
    assert np.array_equal(ab[1].view(np.uint32), ba[1].view(np.uint32)) and (ab[2] == 12).all()
    for r in range(5):
        assert (ab[0][r, 0::2] < 109).all() and (ab[0][r, 1::2] >= 109).all(), ab[0][r]       # list 1's ids (103..108) lead each tied pair
        assert np.array_equal(ab[0][r, 0::2] + 6, ab[0][r, 1::2])
        assert np.array_equal(ba[0][r, 0::2], ab[0][r, 1::2]) and np.array_equal(ba[0][r, 1::2], ab[0][r, 0::2])


# ---- 5. host validation -----------------------------------------------------------------------------------------------------------------
def test_host_entry_validates_the_probes_before_any_launch(native):
    from ivfadc_jl_amd import _native as nat
    oidx, qs, lists, dists = teeth_input("m8")
    g = gpu_index(native, oidx)
    good = g.search_preassigned_raw(qs, 10, lists, dists)
    before = g.get_stats()["queries"]

    def spoiled(what, value):
        l, d = lists.copy(), dists.copy()
        if what == "list":
            l[7, 3] = value
        else:
            d[7, 3] = value
        return l, d
    cases = [("list", 32, "query 7, rank 3: list 32 out of range"), ("list", -1, "query 7, rank 3: negative list -1"),
             ("list", int(lists[7, 0]), "query 7, rank 3: list %d repeated" % int(lists[7, 0])), ("dist", np.nan, "query 7, rank 3: coarse distance is NaN"),
             ("dist", np.inf, "query 7, rank 3: coarse distance is infinite"), ("dist", -1.0, "query 7, rank 3: negative coarse distance")]
    for what, value, msg in cases:
        with pytest.raises(nat.IVFADCError, match=msg) as e:
            g.search_preassigned_raw(qs, 10, *spoiled(what, value))
        assert e.value.code == 2, (msg, e.value.code)
    wide = np.tile(np.arange(33, dtype=np.int32), (40, 1))
    with pytest.raises(nat.IVFADCError, match="w = 33 exceeds the 32 cells") as e:
        g.search_preassigned_raw(qs, 10, wide, np.zeros(wide.shape, f32))
    assert e.value.code == 2
    assert g.get_stats()["queries"] == before, "a refused call launched a search"
    same(g.search_preassigned_raw(qs, 10, lists, dists), good, what="after the refusals")
    same(g.search_raw(qs, 10, 8), oidx.knn_search(qs, 10, 8), what="plain search after the refusals")
    # a handle with a list partition set
    g.set_list_partition(2, 0)
    with pytest.raises(nat.IVFADCError, match="list partition") as e:
        g.search_preassigned_raw(qs, 10, lists, dists)
    assert e.value.code == 4
    g.set_list_partition(1, 0)
    same(g.search_preassigned_raw(qs, 10, lists, dists), good, what="partition off again")


# ---- 6. device pointers, sequences ------------------------------------------------------------------------------------------------------
def test_device_entries_on_torch_buffers(native):
    import torch
    oidx, qs, lists, dists = teeth_input("m8")
    g = gpu_index(native, oidx)
    dev = torch.device("cuda:0")
    nq, K, w = qs.shape[0], 10, 8
    dq = torch.from_numpy(qs).to(dev)
    dl, dd = torch.from_numpy(lists).to(dev), torch.from_numpy(dists).to(dev)
    oi, od, oc = torch.zeros(nq * K, dtype=torch.int32, device=dev), torch.zeros(nq * K, dtype=torch.float32, device=dev), torch.zeros(nq, dtype=torch.int32, device=dev)
    cl, cd = torch.zeros(nq * w, dtype=torch.int32, device=dev), torch.zeros(nq * w, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    g.search_device_preassigned(nq, dq.data_ptr(), K, w, dl.data_ptr(), dd.data_ptr(), oi.data_ptr(), od.data_ptr(), oc.data_ptr())
    g.sync()
    got = (oi.cpu().numpy().view(np.uint32).reshape(nq, K), od.cpu().numpy().reshape(nq, K), oc.cpu().numpy())
    same(got, g.search_preassigned_raw(qs, K, lists, dists), what="device entry vs host entry")
    same(got, expected_pre("m8", K, "interleaved", lists, dists), what="device entry vs pre_knn")
    # coarse search into device rows, fed straight back: the plain search's bytes
    g.coarse_search_device(nq, dq.data_ptr(), w, cl.data_ptr(), cd.data_ptr())
    g.search_device_preassigned(nq, dq.data_ptr(), K, w, cl.data_ptr(), cd.data_ptr(), oi.data_ptr(), od.data_ptr(), oc.data_ptr())
    g.sync()
    same_coarse((cl.cpu().numpy().reshape(nq, w), cd.cpu().numpy().reshape(nq, w)), oracle_coarse(oidx, qs, w), "coarse_search_device")
    got = (oi.cpu().numpy().view(np.uint32).reshape(nq, K), od.cpu().numpy().reshape(nq, K), oc.cpu().numpy())
    same(got, oidx.knn_search(qs, K, w), what="coarse_search_device -> search_device_preassigned vs the oracle")


def test_plain_and_preassigned_searches_interleave_on_one_handle(native):
    """plain, preassigned, plain -- with a push and a delete in between -- each what it is on a fresh handle."""
    from oracle import oracle as ora
    base, qs, lists, dists = teeth_input("m8")
    g = gpu_index(native, base)
    for qg in (-1, 4):
        g.set_tuning(qg, 0)
        oidx = ora.OracleIndex(base.centroids, base.codebooks, base.labels, *g._lists())
        same(g.search_raw(qs, 10, 8), oidx.knn_search(qs, 10, 8), what="plain, first")
        same(g.search_preassigned_raw(qs, 10, lists, dists), pre_knn_batch(oidx, qs, 10, lists, dists), what="preassigned")
        first = 50000 + 10 * (qg + 1)
        g._append(qs[:7], np.arange(first, first + 7, dtype=np.uint32))
        oidx = ora.OracleIndex(base.centroids, base.codebooks, base.labels, *g._lists())
        same(g.search_preassigned_raw(qs, 10, lists, dists), pre_knn_batch(oidx, qs, 10, lists, dists), what="preassigned after a push")
        same(g.search_raw(qs, 10, 8), oidx.knn_search(qs, 10, 8), what="plain after a push")
        g._delete_ids(np.array([3, first], np.uint32))
        oidx = ora.OracleIndex(base.centroids, base.codebooks, base.labels, *g._lists())
        same(g.search_preassigned_raw(qs, 10, lists, dists), pre_knn_batch(oidx, qs, 10, lists, dists), what="preassigned after a delete")
        same(g.search_raw(qs, 10, 8), oidx.knn_search(qs, 10, 8), what="plain after a delete")
