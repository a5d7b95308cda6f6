"""GPU parity tests of the large-K search (csrc/selscan.hip.h, sel_scan_kernel; set_tuning(-4, cap_keys)) against the CPU oracle: ids
exact, distance bits identical, and every search asserts that the path ran (last_striped 9, last_qg -4)."""
import numpy as np
import pytest

import helpers
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

LDS_MAX = 160 << 10
_CACHE = {}


def pow2ceil(x):
    return 1 << max(0, int(x) - 1).bit_length()


def auto_cap(d, m, K):
    """selscan_plan.h: the largest multiple of 1024 keys next to the residual, the table, the scratch, the histograms, the control words"""
    fixed = (d + 3) // 4 * 16 + m * 1024 + (pow2ceil(K) * 8 + 15) // 16 * 16 + 8 * 1024 + 64
    return (LDS_MAX - fixed) // 8 // 1024 * 1024


def sel_index(native, oidx, cap_keys=0, labels=None, codes=None):
    g = native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels if labels is None else labels, oidx.offsets,
                                       oidx.codes if codes is None else codes, oidx.ids)
    g.set_tuning(-4, cap_keys)
    return g


def ran_select(g, what="", cap=None):
    st = g.get_stats()
    assert st["last_striped"] == 9 and st["last_qg"] == -4 and st["last_scan_lds"] <= LDS_MAX, (what, st)
    assert cap is None or st["last_chunk"] == cap, (what, st)
    return st


def same_bits(got, exp, what):
    helpers.assert_same_results(got, exp, what=what)
    assert np.array_equal(got[1][exp[1] < np.inf].view(np.uint32), exp[1][exp[1] < np.inf].view(np.uint32)), what


def fixture(name):
    """(oracle index, data, 61 queries, {(K, w): oracle results}) of a named index: built once, left unchanged."""
    if name not in _CACHE:
        rng = np.random.default_rng(len(name) + 4100)
        if name == "rounds":
            oidx, data = helpers.build_index(4101, 30000, 128, 14, 8, 256, mode="random")
        elif name == "ties":
            oidx, data = helpers.build_index(4102, 30000, 128, 14, 8, 256, mode="random", ndistinct=4)
        elif name == "short":
            oidx, data = helpers.build_index(4103, 30000, 128, 300, 8, 256, mode="random")
        else:   # "clustered": build_index's "encode" mode on points around 14 centres that lie far apart against the codewords' reach
            cent, cbs, labels = helpers.make_quantizers(4104, 128, 14, 8, 256)
            cent *= 4.0
            data = cent[rng.integers(0, 14, 30000)] + (rng.random((30000, 128), dtype=np.float32) - 0.5) * 0.5
            lst, codes = ora.OracleIndex(cent, cbs, labels, np.zeros(15, np.int64), np.zeros((0, 8), np.uint8), np.zeros(0, np.uint32)).encode(data)
            order = np.argsort(lst, kind="stable")
            off = np.zeros(15, np.int64)
            np.cumsum(np.bincount(lst, minlength=14), out=off[1:])
            oidx = ora.OracleIndex(cent, cbs, labels, off, np.ascontiguousarray(codes[order]), order.astype(np.uint32))
        qs = data[:61] + 0.01 if name == "clustered" else rng.random((61, oidx.d), dtype=np.float32)
        _CACHE[name] = (oidx, data, qs, {})
    return _CACHE[name]


def expected(name, K, w):
    oidx, _, qs, res = fixture(name)
    if (K, w) not in res:
        res[(K, w)] = oidx.knn_search(qs, K, w)
    return res[(K, w)]


def check(native, name, K, w, cap_keys, what):
    oidx, _, qs, _ = fixture(name)
    cap = max(cap_keys, 2 * pow2ceil(K), 2048) if cap_keys else auto_cap(oidx.d, oidx.m, K)
    g = sel_index(native, oidx, cap if cap_keys else 0)
    exp = expected(name, K, w)
    same_bits(g.search_raw(qs, K, w), exp, what)
    ran_select(g, what, cap)
    same_bits(g.search_raw(qs[:9], K, w), tuple(a[:9] for a in exp), what + ", second call")
    ran_select(g, what + ", second call", cap)


@pytest.mark.parametrize("w,cap_keys", [(3, 0), (14, 0), (14, 4096), (5, 8192)])
@pytest.mark.parametrize("K", [1, 64, 65, 100, 1000, 2048])
def test_round_structure(native, K, w, cap_keys):
    """14 lists of ~2100 points: w = 14 probes more points than any buffer holds (several rounds), w = 3 fewer than the automatic one."""
    oidx, _, _, _ = fixture("rounds")
    lens = np.diff(oidx.offsets)
    assert lens.sum() == 30000 and 30000 > LDS_MAX // 8, "w = 14: every query probes more points than LDS holds keys"
    assert np.sort(lens)[-3:].sum() < auto_cap(128, 8, K), "w = 3: a query's probes fit the automatic buffer"
    check(native, "rounds", K, w, cap_keys, "select K=%d w=%d cap=%d" % (K, w, cap_keys))


@pytest.mark.parametrize("K", [65, 1000, 2047])
def test_ties_at_the_kth_key(native, K):
    """Four distinct codes: the K-th key ties in its distance word, the visit order decides, tie groups span rounds of a 4096-key buffer."""
    check(native, "ties", K, 14, 4096, "select ties K=%d" % K)


@pytest.mark.parametrize("w", [1, 5])
def test_short_pools(native, w):
    """300 lists of ~100 points, K = 1000: fewer than K points are probed, counts fall below K; one probed list is empty."""
    oidx, _, qs, _ = fixture("short")
    exp = expected("short", 1000, w)
    assert exp[2].max() < 1000
    lens = np.diff(oidx.offsets).copy()
    # empty the list that query 0 probes first
    first = int(np.argmin(((oidx.centroids - qs[0]) ** 2).sum(1)))
    keep = np.ones(oidx.codes.shape[0], bool)
    keep[oidx.offsets[first]:oidx.offsets[first + 1]] = False
    lens[first] = 0
    off = np.zeros(oidx.kc + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    o2 = ora.OracleIndex(oidx.centroids, oidx.codebooks, oidx.labels, off, np.ascontiguousarray(oidx.codes[keep]),
                         np.ascontiguousarray(oidx.ids[keep]))
    for o, e in ((oidx, exp), (o2, o2.knn_search(qs, 1000, w))):
        g = sel_index(native, o)
        same_bits(g.search_raw(qs, 1000, w), e, "select short pools w=%d" % w)
        ran_select(g)
    assert o2.knn_search(qs[:1], 1000, 1)[2][0] == 0


def test_exact_hits(native):
    """Queries that are centroid + codewords: table entries of 0, keys whose distance word equals dc."""
    oidx, _, qs, _ = fixture("rounds")
    rng = np.random.default_rng(4110)
    qs = qs.copy()
    for i in range(16):
        code = rng.integers(0, 256, oidx.m)
        qs[i] = oidx.centroids[i % oidx.kc] + np.concatenate([oidx.codebooks[ii, code[ii]] for ii in range(oidx.m)])
    g = sel_index(native, oidx)
    same_bits(g.search_raw(qs, 100, 3), oidx.knn_search(qs, 100, 3), "select exact hits")
    ran_select(g)


@pytest.mark.parametrize("d,m,ksub,n,perm", [(96, 16, 256, 30000, False), (10, 2, 256, 30000, True), (6, 1, 7, 30000, False),
                                             (768, 48, 256, 8000, False)])
def test_other_shapes(native, d, m, ksub, n, perm):
    """m = 16 (16-byte loads, pair-packed dsub = 6 build); the code stride at m = 2, m = 1 with seven codewords, m = 48 (48 KB of tables)."""
    oidx, _ = helpers.build_index(4120 + m, n, d, 14, m, ksub, label_perm=perm, mode="random")
    qs = np.random.default_rng(4130 + m).random((33, d), dtype=np.float32)
    for K in (100, 1000):
        g = sel_index(native, oidx)
        same_bits(g.search_raw(qs, K, 4), oidx.knn_search(qs, K, 4), "select d=%d m=%d K=%d" % (d, m, K))
        ran_select(g, cap=auto_cap(d, m, K))


def test_pruning_is_exact(native):
    """Clustered data, w = 14, K = 100: the same bytes with pruning on and off, and pruning has something to skip."""
    oidx, _, qs, _ = fixture("clustered")
    exp = expected("clustered", 100, 14)
    last_dc = np.array([oidx.coarse_search(q, 14)[1][13] for q in qs])
    assert (exp[1][:, 99] < last_dc).any(), "for some query the K-th distance lies below the last probe's dc"
    out = {}
    for on in (1, 0):
        g = sel_index(native, oidx)
        g.set_pruning(on)
        out[on] = g.search_raw(qs, 100, 14)
        st = ran_select(g)
        assert (st["pruned_points"] > 0) == bool(on), st
        same_bits(out[on], exp, "select pruning=%d" % on)
    assert all(np.array_equal(a, b) for a, b in zip(out[1], out[0]))


def test_fallbacks_plan_as_the_default(native):
    """Under qg = -4 a UInt16 handle, a masked search and supplied probes return the oracle's bytes and report what qg = 0 reports."""
    oidx, _, qs, _ = fixture("rounds")
    exp = expected("rounds", 100, 3)
    what = ("last_qg", "last_striped", "last_chunk", "last_scan_lds")
    runs = {}
    for qg in (0, -4):
        g16 = sel_index(native, oidx, labels=oidx.labels.astype(np.uint16), codes=oidx.codes.astype(np.uint16))
        g = sel_index(native, oidx)
        for h in (g16, g):
            h.set_tuning(qg, 0)
        ms = g.maskset(masks=[np.ones(30000, bool)])
        lists, cd = g.coarse_search_raw(qs, 3)
        runs[qg] = []
        for h, got in ((g16, lambda: g16.search_raw(qs, 100, 3)), (g, lambda: g.search_masked_raw(qs, 100, ms, None, 3)),
                       (g, lambda: g.search_preassigned_raw(qs, 100, lists, cd))):
            same_bits(got(), exp, "fallback under qg=%d" % qg)
            st = h.get_stats()
            runs[qg].append([st[k] for k in what])
            assert st["last_qg"] != -4, st
    assert runs[0] == runs[-4]


def test_neighbours(native):
    """A view; the refined search at kc = 1000 against the default plan's bytes; one handle alternating plans; three sub-batches."""
    oidx, data, qs, _ = fixture("rounds")
    exp = expected("rounds", 1000, 3)
    g = sel_index(native, oidx)
    v = g.clone_view()
    same_bits(v.search_raw(qs, 1000, 3), exp, "view")
    ran_select(v)
    store = g.vectors(data)
    refined = g.search_refined_raw(store, qs, 10, 1000, 3)
    ran_select(g)
    g.set_tuning(0, 0)
    assert all(np.array_equal(a, b) for a, b in zip(refined, g.search_refined_raw(store, qs, 10, 1000, 3)))
    assert g.get_stats()["last_qg"] != -4
    for qg in (0, -4, -2, -4):
        g.set_tuning(qg, 0)
        same_bits(g.search_raw(qs, 1000, 3), exp, "alternating, qg=%d" % qg)
        assert (g.get_stats()["last_qg"] == -4) == (qg == -4) and (g.get_stats()["last_qg"] == -2) == (qg == -2)
    # 1 MB of workspace at kc = 300, w = 5 (selscan_plan.h: a query's share is its coarse row, its probe arrays and 64 bytes)
    oidx, _, qs, _ = fixture("short")
    many = np.random.default_rng(4140).random((2000, 128), dtype=np.float32)
    g = sel_index(native, oidx)
    one = g.search_raw(many, 1000, 5)
    g.set_workspace_limit(1 << 20)
    three = g.search_raw(many, 1000, 5)
    nb = (1 << 20) // (300 * 4 + 5 * 12 + 64)
    assert 2 * nb < 2000 <= 3 * nb and ran_select(g)["last_scan_grid"] == 2000 - 2 * nb
    assert all(np.array_equal(a, b) for a, b in zip(one, three))
    same_bits((one[0][:61], one[1][:61], one[2][:61]), oidx.knn_search(many[:61], 1000, 5), "sub-batches")
