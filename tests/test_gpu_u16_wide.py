"""GPU tests of the UInt16 scan kernel's LDS-selector form (csrc/u16scan.hip.h, u16_wide_scan_kernel: 64 < K <= 1984), reached through table
mode 10 only.  What is new in the kernel is the selector state that lives in LDS beside the table area across passes, tiles and sub-spaces,
the in-place merge of the four waves' buffers, and the plan's LDS rule (m dsp + qg cap <= 4091).  Every comparison is exact: counts and ids
equal, distance bits identical -- against the same handle's generic path and against tests/u16_ref.py.  Every search asserts through
get_stats() which path ran."""
import ctypes as C

import numpy as np
import pytest

import helpers
import u16_ref
from u16_ref import assert_exact
from test_gpu_u16_edges import _tie_indexes, assert_fast, assert_generic, generic_of, same_bytes, u16_index

pytestmark = pytest.mark.gpu
f32 = np.float32
LDS_MAX = 160 << 10


def cap_of(K):
    """make_plan's selector capacity: max(128, pow2ceil(K + 64))."""
    p = 1
    while p < K + 64:
        p <<= 1
    return max(128, p)


def small_lds(m, dsub):
    """u16_lds_bytes: residuals of 8 pairs (dsub rounded up to 4), 32 KB of tables, per-wave counts, two words."""
    return 8 * m * ((dsub + 3) & ~3) * 4 + 32768 + 4 * 8 * 4 + 16


def wide_lds(m, dsub, qg, cap):
    """u16_wide_lds_bytes: the same plus selbuf[4 waves][qg][cap] u64."""
    return small_lds(m, dsub) + 4 * qg * cap * 8


def planned_qg(m, dsub, qg, K):
    """The plan's rule: qg halved until the need fits a CU; 0 = does not fit at qg = 1 (generic path)."""
    while qg > 1 and wide_lds(m, dsub, qg, cap_of(K)) > LDS_MAX:
        qg >>= 1
    return qg if wide_lds(m, dsub, qg, cap_of(K)) <= LDS_MAX else 0


def wide(g, q, K, w, qg=0, chunk=0):
    """A mode-10 search that must have run the kernel: the results and the stats."""
    g.set_tuning(qg, chunk)
    got = g.search_raw(q, K, w)
    st = assert_fast(g)
    if qg:
        assert st["last_qg"] <= qg, st
    if chunk:
        assert st["last_chunk"] == chunk, st
    g.set_tuning(0, 0)
    return got, st


# ---- 1. the kernel at K > 64 -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_lists(native):
    ix = u16_ref.make_index(4242, 40000, 32, 4, 4, 1024, perm_labels=True, ndistinct=5000)
    g = u16_index(native, ix)
    q = np.random.default_rng(9).random((96, 32), dtype=f32)
    g.search_raw(q, 64, 1)
    lds64 = assert_fast(g)["last_scan_lds"]
    assert lds64 == small_lds(4, 8)
    g.set_table_mode(10)
    return ix, g, q, lds64


@pytest.mark.parametrize("w", [1, 4])
@pytest.mark.parametrize("K", [65, 100, 192, 193, 1000])
def test_mode_10_runs_the_kernel_above_64(long_lists, K, w):
    """Four lists of ~10 000 points (several 1024-point passes per chunk, several chunks), 96 queries; K = 192 / 193 straddle cap 256 / 512.
    Forced qg = 1 / 2 / 4 / 8 with chunks of 4096 and automatic: the kernel runs (last_qg >= 1, not above the forced value, the planned
    one; more LDS than the K = 64 kernel) and returns the generic path's bytes, which equal numpy on the first 8 queries."""
    ix, g, q, lds64 = long_lists
    gen = generic_of(g, q, K, w)
    assert_exact(tuple(a[:8] for a in gen), u16_ref.knn(ix, q[:8], K, w), "generic vs numpy K=%d w=%d" % (K, w))
    for qg in (1, 2, 4, 8):
        for chunk in (4096, 0):
            got, st = wide(g, q, K, w, qg, chunk)
            assert st["last_qg"] == planned_qg(4, 8, qg, K), st
            assert st["last_scan_lds"] == wide_lds(4, 8, st["last_qg"], cap_of(K)) > lds64, st
            assert_exact(got, gen, "K=%d w=%d qg=%d chunk=%d" % (K, w, qg, chunk))
            same_bytes(got, gen, "bytes K=%d w=%d qg=%d chunk=%d" % (K, w, qg, chunk))
    got, st = wide(g, q, K, w)                    # the plan's own grouping
    assert st["last_scan_lds"] > lds64, st
    same_bytes(got, gen, "automatic K=%d w=%d" % (K, w))


# ---- 2. what mode 10 must not touch ----------------------------------------------------------------------------------------------------
def test_mode_0_and_small_k_are_untouched(native):
    ix = u16_ref.make_index(4243, 20000, 32, 8, 4, 1024, perm_labels=True, ndistinct=3000)
    g = u16_index(native, ix)
    q = np.random.default_rng(10).random((64, 32), dtype=f32)
    keys = ("last_qg", "last_chunk", "last_scan_lds")
    res = {}
    for mode in (0, 10):
        g.set_table_mode(mode)
        for K in (1, 10, 64):
            got = g.search_raw(q, K, 3)
            st = assert_fast(g)
            res[mode, K] = (got, tuple(st[k] for k in keys))
    for K in (1, 10, 64):
        assert res[0, K][1] == res[10, K][1], (K, res[0, K][1], res[10, K][1])
        same_bytes(res[0, K][0], res[10, K][0], "K=%d under mode 10 vs mode 0" % K)
    exp = u16_ref.knn(ix, q[:6], 100, 3)
    assert_exact(tuple(a[:6] for a in g.search_raw(q, 100, 3)), exp, "mode 10 K=100")
    assert_fast(g)
    for mode in range(10):                        # modes 0 ... 9: K > 64 on a 16-bit handle is the generic path's
        g.set_table_mode(mode)
        assert_exact(tuple(a[:6] for a in g.search_raw(q, 100, 3)), exp, "mode %d K=100" % mode)
        assert_generic(g)
    from ivfadc_jl_amd import _native as nat
    with pytest.raises(nat.IVFADCError) as e:
        g.set_table_mode(11)
    assert e.value.code == nat.ERR_INVALID


# ---- 3. ties and short pools -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_ties_across_waves_passes_chunks_pairs_and_lists(native, which):
    """Few distinct codes: keys of equal distance span waves, passes, chunks, pairs and lists, and K = 65 / 130 cut through a group of them
    (every list holds >= 10 000 points of one distance, or of dc itself).  The visit order alone decides; byte-equal to the generic path,
    which equals numpy on a sample."""
    name, ix, q = _tie_indexes()[which]
    g = u16_index(native, ix)
    g.set_table_mode(10)
    sub = np.array([0, 1, 3, 5, 20])
    for K, w in ((65, 2), (130, 3)):
        gen = generic_of(g, q, K, w)
        assert_exact(tuple(a[sub] for a in gen), u16_ref.knn(ix, q[sub], K, w), "%s generic K=%d w=%d" % (name, K, w))
        for qg in (1, 2, 4, 8):
            for chunk in (4096, 0):
                for prune in (False, True):
                    g.set_pruning(prune)
                    got, st = wide(g, q, K, w, qg, chunk)
                    assert st["last_qg"] == qg, st
                    same_bytes(got, gen, "%s K=%d w=%d qg=%d chunk=%d pruning=%s" % (name, K, w, qg, chunk, prune))
        g.set_pruning(True)


def test_short_pools_and_empty_lists(native):
    """Probed lists that hold fewer than K points in total (counts < K; the slots beyond the count are not compared), and an index with
    every third list empty."""
    ix = u16_ref.make_index(31, 150, 16, 8, 2, 1024, ndistinct=20)
    g = u16_index(native, ix)
    g.set_table_mode(10)
    q = np.random.default_rng(31).random((24, 16), dtype=f32)
    for K, w in ((65, 2), (130, 3), (130, 8)):
        exp = u16_ref.knn(ix, q, K, w)
        assert (exp[2] < K).all() if w < 8 else (exp[2] == 130).all(), exp[2]
        gen = generic_of(g, q, K, w)
        assert_exact(gen, exp, "generic short K=%d w=%d" % (K, w))
        for qg in (1, 4, 8):
            got, _ = wide(g, q, K, w, qg)
            assert_exact(got, exp, "short pools K=%d w=%d qg=%d" % (K, w, qg))
    ix = u16_ref.make_index(32, 6000, 16, 30, 2, 1024, empty_every=3, ndistinct=400)
    g = u16_index(native, ix)
    g.set_table_mode(10)
    q = np.random.default_rng(32).random((40, 16), dtype=f32)
    for K, w in ((100, 6), (300, 30)):
        exp = u16_ref.knn(ix, q[:10], K, w)
        gen = generic_of(g, q, K, w)
        assert_exact(tuple(a[:10] for a in gen), exp, "generic, empty lists K=%d w=%d" % (K, w))
        for qg in (1, 8, 0):
            got, _ = wide(g, q, K, w, qg)
            assert_exact(got, gen, "empty lists K=%d w=%d qg=%d" % (K, w, qg))


# ---- 4. the LDS boundary, both sides -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,kmax,low_k", [(8, 1984, 1000), (3064, 960, 100)])
def test_lds_boundary_both_sides(native, d, kmax, low_k):
    """m = 1: 32 (dsp + qg cap) + 32 912 B <= 160 KB.  The largest K that fits at qg = 1 (derived here from the formula; 1984 at d = 8,
    where only cap = 4096 fails, 960 at d = 3064) runs the kernel, K + 1 goes generic; a forced qg = 8 is lowered at K = low_k to what the
    formula gives.  Exact on both sides."""
    fits = [K for K in range(65, 2049) if planned_qg(1, d, 1, K)]
    assert max(fits) == kmax and planned_qg(1, d, 1, kmax + 1) == 0 and fits == list(range(65, kmax + 1))
    ix = u16_ref.make_index(d, 2600 if d == 8 else 1300, d, 2, 1, 257, ndistinct=700)
    g = u16_index(native, ix)
    g.set_table_mode(10)
    q = np.random.default_rng(d).random((12, d), dtype=f32)
    exp = u16_ref.knn(ix, q[:3], kmax + 1, 2)
    got, st = wide(g, q, kmax, 2)
    assert st["last_qg"] == 1 and st["last_scan_lds"] == wide_lds(1, d, 1, cap_of(kmax)) <= LDS_MAX, st
    assert_exact(tuple(a[:3] for a in got), (exp[0][:, :kmax], exp[1][:, :kmax], np.minimum(exp[2], kmax)), "d=%d K=%d" % (d, kmax))
    same_bytes(got, generic_of(g, q, kmax, 2), "d=%d K=%d vs generic" % (d, kmax))
    over = g.search_raw(q, kmax + 1, 2)
    assert_generic(g)
    assert_exact(tuple(a[:3] for a in over), exp, "d=%d K=%d" % (d, kmax + 1))
    want = planned_qg(1, d, 8, low_k)
    assert 1 <= want < 8
    got, st = wide(g, q, low_k, 2, qg=8)
    assert st["last_qg"] == want and st["last_scan_lds"] == wide_lds(1, d, want, cap_of(low_k)), st
    assert wide_lds(1, d, 2 * want, cap_of(low_k)) > LDS_MAX
    same_bytes(got, generic_of(g, q, low_k, 2), "d=%d K=%d lowered qg vs generic" % (d, low_k))
    assert_exact(tuple(a[:3] for a in got), (exp[0][:, :low_k], exp[1][:, :low_k], np.minimum(exp[2], low_k)), "d=%d K=%d" % (d, low_k))


# ---- 5. tiled tables -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ksub", [8193, 65536])
def test_selectors_survive_the_tile_loop(native, ksub):
    """ksub = 65536 (8 ... 64 tiles per sub-space) and 8193 (a last tile of one codeword) at K = 100: the tables are rebuilt per tile, the
    selectors sit beside them."""
    ix = u16_ref.make_index(ksub, 3000, 4, 3, 2, ksub)
    g = u16_index(native, ix)
    g.set_table_mode(10)
    q = np.random.default_rng(ksub).random((24, 4), dtype=f32)
    for w in (1, 3):
        exp = u16_ref.knn(ix, q[:8], 100, w)
        gen = generic_of(g, q, 100, w)
        assert_exact(tuple(a[:8] for a in gen), exp, "generic ksub=%d w=%d" % (ksub, w))
        for qg in (1, 2, 4, 8):
            got, st = wide(g, q, 100, w, qg)
            assert st["last_qg"] == qg, st
            same_bytes(got, gen, "ksub=%d w=%d qg=%d" % (ksub, w, qg))


# ---- 6. pruning and the serving entries --------------------------------------------------------------------------------------------------
def test_pruning_changes_nothing(native):
    """Well separated cells, queries next to the centroids: probe pruning fires (pruned_points > 0) and K = 100 returns the same bytes with
    it on and off."""
    rng = np.random.default_rng(90)
    kc, d, m, nq = 40, 32, 4, 512
    cent = (rng.random((kc, d), dtype=f32) * f32(4.0)).astype(f32)
    ix = u16_ref.make_index(90, 40000, d, kc, m, 1024, centroids=cent, scale=0.05)
    q = (cent[rng.integers(0, kc, nq)] + (rng.random((nq, d), dtype=f32) - f32(0.5)) * f32(0.1)).astype(f32)
    g = u16_index(native, ix)
    g.set_table_mode(10)
    sub = np.arange(0, nq, 64)
    exp = u16_ref.knn(ix, q[sub], 100, 8)
    fired = 0
    for qg in (1, 4):
        res = {}
        for prune in (False, True):
            g.set_pruning(prune)
            g.reset_stats()
            res[prune], st = wide(g, q, 100, 8, qg, 1024)
            assert st["last_qg"] == qg, st
            if prune:
                fired += st["pruned_points"] > 0
            else:
                assert st["pruned_points"] == 0, st
        same_bytes(res[True], res[False], "pruning on vs off qg=%d" % qg)
        assert_exact(tuple(a[sub] for a in res[True]), exp, "pruned qg=%d" % qg)
    assert fired > 0


def test_serving_entries(native):
    """search_device, search_batches, a view cloned after mode 10 was set (it must run the kernel, not the generic path) and host memory
    from ivfadc_host_alloc: the bytes of search_raw."""
    import torch
    ix = u16_ref.make_index(77, 8000, 32, 32, 4, 1024, perm_labels=True)
    g = u16_index(native, ix)
    g.set_table_mode(10)
    q = np.random.default_rng(2).random((300, 32), dtype=f32)
    K, w = 100, 8
    exp = g.search_raw(q, K, w)
    assert_fast(g)
    assert_exact(tuple(x[:10] for x in exp), u16_ref.knn(ix, q[:10], K, w), "search_raw")
    dq = torch.from_numpy(q).cuda()
    di = torch.zeros((300, K), dtype=torch.int32, device="cuda")
    dd = torch.zeros((300, K), dtype=torch.float32, device="cuda")
    dc = torch.zeros(300, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g.search_device(300, dq.data_ptr(), K, w, di.data_ptr(), dd.data_ptr(), dc.data_ptr())
    g.sync()
    assert_fast(g)
    assert_exact((di.cpu().numpy().view(np.uint32), dd.cpu().numpy(), dc.cpu().numpy()), exp, "search_device")
    outs = g.search_batches_raw([q[:100], q[100:101], q[101:]], K, w)
    assert_exact(tuple(np.concatenate([o[i] for o in outs]) for i in range(3)), exp, "search_batches")
    assert_fast(g)
    v = g.clone_view()
    assert_exact(v.search_raw(q, K, w), exp, "view")
    assert_fast(v)
    lib = native.load_library()
    p = C.c_void_p()
    assert lib.ivfadc_host_alloc(C.c_size_t(q.nbytes), C.byref(p)) == 0
    try:
        hq = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(300, 32))
        hq[:] = q
        assert_exact(g.search_raw(hq, K, w), exp, "host_alloc")
        assert_fast(g)
    finally:
        lib.ivfadc_host_free(p)


# ---- 7. an 8-bit handle ----------------------------------------------------------------------------------------------------------------
def test_8bit_handle_plans_what_mode_0_plans(native):
    oidx, data = helpers.build_index(15, 4000, 64, 40, 8, ksub=256, label_perm=True, mode="random", ndistinct=300)
    g = native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)
    assert g.code_type == np.uint8
    q = data[:48] + 0.01
    keys = ("last_qg", "last_chunk", "last_scan_lds", "last_striped", "last_nf")
    for K, w in ((10, 4), (100, 8)):
        res = {}
        for mode in (0, 10):
            g.set_table_mode(mode)
            got = g.search_raw(q, K, w)
            st = g.get_stats()
            res[mode] = (got, tuple(st[k] for k in keys))
        assert res[0][1] == res[10][1], (K, res[0][1], res[10][1])
        same_bytes(res[0][0], res[10][0], "8-bit K=%d: mode 10 vs mode 0" % K)
        assert_exact(res[10][0], oidx.knn_search(q, K, w), "8-bit K=%d vs the oracle" % K)
