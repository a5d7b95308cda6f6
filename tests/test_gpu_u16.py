"""GPU tests of indexes with UInt16 codes (csrc/u16scan.hip.h and the 16-bit generic path): cross-width equality with 8-bit indexes
and the C oracle, true 16-bit shapes against the numpy restatement (tests/u16_ref.py), the fast kernel against the generic path,
the life cycle (train, encode, push!, delete, save / load) and every search entry.  Ids and distance bits are compared exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import u16_ref
from u16_ref import assert_exact

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def u16_index(native, ix):
    return native.IVFADCIndex.from_arrays(ix.centroids, ix.codebooks, ix.labels.astype(np.uint16), ix.offsets, ix.codes.astype(np.uint16),
                                          ix.ids)


def path_of(g):
    st = g.get_stats()
    return "generic" if st["last_qg"] == -2 else "u16"


@pytest.mark.parametrize("d,m", [(128, 8), (96, 16), (64, 4)])
def test_cross_width_equality(native, d, m):
    """An 8-bit index re-expressed as 16-bit (same quantizers, uint16 labels -- identity and permuted -- widened codes) returns what the
    oracle and the 8-bit handle return, bit for bit."""
    for perm in (False, True):
        oidx, data = helpers.build_index(7 + m, 4000, d, 40, m, ksub=256, label_perm=perm, mode="random", ndistinct=300)
        g8 = native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)
        g16 = native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels.astype(np.uint16), oidx.offsets,
                                             oidx.codes.astype(np.uint16), oidx.ids)
        assert g16.code_type == np.uint16 and g8.code_type == np.uint8
        q = data[:48] + 0.01
        for K in (1, 10, 64, 100):
            for w in (1, 8, 64, oidx.kc):
                exp = oidx.knn_search(q, K, w)
                got = g16.search_raw(q, K, w)
                assert_exact(got, exp, "u16 d=%d m=%d K=%d w=%d perm=%s" % (d, m, K, w, perm))
                assert path_of(g16) == ("generic" if K > 64 else "u16")
                if K <= 64:
                    assert g16.get_stats()["last_qg"] >= 1 and g16.get_stats()["last_scan_lds"] > 0
                assert_exact(g8.search_raw(q, K, w), exp, "u8")


SHAPES = [  # (ksub, d, m, kc, n, K, w)
    (257, 32, 4, 16, 3000, 10, 4),
    (1024, 64, 8, 24, 5000, 64, 8),
    (4096, 32, 4, 12, 2500, 5, 12),       # tiles of codewords at eight pairs per item (T = 1024)
    (65536, 16, 2, 6, 600, 10, 3),        # tiles at any grouping
]


@pytest.mark.parametrize("ksub,d,m,kc,n,K,w", SHAPES)
def test_true_16bit_shapes(native, ksub, d, m, kc, n, K, w):
    ix = u16_ref.make_index(100 + ksub, n, d, kc, m, ksub, perm_labels=True, empty_every=5, ndistinct=n // 3)
    g = u16_index(native, ix)
    rng = np.random.default_rng(ksub)
    q = rng.random((24, d), dtype=np.float32)
    for KK, ww in ((K, w), (1, 1), (n + 5, kc)):       # the last: K > total points, every list probed (generic path)
        exp = u16_ref.knn(ix, q, KK, ww)
        got = g.search_raw(q, KK, ww)
        assert_exact(got, exp, "ksub=%d K=%d w=%d" % (ksub, KK, ww))
    # lists shorter than K
    exp = u16_ref.knn(ix, q, 64, 1)
    assert_exact(g.search_raw(q, 64, 1), exp, "short lists")


def test_fast_kernel_and_generic_path_agree(native):
    for ksub, d, m in ((1024, 64, 8), (4096, 32, 4)):
        ix = u16_ref.make_index(5 + ksub, 20000, d, 64, m, ksub, perm_labels=True, ndistinct=2000)
        g = u16_index(native, ix)
        q = np.random.default_rng(3).random((512, d), dtype=np.float32)
        for K, w in ((10, 8), (64, 16), (1, 1)):
            for qg in (0, 1, 2, 4, 8):
                g.set_tuning(qg, 0)
                fast = g.search_raw(q, K, w)
                assert path_of(g) == "u16"
                g.set_tuning(-2, 0)
                gen = g.search_raw(q, K, w)
                assert path_of(g) == "generic"
                assert_exact(fast, gen, "fast vs generic ksub=%d K=%d w=%d qg=%d" % (ksub, K, w, qg))
            g.set_tuning(0, 0)


def test_life_cycle(native, tmp_path):
    rng = np.random.default_rng(11)
    data = rng.random((6000, 32), dtype=np.float32)
    a = native.IVFADCIndex(data[:5000], kc=16, k=1024, m=4, seed=3, coarse_maxiter=5, quantization_maxiter=5)
    b = native.IVFADCIndex(data[:5000], kc=16, k=1024, m=4, seed=3, coarse_maxiter=5, quantization_maxiter=5)
    assert a.code_type == np.uint16 and "UInt16" in repr(a.inverse_index[0]) and "(4 + 2×4)" in repr(a)
    oa, ca, ia = a._lists()
    ob, cb, ib = b._lists()
    assert np.array_equal(a._codebooks, b._codebooks) and np.array_equal(oa, ob) and np.array_equal(ca, cb) and np.array_equal(ia, ib)

    def ref_of(g):
        off, codes, ids = g._lists()
        return u16_ref.U16Index(g._centroids, g._codebooks, g._labels, off, codes, ids)

    # encode: numpy argmin, ties to the first codeword; labels out (non-identity labels: a permuted copy of the trained quantizer)
    perm = np.stack([rng.permutation(65536)[:1024] for _ in range(4)]).astype(np.uint16)
    p = native.IVFADCIndex.from_arrays(a._centroids, a._codebooks, perm, index_type=np.uint32)
    tie_cbs = a._codebooks.copy()
    tie_cbs[:, 5] = tie_cbs[:, 900]                       # duplicate codewords: exact ties
    t = native.IVFADCIndex.from_arrays(a._centroids, tie_cbs, perm, index_type=np.uint32)
    for g in (p, t):
        ref = u16_ref.U16Index(g._centroids, g._codebooks, g._labels, np.zeros(17, np.int64), np.zeros((0, 4), np.uint16), np.zeros(0, np.uint32))
        gl, gc = g.encode(data[:300])
        el, ec = u16_ref.encode(ref, data[:300])
        assert np.array_equal(gl, el) and np.array_equal(gc, ec)
    # push! in place, then search
    p._append(data[:3000], np.arange(3000, dtype=np.uint32))
    p.search_raw(data[:4], 1, 1)                          # lays the lists out on the device (with spare capacity)
    before = p.get_stats()["inplace_appends"]
    p._append(data[3000:3100], np.arange(3000, 3100, dtype=np.uint32))
    assert p.get_stats()["inplace_appends"] == before + 1
    q = data[5000:5040] + 0.003
    assert_exact(p.search_raw(q, 10, 4), u16_ref.knn(ref_of(p), q, 10, 4), "after push!")
    # delete / pop / pushfirst, then search
    assert p._delete_ids(np.array([0, 17, 2999, 3050], np.uint32)) == 4
    p._shift_ids(1)
    assert_exact(p.search_raw(q, 10, 4), u16_ref.knn(ref_of(p), q, 10, 4), "after delete + shift")
    # save -> load -> save, byte for byte; the loaded index searches the same
    f1, f2 = os.path.join(str(tmp_path), "a.bin"), os.path.join(str(tmp_path), "b.bin")
    native.save_ivfadc_index(f1, p)
    l = native.load_ivfadc_index(f1)
    assert l.code_type == np.uint16 and np.array_equal(l._labels, perm)
    native.save_ivfadc_index(f2, l)
    assert open(f1, "rb").read() == open(f2, "rb").read()
    assert_exact(l.search_raw(q, 10, 4), p.search_raw(q, 10, 4), "loaded")
    # the committed fixture
    fx = native.load_ivfadc_index(os.path.join(GOLDEN, "persistency_u16_codes.bin"))
    qq = np.random.default_rng(1).random((16, 4), dtype=np.float32) * 3
    for K, w in ((3, 1), (9, 3)):
        assert_exact(fx.search_raw(qq, K, w), u16_ref.knn(ref_of(fx), qq, K, w), "fixture")
    f3 = os.path.join(str(tmp_path), "c.bin")
    native.save_ivfadc_index(f3, fx)
    assert open(f3, "rb").read() == open(os.path.join(GOLDEN, "persistency_u16_codes.bin"), "rb").read()


def test_every_search_entry_returns_the_same_bytes(native):
    import torch
    ix = u16_ref.make_index(77, 8000, 32, 32, 4, 1024, perm_labels=True)
    g = u16_index(native, ix)
    q = np.random.default_rng(2).random((300, 32), dtype=np.float32)
    K, w = 10, 8
    exp = g.search_raw(q, K, w)
    sub = u16_ref.knn(ix, q[:20], K, w)
    assert_exact(tuple(x[:20] for x in exp), sub, "ivfadc_search")
    # device pointers
    dq = torch.from_numpy(q).cuda()
    di = torch.zeros((300, K), dtype=torch.int32, device="cuda")
    dd = torch.zeros((300, K), dtype=torch.float32, device="cuda")
    dc = torch.zeros(300, dtype=torch.int32, device="cuda")
    g.search_device(300, dq.data_ptr(), K, w, di.data_ptr(), dd.data_ptr(), dc.data_ptr())
    torch.cuda.synchronize()
    assert_exact((di.cpu().numpy().view(np.uint32), dd.cpu().numpy(), dc.cpu().numpy()), exp, "search_device")
    # batches
    outs = g.search_batches_raw([q[:100], q[100:]], K, w)
    got = tuple(np.concatenate([o[i] for o in outs]) for i in range(3))
    assert_exact(got, exp, "search_batches")
    # a view
    v = g.clone_view()
    assert_exact(v.search_raw(q, K, w), exp, "view")
    # caller host memory from ivfadc_host_alloc
    lib = native.load_library()
    p = C.c_void_p()
    nbytes = q.nbytes
    assert lib.ivfadc_host_alloc(C.c_size_t(nbytes), C.byref(p)) == 0
    try:
        hq = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(300, 32))
        hq[:] = q
        assert_exact(g.search_raw(hq, K, w), exp, "host_alloc")
    finally:
        lib.ivfadc_host_free(p)
    # the uint8_t entries refuse a 16-bit handle (ERR_STATE), naming the _u16 entry
    assert lib.ivfadc_get_lists(g._h, None, None, None) == 4 and b"_u16" in lib.ivfadc_last_error()
    assert lib.ivfadc_set_list_partition(g._h, 2, 0) == 2


def test_randomised_differential(native):
    rng = np.random.default_rng(2024)
    for draw in range(24):
        m = int(rng.choice([1, 2, 4, 8]))
        dsub = int(rng.choice([1, 2, 3, 4, 8]))
        d = m * dsub
        ksub = int(rng.choice([1, 17, 257, 1000, 2048, 5000]))
        kc = int(rng.integers(2, 40))
        n = int(rng.integers(0, 3000))
        ix = u16_ref.make_index(3000 + draw, n, d, kc, m, ksub, perm_labels=bool(rng.integers(0, 2)),
                                empty_every=int(rng.choice([0, 3])), ndistinct=int(rng.choice([0, 5, 50])))
        g = u16_index(native, ix)
        q = rng.random((int(rng.integers(1, 40)), d), dtype=np.float32)
        K = int(rng.choice([1, 3, 10, 64, 65]))
        w = int(rng.integers(1, kc + 1))
        assert_exact(g.search_raw(q, K, w), u16_ref.knn(ix, q, K, w), "draw %d" % draw)
        if n > 10 and draw % 3 == 0:     # interleaved mutation: delete a few ids, search again
            dels = rng.choice(n, 5, replace=False).astype(np.uint32)
            g._delete_ids(dels)
            off, codes, ids = g._lists()
            ix2 = u16_ref.U16Index(ix.centroids, ix.codebooks, ix.labels, off, codes, ids)
            assert_exact(g.search_raw(q, K, w), u16_ref.knn(ix2, q, K, w), "draw %d after delete" % draw)


def test_long_lists_several_passes_per_chunk(native):
    """Chunks of 4096 / 8192 points (set_tuning) on lists of ~10 000 points: each work item walks several 1024-point passes (tables
    rebuilt per pass, sums restarted, selectors carried over) -- against the generic path and numpy."""
    ix = u16_ref.make_index(4242, 40000, 32, 4, 4, 1024, perm_labels=True, ndistinct=5000)
    g = u16_index(native, ix)
    q = np.random.default_rng(9).random((96, 32), dtype=np.float32)
    g.set_tuning(-2, 0)
    gen = {(K, w): g.search_raw(q, K, w) for K, w in ((10, 2), (64, 4), (1, 1))}
    for (K, w), exp in gen.items():
        assert_exact(tuple(x[:8] for x in exp), u16_ref.knn(ix, q[:8], K, w), "generic vs numpy K=%d w=%d" % (K, w))
        for qg in (1, 2, 4, 8):
            for chunk in (4096, 8192, 0):
                g.set_tuning(qg, chunk)
                got = g.search_raw(q, K, w)
                st = g.get_stats()
                assert st["last_qg"] == qg
                if chunk:
                    assert st["last_chunk"] == chunk
                assert_exact(got, exp, "K=%d w=%d qg=%d chunk=%d" % (K, w, qg, chunk))
    g.set_tuning(0, 0)


def test_sift1m_shape_k1024(native):
    """SIFT1M shape at k = 1024: n = 1e6, d = 128, kc = 1024, m = 8, trained; 1024 queries, K = 10, w = 8.  64 sampled queries equal
    numpy bit for bit; the whole batch is byte-equal between the fast kernel and the generic path."""
    rng = np.random.default_rng(1234)
    n, d = 1_000_000, 128
    centres = rng.random((256, d), dtype=np.float32)
    data = (centres[rng.integers(0, 256, n)] + rng.normal(0, 0.08, (n, d))).astype(np.float32)
    g = native.IVFADCIndex(data, kc=1024, k=1024, m=8, seed=5, coarse_maxiter=4, quantization_maxiter=4)
    assert g.code_type == np.uint16 and len(g) == n
    q = (data[rng.integers(0, n, 1024)] + rng.normal(0, 0.02, (1024, d))).astype(np.float32)
    fast = g.search_raw(q, 10, 8)
    st = g.get_stats()
    assert st["last_qg"] >= 1 and st["last_scan_lds"] > 0
    g.set_tuning(-2, 0)
    gen = g.search_raw(q, 10, 8)
    assert g.get_stats()["last_qg"] == -2
    g.set_tuning(0, 0)
    for a, b in zip(fast, gen):
        assert a.tobytes() == b.tobytes()
    off, codes, ids = g._lists()
    ref = u16_ref.U16Index(g._centroids, g._codebooks, g._labels, off, codes, ids)
    sample = rng.choice(1024, 64, replace=False)
    exp = u16_ref.knn(ref, q[sample], 10, 8)
    assert_exact(tuple(x[sample] for x in fast), exp, "SIFT1M k=1024 sample")
