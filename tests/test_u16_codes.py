"""CPU checks of the UInt16-code boundary (ivfadc_create_u16, the UInt16 file gate, the Python gates), of the numpy restatement the GPU
tests of 16-bit indexes compare against, and of the new kernels' resources.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers
import u16_ref
from oracle import oracle as ora

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _create_u16(lib, d, m, ksub, labels):
    h = C.c_void_p()
    z = np.zeros(max(1, d * max(ksub, 2)), np.float32)
    lab = np.ascontiguousarray(labels, np.uint16)
    fp = C.POINTER(C.c_float)
    return lib.ivfadc_create_u16(C.byref(h), 0, d, 2, m, ksub, z.ctypes.data_as(fp), z.ctypes.data_as(fp), lab.ctypes.data_as(C.c_void_p))


def test_create_u16_validation_before_any_device_call(native):
    lib = native.load_library()
    assert _create_u16(lib, 4, 2, 65537, np.zeros(2 * 65537, np.uint16)) == 2
    dup = np.tile(np.arange(300, dtype=np.uint16), (2, 1))
    dup[1, 7] = dup[1, 8]
    assert _create_u16(lib, 4, 2, 300, dup) == 2 and b"duplicate label" in lib.ivfadc_last_error()
    assert _create_u16(lib, 5, 2, 300, np.tile(np.arange(300, dtype=np.uint16), (2, 1))) == 2
    assert b"d % m" in lib.ivfadc_last_error()
    assert _create_u16(lib, 2, 3, 300, np.tile(np.arange(300, dtype=np.uint16), (3, 1))) == 1
    # ivfadc_create keeps refusing ksub > 256
    h = C.c_void_p()
    z = np.zeros(4 * 300, np.float32)
    lab8 = np.zeros(600, np.uint8)
    fp = C.POINTER(C.c_float)
    assert lib.ivfadc_create(C.byref(h), 0, 4, 2, 2, 300, z.ctypes.data_as(fp), z.ctypes.data_as(fp), lab8.ctypes.data_as(C.POINTER(C.c_uint8))) == 2


def _load_rc(lib, data, tmp_path):
    p = os.path.join(str(tmp_path), "f.bin")
    open(p, "wb").write(data)
    h = C.c_void_p()
    bits = C.c_int(0)
    rc = lib.ivfadc_load_index(C.byref(h), 0, p.encode(), C.byref(bits))
    if rc == 0:
        lib.ivfadc_destroy(h)
    return rc, lib.ivfadc_last_error().decode()


def _fixture_offsets(good):
    """Byte offsets of the first label of codebook 1 and of the first code of list 1 in the UInt16 fixture."""
    hdr = len(good) - len(good.split(b"Float32\n", 1)[1])
    d, kc, m, k, dsub = 4, 3, 2, 300, 2
    lab0 = hdr + 4 * d * kc
    list0 = lab0 + m * (2 * k + 4 * dsub * k) + 4 * d * d
    code0 = list0 + 8 + 4 * 5
    return lab0, code0


def test_uint16_file_gate(native, tmp_path):
    lib = native.load_library()
    good = open(os.path.join(GOLDEN, "persistency_u16_codes.bin"), "rb").read()
    rc, msg = _load_rc(lib, good, tmp_path)
    # a well-formed UInt16 file passes the gate; without a GPU the call then ends at device init (not at the gate: rc != 2)
    assert rc != 2, msg
    lab0, code0 = _fixture_offsets(good)
    dup = bytearray(good)
    dup[lab0 + 2:lab0 + 4] = dup[lab0:lab0 + 2]
    rc, msg = _load_rc(lib, bytes(dup), tmp_path)
    assert rc == 2 and "duplicate label" in msg, msg
    bad = bytearray(good)
    bad[code0:code0 + 2] = np.uint16(1).tobytes()           # 1 = label(1, c) for no c (labels are 217 c mod 65536)
    rc, msg = _load_rc(lib, bytes(bad), tmp_path)
    assert rc == 2 and "not a label" in msg, msg
    rc, msg = _load_rc(lib, good[:-3], tmp_path)
    assert rc == 2, msg


def test_python_gates(native):
    data = np.random.default_rng(0).random((70000, 2), dtype=np.float32)
    with pytest.raises(NotImplementedError):
        native.IVFADCIndex(data, kc=2, k=65537, m=1)
    small = data[:2000]
    try:
        native.IVFADCIndex(small, kc=2, k=1024, m=1)
    except NotImplementedError:
        pytest.fail("k = 1024 must pass the Python gate")
    except (native.IVFADCError, AssertionError, RuntimeError):
        pass        # no GPU here: the native trainer refuses to run, after the gate


def test_numpy_restatement_equals_oracle_on_8bit_data():
    """u16_ref (16-bit codes, the tests' reference for 16-bit indexes) against the pinned C oracle on 8-bit indexes re-expressed as
    16-bit: ids and distance bits identical."""
    for seed, (d, kc, m, ksub, perm) in enumerate([(32, 12, 4, 256, True), (24, 9, 8, 100, False), (16, 5, 2, 256, True)]):
        oidx, data = helpers.build_index(40 + seed, 600, d, kc, m, ksub=ksub, label_perm=perm, mode="random", ndistinct=40)
        ix = u16_ref.U16Index(oidx.centroids, oidx.codebooks, oidx.labels.astype(np.uint16), oidx.offsets,
                              oidx.codes.astype(np.uint16), oidx.ids)
        q = data[:12] + 0.01
        for K, w in ((1, 1), (10, 3), (64, kc)):
            oi, od, oc = oidx.knn_search(q, K, w)
            ui, ud, uc = u16_ref.knn(ix, q, K, w)
            assert np.array_equal(oc, uc)
            for r in range(q.shape[0]):
                c = int(oc[r])
                assert np.array_equal(oi[r, :c], ui[r, :c]), (seed, K, w, r)
                assert np.array_equal(od[r, :c].view(np.uint32), ud[r, :c].view(np.uint32)), (seed, K, w, r)
        # _encode_point: labels of the first minimum
        ol, ocodes = oidx.encode(data[:50])
        ul, ucodes = u16_ref.encode(ix, data[:50])
        assert np.array_equal(ol, ul) and np.array_equal(ocodes.astype(np.uint16), ucodes)
    # the edges 8-bit data can express: +inf sums, zero codebooks with queries on centroids (every sum equals dc = +0), duplicate
    # centroids, dsub 5 / 7 / 32, empty lists probed with w = kc, K above the number of probed points
    for seed, (case, d, m) in enumerate([("inf_sums", 16, 4), ("zero_codebooks", 16, 4), ("dup_centroids", 16, 4), ("dsub5", 20, 4),
                                          ("dsub7", 28, 4), ("dsub32", 64, 2), ("empty_lists", 16, 4)]):
        kc = 10
        oidx, data = helpers.build_index(70 + seed, 400, d, kc, m, ksub=256, label_perm=True, mode="random", ndistinct=30)
        q = (data[:10] + np.float32(0.01)).astype(np.float32)
        if case == "inf_sums":
            u = np.random.default_rng(seed).random(oidx.codebooks.shape, dtype=np.float32)
            oidx.codebooks[:] = np.where(u < 0.5, np.float32(-1), np.float32(1)) * (np.float32(1) + u) * np.float32(1e20)
        elif case == "zero_codebooks":
            oidx.codebooks[:] = 0
            q[:5] = oidx.centroids[:5]
        elif case == "dup_centroids":
            oidx.centroids[5:] = oidx.centroids[:5]
            q[:5] = oidx.centroids[:5]
        elif case == "empty_lists":
            lens = np.diff(oidx.offsets)
            lens[[0, 3, 7]] = 0
            sel = np.concatenate([np.arange(oidx.offsets[l], oidx.offsets[l] + lens[l]) for l in range(kc)]).astype(np.int64)
            oidx.codes, oidx.ids = np.ascontiguousarray(oidx.codes[sel]), np.ascontiguousarray(oidx.ids[sel])
            oidx.offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ix = u16_ref.U16Index(oidx.centroids, oidx.codebooks, oidx.labels.astype(np.uint16), oidx.offsets, oidx.codes.astype(np.uint16),
                              oidx.ids)
        if case == "inf_sums":
            assert np.isinf(u16_ref.knn(ix, q, 5, 2)[1]).all()
        for K, w in ((1, 1), (10, 3), (64, 2), (500, kc)):
            oi, od, oc = oidx.knn_search(q, K, w)
            ui, ud, uc = u16_ref.knn(ix, q, K, w)
            assert np.array_equal(oc, uc), (case, K, w)
            for r in range(q.shape[0]):
                c = int(oc[r])
                assert np.array_equal(oi[r, :c], ui[r, :c]), (case, K, w, r)
                assert np.array_equal(od[r, :c].view(np.uint32), ud[r, :c].view(np.uint32)), (case, K, w, r)
        assert (oc < 500).all()           # K = 500 is more than every list together holds


@pytest.mark.parametrize("ksub", [257, 4096, 65536])
def test_numpy_restatement_against_float64(ksub):
    """An independent check of u16_ref for ksub > 256, where nothing pins it to the C oracle: every returned distance is recomputed in
    float64 without tables, dc + sum_i |r_i - cw_i[label^-1(code_i)]|^2, through a label -> codeword map built from a dict (not
    u16_ref.inv); the returned ids are the float64 top-K of the float64 top-w lists, wherever the float64 gap at the w-th and at the
    K-th boundary is above the tolerance.  Catches a label-translation or indexing error the GPU code and u16_ref could share."""
    m, dsub = (2, 4) if ksub == 65536 else (4, 4)
    d, kc, K, w = m * dsub, 12, 10, 3
    ix = u16_ref.make_index(ksub + 1, 3000, d, kc, m, ksub, perm_labels=True)
    assert (ix.labels.astype(np.int64) != np.arange(ksub)).any()
    inv = [dict(zip(ix.labels[i].tolist(), range(ksub))) for i in range(m)]
    cb64 = ix.codebooks.astype(np.float64)
    cent64 = ix.centroids.astype(np.float64)
    lst_of = np.searchsorted(ix.offsets, np.arange(ix.codes.shape[0]), side="right") - 1
    cw = np.array([[inv[i][int(c)] for i, c in enumerate(row)] for row in ix.codes], np.int64)
    tol = 1e-5 * m
    q = np.random.default_rng(ksub).random((24, d), dtype=np.float32)
    ids, dists, cnt = u16_ref.knn(ix, q, K, w)
    checked = 0
    for r in range(q.shape[0]):
        q64 = q[r].astype(np.float64)
        dc = ((cent64 - q64) ** 2).sum(1)
        full = dc[lst_of] + sum(((cb64[i, cw[:, i]] - (q64 - cent64[lst_of])[:, i * dsub:(i + 1) * dsub]) ** 2).sum(1) for i in range(m))
        # every returned distance
        pos = np.array([int(np.nonzero(ix.ids == i)[0][0]) for i in ids[r, :cnt[r]]])
        # float32 sums against a float64 recomputation without tables: different arithmetic, so a tolerance (m roundings) and no bits
        assert np.allclose(dists[r, :cnt[r]], full[pos], rtol=tol, atol=0), (ksub, r)
        # the id set, where float64 separates the boundaries
        order = np.argsort(dc, kind="stable")
        if dc[order[w]] - dc[order[w - 1]] <= tol * dc[order[w]]:
            continue
        probed = np.isin(lst_of, order[:w])
        cand = np.nonzero(probed)[0]
        fo = cand[np.argsort(full[cand], kind="stable")]
        assert cnt[r] == min(K, cand.shape[0])
        if fo.shape[0] > K and full[fo[K]] - full[fo[K - 1]] <= tol * full[fo[K]]:
            continue
        assert set(ix.ids[fo[:K]].tolist()) == set(ids[r, :cnt[r]].tolist()), (ksub, r)
        checked += 1
    assert checked >= 12


def test_u16_kernel_resources(native):
    """No scratch in the new kernels; the scan kernel keeps three workgroups per CU (<= 168 VGPRs: 512 / 3 waves per SIMD)."""
    import test_resources as tr
    res = tr._kernel_resources(native.build_library())
    got = {k: v for k, v in res.items() if "u16" in k}
    names = ("u16_scan_kernel", "gen_dump_u16_kernel", "encode_u16_kernel")
    for frag in names:
        hits = [v for k, v in got.items() if frag in k]
        assert hits, "%s not in the code object" % frag
        for v in hits:
            assert v.get("vgpr_spill_count", 0) == 0, (frag, v)
            assert v.get("group_segment_fixed_size", 0) == 0, (frag, v)
    scan = [v for k, v in got.items() if "u16_scan_kernel" in k][0]
    assert scan["vgpr_count"] <= 168, scan


def test_u16_entries_exist(native):
    lib = native.load_library()
    for s in ("ivfadc_create_u16", "ivfadc_code_bits", "ivfadc_set_lists_u16", "ivfadc_get_lists_u16", "ivfadc_encode_u16",
              "ivfadc_append_u16", "ivfadc_get_quantizers_u16"):
        assert hasattr(lib, s), s
    assert lib.ivfadc_abi_version() == 4
