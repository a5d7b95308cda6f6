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
