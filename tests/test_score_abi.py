"""CPU checks of the boundary of ivfadc_score_ids: both symbols declared and exported, the change additive (ABI version unchanged in
header, binding and shim), every argument error returned before the handle is looked at or the device is touched and named in
ivfadc_last_error(), empty calls accepted, the header comment's contract, and the Python surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["ivfadc_t *", "int64_t", "const float *", "int64_t", "int64_t", "const uint32_t *", "const int32_t *", "float *", "uint8_t *"]
ENTRIES = ("ivfadc_score_ids", "ivfadc_score_ids_device")
INVALID = 2


def _header():
    return open(os.path.join(ROOT, "include", "ivfadc_hip.h")).read()


def test_both_entries_are_declared_and_exported(native):
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    lib = native.load_library()
    # the type words of the other prototypes: the new entries use no other
    known = set()
    for name, arglist in re.findall(r"\bint\s+(ivfadc_\w+)\s*\(([^()]*)\)\s*;", code):
        if name not in ENTRIES:
            known |= {re.sub(r"\b\w+$", "", re.sub(r"\s+", " ", a.strip())).strip() for a in arglist.split(",")}
    assert set(ARGS) <= known, set(ARGS) - known
    for s in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % s, code)
        assert m, "%s is not declared in include/ivfadc_hip.h" % s
        args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        types = [re.sub(r"\b\w+$", "", a).strip() for a in args]
        assert types == ARGS, (s, args)
        assert hasattr(lib, s), "libivfadc_hip.so does not export %s" % s


def test_the_change_is_additive():
    hdr = _header()
    ver = int(re.search(r"#define\s+IVFADC_ABI_VERSION\s+(\d+)", hdr).group(1))
    from ivfadc_jl_amd import _native as nat
    jl = open(os.path.join(ROOT, "julia", "IVFADCHip.jl")).read()
    assert nat.ABI_VERSION == ver == int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1)) == 4
    assert "score_ids" not in jl, "the Julia shim is out of scope"
    stats = hdr[hdr.index("typedef struct {", hdr.index("scan_ms") - 200):hdr.index("} ivfadc_stats;")]
    assert "score_ids" not in stats, "ivfadc_stats is as it was"


def test_header_comment_states_the_contract():
    hdr = _header()
    block = hdr[hdr.index("SCORE caller-supplied candidate ids"):hdr.index("int ivfadc_score_ids_device(")]
    for needle in ("utils.jl:49-55", "coarsequantizers.jl:33-34", "coarsequantizers.jl:40-45", "index.jl:232-236", "index.jl:242-246", "LAST list",
                   "FIRST position", "list_len", "one rounding per operation", "nothing contracted", "LABEL", "BIT FOR BIT", "UInt16", "rotation",
                   ":opq", "NOT applied", "+Inf", "0x7F800000", "found = 0", "Not an error", "sort last", "d x nq", "ids_stride == C",
                   "ids_stride == 0", "shared row", "runs once", "counts may be NULL", "outside [0, C]", "clamps", "out_found", "may be NULL",
                   "slot by slot", "repeat", "0xFFFFFFFF", "2^31 - 1", "ivfadc_clone_view", "subset views", "dropped", "device-synthesised",
                   "push!", "laid out first", "IVFADC_ERR_STATE", "blocks", "only enqueues", "uploads nothing", "waits for nothing",
                   "ivfadc_sync", "per-handle lock", "ivfadc_set_workspace_limit", "slices of whole queries", "IVFADC_ERR_INVALID",
                   "before the handle is looked at", "nq == 0 or C == 0", "Not covered", "ivfadc_mg_", "list-partitioned", "ivfadc_search_batches"):
        assert needle in block, needle


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_validation_needs_no_gpu(native, entry):
    """each error decided before the handle is looked at or the device is touched, each named in ivfadc_last_error()"""
    lib = native.load_library()
    fn = getattr(lib, entry)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    q = np.zeros(64, np.float32)
    ids = np.arange(8, dtype=np.uint32)
    out = np.zeros(64, np.float32)
    qp, ip, op = C.c_void_p(q.ctypes.data), C.c_void_p(ids.ctypes.data), C.c_void_p(out.ctypes.data)
    fake = C.c_void_p(0x10)                      # never dereferenced: every call below is decided on its arguments

    def err():
        return lib.ivfadc_last_error()

    assert fn(None, 2, qp, 4, 4, ip, None, op, None) == INVALID and b"null handle" in err() and entry.encode() in err()
    assert fn(None, 0, qp, 4, 4, ip, None, op, None) == INVALID and b"null handle" in err()
    assert fn(fake, -1, qp, 4, 4, ip, None, op, None) == INVALID and b"nq = -1" in err() and entry.encode() in err()
    assert fn(fake, 2, qp, -3, -3, ip, None, op, None) == INVALID and b"C = -3" in err()
    for stride in (1, 3, 5, 8, -4):
        assert fn(fake, 2, qp, 4, stride, ip, None, op, None) == INVALID and b"ids_stride = %d" % stride in err(), stride
    assert fn(fake, 0, qp, 4, 3, ip, None, op, None) == INVALID and b"ids_stride" in err()       # (a bad stride is bad at nq == 0 too)
    # more than 2^31 - 1 pairs, in both stride forms; 2^31 - 1 itself passes this check (and fails on the next one here: null queries)
    for nq, ncand in ((1 << 31, 1), (1, 1 << 31), (65536, 32768), (1 << 40, 1 << 40), (46341, 46341)):
        for stride in (ncand, 0):
            assert fn(fake, nq, qp, ncand, stride, ip, None, op, None) == INVALID and b"pairs" in err() and b"2^31 - 1" in err(), (nq, ncand)
    for nq, ncand in (((1 << 31) - 1, 1), (1, (1 << 31) - 1), (46340, 46341)):
        assert fn(fake, nq, None, ncand, ncand, ip, None, op, None) == INVALID and b"null queries" in err(), (nq, ncand)
    assert fn(fake, 2, None, 4, 4, ip, None, op, None) == INVALID and b"null queries" in err()
    assert fn(fake, 2, qp, 4, 4, None, None, op, None) == INVALID and b"null ids" in err()
    assert fn(fake, 2, qp, 4, 0, None, None, op, None) == INVALID and b"null ids" in err()
    assert fn(fake, 2, qp, 4, 4, ip, None, None, None) == INVALID and b"null out_dists" in err()
    # nothing to score: OK, whatever the pointers are, and the handle is not looked at
    assert fn(fake, 0, None, 4, 4, None, None, None, None) == 0
    assert fn(fake, 0, None, 4, 0, None, None, None, None) == 0
    assert fn(fake, 2, None, 0, 0, None, None, None, None) == 0
    assert fn(fake, 0, None, 0, 0, None, None, None, None) == 0


def test_host_entry_refuses_counts_outside_the_row(native):
    """counts[q] outside [0, C] names the query; decided on the host arrays, before the handle is looked at"""
    lib = native.load_library()
    fn = lib.ivfadc_score_ids
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    q = np.zeros(3 * 8, np.float32)
    ids = np.arange(12, dtype=np.uint32)
    out = np.zeros(12, np.float32)
    qp, ip, op = C.c_void_p(q.ctypes.data), C.c_void_p(ids.ctypes.data), C.c_void_p(out.ctypes.data)
    fake = C.c_void_p(0x10)
    for counts, query in (([4, 5, 0], 1), ([0, 4, -1], 2), ([-7, 9, 9], 0)):
        c = np.array(counts, np.int32)
        for stride in (4, 0):
            assert fn(fake, 3, qp, 4, stride, ip, C.c_void_p(c.ctypes.data), op, None) == INVALID
            msg = lib.ivfadc_last_error()
            assert b"query %d" % query in msg and b"counts = %d" % counts[query] in msg and b"[0, 4]" in msg, msg


def test_python_surface(native):
    import ivfadc_jl_amd as pkg
    for name in ("score_raw", "score_device"):
        assert callable(getattr(native.IVFADCIndex, name, None)), name
    for name in ("score", "knn_among"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__


def test_knn_among_orders_by_distance_then_row_position_and_drops_absent_ids():
    """the host-side convenience on a handle whose score_raw is replaced (no GPU)"""
    import ivfadc_jl_amd as pkg

    class Fake:
        d = 3
        index_type = np.uint32

        def score_raw(self, queries, ids, counts=None):
            ids = np.asarray(ids, np.uint32)
            rows = np.broadcast_to(ids, (len(queries), ids.shape[-1]))
            found = rows < 100
            dists = np.where(found, (rows % 4).astype(np.float32), np.float32(np.inf)).astype(np.float32)
            return dists, found

    ids = np.array([7, 400, 4, 8, 5, 0xFFFFFFFF, 12, 3], np.uint32)                # distances 3 inf 0 0 1 inf 0 3
    got_i, got_d = pkg.knn_among(Fake(), np.zeros(3, np.float32), ids, 5)
    assert got_i.tolist() == [4, 8, 12, 5, 7] and got_d.tolist() == [0.0, 0.0, 0.0, 1.0, 3.0] and got_d.dtype == np.float32
    got_i, got_d = pkg.knn_among(Fake(), np.zeros((2, 3), np.float32), np.stack([ids, ids[::-1]]), 100)
    assert got_i[0].tolist() == [4, 8, 12, 5, 7, 3] and got_i[1].tolist() == [12, 8, 4, 5, 3, 7], "absent ids are dropped"
    assert pkg.score(Fake(), np.zeros(3, np.float32), ids).shape == (8,) and pkg.score(Fake(), np.zeros((2, 3), np.float32), ids).shape == (2, 8)
    with pytest.raises(AssertionError):
        pkg.knn_among(Fake(), np.zeros(3, np.float32), ids, 0)
