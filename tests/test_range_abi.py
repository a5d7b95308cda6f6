"""CPU checks of the range search's boundary: the six symbols declared and exported, the header comment's contract, every argument error
returned before the handle is looked at or the device is touched, and the Python surface with the reference's assertion texts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "ivfadc_range_search": ("int", ["ivfadc_t *", "int64_t", "const float *", "const float *", "int", "int64_t", "ivfadc_range_result_t **"]),
    "ivfadc_range_search_device": ("int", ["ivfadc_t *", "int64_t", "const float *", "const float *", "int", "int64_t", "ivfadc_range_result_t **"]),
    "ivfadc_range_result_sizes": ("int", ["const ivfadc_range_result_t *", "int64_t *", "int64_t *"]),
    "ivfadc_range_result_copy": ("int", ["const ivfadc_range_result_t *", "int64_t *", "uint32_t *", "float *"]),
    "ivfadc_range_result_device": ("int", ["const ivfadc_range_result_t *", "const int64_t **", "const uint32_t **", "const float **"]),
    "ivfadc_range_result_destroy": ("void", ["ivfadc_range_result_t *"]),
}


def _header():
    return open(os.path.join(ROOT, "include", "ivfadc_hip.h")).read()


def test_the_six_entries_are_declared_and_exported(native):
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+ivfadc_range_result\s+ivfadc_range_result_t\s*;", code)
    lib = native.load_library()
    for s, (ret, want) in PROTOS.items():
        m = re.search(r"\b(int|void)\s+%s\s*\(([^()]*)\)\s*;" % s, code)
        assert m, "%s is not declared in include/ivfadc_hip.h" % s
        args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(2).split(",")]
        assert m.group(1) == ret and [re.sub(r"\b\w+$", "", a).strip() for a in args] == want, (s, args)
        assert hasattr(lib, s), "libivfadc_hip.so does not export %s" % s


def test_the_change_is_additive():
    """no prototype changed in place and no struct grew: by the header's own rule the ABI version stays, in all three places"""
    hdr = _header()
    ver = int(re.search(r"#define\s+IVFADC_ABI_VERSION\s+(\d+)", hdr).group(1))
    from ivfadc_jl_amd import _native as nat
    jl = open(os.path.join(ROOT, "julia", "IVFADCHip.jl")).read()
    assert nat.ABI_VERSION == ver == int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1))
    stats = hdr[hdr.index("typedef struct {", hdr.index("scan_ms") - 200):hdr.index("} ivfadc_stats;")]
    assert "range" not in stats, "ivfadc_stats is as it was"


def test_header_comment_states_the_contract():
    hdr = _header()
    block = hdr[hdr.index("RANGE search"):hdr.index("typedef struct ivfadc_range_result")]
    for needle in ("NO REFERENCE COUNTERPART", "index.jl:204-258", "index.jl:211", "d <= r", "INCLUSIVE", "SQUARED", "r < 0", "+inf", "NaN",
                   "precondition", "one radius per query", "lims", "BLOCKING", "SAFE", "max_total", "before anything of the result is allocated",
                   "IVFADC_ERR_INVALID", "IVFADC_ERR_ASSERT", "IVFADC_ERR_STATE", "UInt16", "ivfadc_clone_view", "subset views", ":opq",
                   "ivfadc_set_workspace_limit", "ivfadc_set_stream", "scanned_points", "chunk_points", "2^32", "Not covered", "mask sets",
                   "list-partitioned", "ivfadc_mg_"):
        assert needle in block, needle


def test_argument_validation_needs_no_gpu(native):
    """each error decided before the handle is looked at or the device is touched, each named in the message, *out cleared"""
    lib = native.load_library()
    q = np.zeros(8, np.float32)
    r = np.ones(2, np.float32)
    nan = np.array([1.0, np.nan], np.float32)
    qp, rp, np_ = C.c_void_p(q.ctypes.data), C.c_void_p(r.ctypes.data), C.c_void_p(nan.ctypes.data)
    for entry in ("ivfadc_range_search", "ivfadc_range_search_device"):
        fn = getattr(lib, entry)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_void_p)]
        out = C.c_void_p(0x1234)
        assert fn(None, 2, qp, rp, 1, 0, None) == 2 and b"null out" in lib.ivfadc_last_error()
        assert fn(None, 2, qp, rp, 1, -1, C.byref(out)) == 2 and b"max_total" in lib.ivfadc_last_error()
        assert out.value is None, "out is cleared on failure"
        out = C.c_void_p(0x1234)
        assert fn(None, 2, qp, rp, 0, 0, C.byref(out)) == 1 and lib.ivfadc_last_error() == b"Number of clusters to search in must be w >= 1"
        assert fn(None, 2, qp, rp, -3, 0, C.byref(out)) == 1
        assert fn(None, -1, qp, rp, 1, 0, C.byref(out)) == 2 and b"nq < 0" in lib.ivfadc_last_error()
        assert fn(None, 2, qp, None, 1, 0, C.byref(out)) == 2 and b"null radii" in lib.ivfadc_last_error()
        assert fn(None, 2, None, rp, 1, 0, C.byref(out)) == 2 and b"null queries" in lib.ivfadc_last_error()
        assert fn(None, 2, qp, rp, 1, 0, C.byref(out)) == 2 and b"null handle" in lib.ivfadc_last_error()
        assert fn(None, 2, qp, rp, 1, 5, C.byref(out)) == 2 and b"null handle" in lib.ivfadc_last_error()
        assert out.value is None
    # a NaN radius: the host entry reads its radii before anything else and names the query; the device entry cannot (a precondition)
    fn = lib.ivfadc_range_search
    out = C.c_void_p()
    assert fn(None, 2, qp, np_, 1, 0, C.byref(out)) == 2 and b"query 1 is NaN" in lib.ivfadc_last_error()
    assert fn(None, 1, qp, np_, 1, 0, C.byref(out)) == 2 and b"null handle" in lib.ivfadc_last_error()      # (the NaN is behind nq)
    # the result entries
    for name, nargs in (("ivfadc_range_result_sizes", 3), ("ivfadc_range_result_copy", 4), ("ivfadc_range_result_device", 4)):
        f = getattr(lib, name)
        f.restype = C.c_int
        f.argtypes = [C.c_void_p] * nargs
        assert f(*([None] * nargs)) == 2 and b"null result" in lib.ivfadc_last_error()
    lib.ivfadc_range_result_destroy.restype = None
    lib.ivfadc_range_result_destroy.argtypes = [C.c_void_p]
    lib.ivfadc_range_result_destroy(None)                        # a no-op, as free(NULL)


def test_python_surface(native):
    import ivfadc_jl_amd as pkg
    from ivfadc_jl_amd import index as ix
    for name in ("range_search_raw", "range_search_device"):
        assert callable(getattr(native.IVFADCIndex, name, None)), name
    for name in ("range_result_sizes", "range_result_copy", "range_result_device", "range_result_destroy"):
        assert callable(getattr(ix, name, None)), name
    assert callable(pkg.range_search) and "range_search" in pkg.__all__
    fake = native.IVFADCIndex.__new__(native.IVFADCIndex)          # the argument checks come before the handle is touched
    fake.d = 4
    with pytest.raises(AssertionError, match="w >= 1"):
        pkg.range_search(fake, np.zeros(4, np.float32), 1.0, w=0)
    with pytest.raises(AssertionError, match="queries must be"):
        pkg.range_search(fake, np.zeros(5, np.float32), 1.0)
    with pytest.raises(AssertionError, match="NaN"):
        pkg.range_search(fake, np.zeros(4, np.float32), np.nan)
    with pytest.raises(AssertionError, match="one radius per query"):
        fake.range_search_raw(np.zeros((2, 4), np.float32), np.ones(3, np.float32))
    with pytest.raises(AssertionError, match="queries must be"):
        fake.range_search_raw(np.zeros((2, 5), np.float32), np.ones(2, np.float32))
