"""CPU checks of the masked range search's boundary: the two symbols declared and exported, the header block behind the result typedef,
every argument error returned before the handle is looked at or the device is touched (in the plain entries' order, with the stray
mask_of_query among them), the ABI version, and the Python surface with its assertion texts."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "ivfadc_range_search_masked": ("int", ["ivfadc_t *", "const ivfadc_maskset_t *", "int64_t", "const float *", "const float *", "int", "int64_t",
                                           "const int32_t *", "ivfadc_range_result_t **"]),
    "ivfadc_range_search_device_masked": ("int", ["ivfadc_t *", "const ivfadc_maskset_t *", "int64_t", "const float *", "const float *", "int",
                                                  "int64_t", "const int32_t *", "ivfadc_range_result_t **"]),
}


def _header():
    return open(os.path.join(ROOT, "include", "ivfadc_hip.h")).read()


def test_the_two_entries_are_declared_and_exported(native):
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    lib = native.load_library()
    for s, (ret, want) in PROTOS.items():
        m = re.search(r"\b(int|void)\s+%s\s*\(([^()]*)\)\s*;" % s, code)
        assert m, "%s is not declared in include/ivfadc_hip.h" % s
        args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(2).split(",")]
        assert m.group(1) == ret and [re.sub(r"\b\w+$", "", a).strip() for a in args] == want, (s, args)
        assert hasattr(lib, s), "libivfadc_hip.so does not export %s" % s
        assert code.index(s) > code.index("typedef struct ivfadc_range_result"), "declared behind the result type"
    # the plain entries are as they were
    assert re.search(r"int\s+ivfadc_range_search\s*\(\s*ivfadc_t \*h, int64_t nq, const float \*queries, const float \*radii, int w, int64_t max_total,", code)


def test_the_change_is_additive():
    hdr = _header()
    ver = int(re.search(r"#define\s+IVFADC_ABI_VERSION\s+(\d+)", hdr).group(1))
    from ivfadc_jl_amd import _native as nat
    jl = open(os.path.join(ROOT, "julia", "IVFADCHip.jl")).read()
    assert nat.ABI_VERSION == ver == 4 == int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1))
    assert "range_search_masked" not in jl, "the Julia shim does not carry the entries"
    stats = hdr[hdr.index("typedef struct {", hdr.index("scan_ms") - 200):hdr.index("} ivfadc_stats;")]
    assert "range" not in stats, "ivfadc_stats is as it was"


def test_header_block_states_the_contract():
    hdr = _header()
    start = hdr.index("MASKED range search")
    assert start > hdr.index("typedef struct ivfadc_range_result")
    block = re.sub(r"\s*\n \* ", " ", hdr[start:hdr.index("int ivfadc_range_search_masked")])      # (the comment's line breaks aside)
    for needle in ("NO REFERENCE COUNTERPART", "ivfadc_search_masked", "UNFILTERED", "ORIGINAL visit numbers", "-1", "mask 0 for every query",
                   "s == NULL", "UInt16", "codebook", "ivfadc_clone_view", "push!", "IVFADC_ERR_STATE", "subset view", "another index",
                   "changed since", "list partition", "stale view", "IVFADC_ERR_INVALID", "IVFADC_ERR_ASSERT", "NULL out", "max_total < 0",
                   "nq < 0", "NULL radii", "NaN", "NULL h", "clamps", "scanned_points", "selected or not", "1024", "Not covered", "ivfadc_mg_"):
        assert needle in block, needle
    plain = hdr[hdr.index("RANGE search"):hdr.index("typedef struct ivfadc_range_result")]
    assert "ivfadc_range_search_masked" in plain, "the plain block points at the new entries"


def test_argument_validation_needs_no_gpu(native):
    """each error decided before the handle is looked at or the device is touched, in the plain entries' order, *out cleared"""
    lib = native.load_library()
    q = np.zeros(8, np.float32)
    r = np.ones(2, np.float32)
    nan = np.array([1.0, np.nan], np.float32)
    moq = np.zeros(2, np.int32)
    qp, rp, np_, mp = (C.c_void_p(a.ctypes.data) for a in (q, r, nan, moq))
    for entry in PROTOS:
        fn = getattr(lib, entry)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p)]
        out = C.c_void_p(0x1234)
        assert fn(None, None, 2, qp, rp, 1, 0, None, None) == 2 and b"null out" in lib.ivfadc_last_error()
        assert fn(None, None, 2, qp, rp, 1, -1, None, C.byref(out)) == 2 and b"max_total" in lib.ivfadc_last_error()
        assert out.value is None, "out is cleared on failure"
        out = C.c_void_p(0x1234)
        assert fn(None, None, 2, qp, rp, 0, 0, None, C.byref(out)) == 1
        assert lib.ivfadc_last_error() == b"Number of clusters to search in must be w >= 1"
        assert out.value is None
        assert fn(None, None, -1, qp, rp, 1, 0, None, C.byref(out)) == 2 and b"nq < 0" in lib.ivfadc_last_error()
        assert fn(None, None, 2, qp, None, 1, 0, None, C.byref(out)) == 2 and b"null radii" in lib.ivfadc_last_error()
        assert fn(None, None, 2, None, rp, 1, 0, None, C.byref(out)) == 2 and b"null queries" in lib.ivfadc_last_error()
        # the order: max_total before nq, nq before radii, radii before queries
        assert fn(None, None, -1, None, None, 1, -1, None, C.byref(out)) == 2 and b"max_total" in lib.ivfadc_last_error()
        assert fn(None, None, -1, None, None, 1, 0, None, C.byref(out)) == 2 and b"nq < 0" in lib.ivfadc_last_error()
        assert fn(None, None, 2, None, None, 1, 0, None, C.byref(out)) == 2 and b"null radii" in lib.ivfadc_last_error()
        # a null set with mask numbers: refused, before the handle is looked at
        assert fn(None, None, 2, qp, rp, 1, 0, mp, C.byref(out)) == 2 and b"mask_of_query without a mask set" in lib.ivfadc_last_error()
        assert fn(None, None, 2, qp, rp, 1, 0, None, C.byref(out)) == 2 and b"null handle" in lib.ivfadc_last_error()
        assert out.value is None
    fn = lib.ivfadc_range_search_masked
    out = C.c_void_p()
    assert fn(None, None, 2, qp, np_, 1, 0, None, C.byref(out)) == 2 and b"query 1 is NaN" in lib.ivfadc_last_error()
    assert fn(None, None, 2, qp, np_, 1, 0, mp, C.byref(out)) == 2 and b"query 1 is NaN" in lib.ivfadc_last_error()   # (the NaN comes first)
    assert fn(None, None, 1, qp, np_, 1, 0, None, C.byref(out)) == 2 and b"null handle" in lib.ivfadc_last_error()     # (the NaN is behind nq)
    fn = lib.ivfadc_range_search_device_masked                  # the device entry cannot read its radii
    assert fn(None, None, 2, qp, np_, 1, 0, None, C.byref(out)) == 2 and b"null handle" in lib.ivfadc_last_error()


def test_python_surface(native):
    import ivfadc_jl_amd as pkg
    for name in ("range_search_masked_raw", "range_search_device_masked"):
        assert callable(getattr(native.IVFADCIndex, name, None)), name
    assert callable(pkg.range_search_masked) and "range_search_masked" in pkg.__all__
    fake = native.IVFADCIndex.__new__(native.IVFADCIndex)          # the argument checks come before the handle is touched
    fake.d = 4
    with pytest.raises(AssertionError, match="w >= 1"):
        pkg.range_search_masked(fake, np.zeros(4, np.float32), 1.0, w=0)
    with pytest.raises(AssertionError, match="queries must be"):
        pkg.range_search_masked(fake, np.zeros(5, np.float32), 1.0)
    with pytest.raises(AssertionError, match="NaN"):
        pkg.range_search_masked(fake, np.zeros(4, np.float32), np.nan)
    with pytest.raises(AssertionError, match="needs a maskset"):
        pkg.range_search_masked(fake, np.zeros(4, np.float32), 1.0, mask_of_query=0)
    with pytest.raises(AssertionError, match="one radius per query"):
        fake.range_search_masked_raw(np.zeros((2, 4), np.float32), np.ones(3, np.float32))
    with pytest.raises(AssertionError, match="queries must be"):
        fake.range_search_masked_raw(np.zeros((2, 5), np.float32), np.ones(2, np.float32))
    with pytest.raises(AssertionError, match=r"mask_of_query must be \(nq,\)"):
        fake.range_search_masked_raw(np.zeros((2, 4), np.float32), np.ones(2, np.float32), None, np.zeros(3, np.int32))
