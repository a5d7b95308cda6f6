"""CPU checks of the masked-search entries' boundary: the five symbols declared and exported, the ABI version unchanged (the change is
additive), the header comment's contract, the argument validation that needs no device, and the Python surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "ivfadc_maskset_create": ("int", ["ivfadc_t *", "int", "const uint32_t *", "uint64_t", "ivfadc_maskset_t **", "int64_t *"]),
    "ivfadc_maskset_create_device": ("int", ["ivfadc_t *", "int", "const uint32_t *", "uint64_t", "ivfadc_maskset_t **", "int64_t *"]),
    "ivfadc_maskset_destroy": ("void", ["ivfadc_maskset_t *"]),
    "ivfadc_search_masked": ("int", ["ivfadc_t *", "const ivfadc_maskset_t *", "int64_t", "const float *", "int", "int", "const int32_t *",
                                     "uint32_t *", "float *", "int32_t *"]),
    "ivfadc_search_device_masked": ("int", ["ivfadc_t *", "const ivfadc_maskset_t *", "int64_t", "const float *", "int", "int", "const int32_t *",
                                            "uint32_t *", "float *", "int32_t *"]),
}


def _header():
    return open(os.path.join(ROOT, "include", "ivfadc_hip.h")).read()


def test_the_five_entries_are_declared_and_exported(native):
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+ivfadc_maskset\s+ivfadc_maskset_t\s*;", code)
    lib = native.load_library()
    for s, (ret, want) in PROTOS.items():
        m = re.search(r"\b(int|void)\s+%s\s*\(([^()]*)\)\s*;" % s, code)
        assert m, "%s is not declared in include/ivfadc_hip.h" % s
        args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(2).split(",")]
        assert m.group(1) == ret and [re.sub(r"\b\w+$", "", a).strip() for a in args] == want, (s, args)
        assert hasattr(lib, s), "libivfadc_hip.so does not export %s" % s


def test_abi_version_is_still_4(native):
    assert int(re.search(r"#define\s+IVFADC_ABI_VERSION\s+(\d+)", _header()).group(1)) == 4
    from ivfadc_jl_amd import _native as nat
    assert nat.ABI_VERSION == 4
    jl = open(os.path.join(ROOT, "julia", "IVFADCHip.jl")).read()
    assert int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1)) == 4
    assert native.load_library().ivfadc_abi_version() == 4


def test_header_comment_states_the_contract():
    hdr = _header()
    block = hdr[hdr.index("PER-QUERY filtered search"):hdr.index("typedef struct ivfadc_maskset")]
    for needle in ("index.jl:204-258", "utils.jl:98-99", "_shift_inverse_index!", "the -1 rule", "the view rule", "ivfadc_clone_view", "i < nbits",
                   "(i & 31)", "[-1, nmasks)", "clamps", "IVFADC_ERR_STATE", "IVFADC_ERR_INVALID", "IVFADC_ERR_ASSERT", "before any device call",
                   "stats.last_striped == 8", "Not covered", "immutable", "ivfadc_set_workspace_limit"):
        assert needle in block, needle
    stats = hdr[hdr.index("int32_t  last_striped;"):hdr.index("int32_t  coarse_listed;")]
    assert "8 = the masked scan" in stats
    subset_block = hdr[hdr.index("A SUBSET view"):hdr.index("int ivfadc_clone_subset(")]
    assert "ivfadc_search_masked" in subset_block, "the subset comment points at the per-query entry instead of calling it uncovered"


def test_argument_validation_needs_no_gpu(native):
    """IVFADC_ERR_INVALID (2), each named in the message, each decided before the handle is looked at or the device is touched"""
    lib = native.load_library()
    words = np.zeros(8, np.uint32)
    bits = C.c_void_p(words.ctypes.data)
    for entry in ("ivfadc_maskset_create", "ivfadc_maskset_create_device"):
        fn = getattr(lib, entry)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        out = C.c_void_p(0x1234)
        kept = (C.c_int64 * 2)(-7, -7)
        assert fn(None, 2, bits, 128, None, kept) == 2 and b"null out" in lib.ivfadc_last_error()
        assert fn(None, 0, bits, 128, C.byref(out), kept) == 2 and b"nmasks" in lib.ivfadc_last_error()
        assert out.value is None, "out is cleared on failure"
        assert fn(None, -3, bits, 128, C.byref(out), kept) == 2 and b"nmasks" in lib.ivfadc_last_error()
        assert fn(None, 2, bits, 2 ** 32 + 1, C.byref(out), kept) == 2 and b"2^32" in lib.ivfadc_last_error()
        assert fn(None, 2, None, 1, C.byref(out), kept) == 2 and b"null bitmap" in lib.ivfadc_last_error()
        assert fn(None, 2, bits, 128, C.byref(out), kept) == 2 and b"null handle" in lib.ivfadc_last_error()
        assert fn(None, 1, None, 0, C.byref(out), None) == 2 and b"null handle" in lib.ivfadc_last_error()      # (nbits == 0 needs no bitmap)
        assert fn(None, 1, bits, 2 ** 32, C.byref(out), None) == 2 and b"null handle" in lib.ivfadc_last_error()  # (2^32 itself is allowed)
        assert kept[0] == -7 and kept[1] == -7 and out.value is None
    q = np.zeros(4, np.float32)
    for entry in ("ivfadc_search_masked", "ivfadc_search_device_masked"):
        fn = getattr(lib, entry)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        assert fn(None, None, 1, C.c_void_p(q.ctypes.data), 1, 1, None, None, None, None) == 2 and b"null handle" in lib.ivfadc_last_error()
    lib.ivfadc_maskset_destroy.restype = None
    lib.ivfadc_maskset_destroy.argtypes = [C.c_void_p]
    lib.ivfadc_maskset_destroy(None)                        # a no-op, as free(NULL)


def test_python_surface(native):
    import ivfadc_jl_amd as pkg
    from ivfadc_jl_amd import index as ix
    for name in ("maskset", "maskset_device", "search_masked_raw", "search_device_masked"):
        assert callable(getattr(native.IVFADCIndex, name, None)), name
    assert callable(pkg.knn_search_masked) and "knn_search_masked" in pkg.__all__ and pkg.MaskSet is ix.MaskSet
    assert isinstance(ix.MaskSet.kept, property) and hasattr(ix.MaskSet, "__len__") and hasattr(ix.MaskSet, "__del__")
    fake = native.IVFADCIndex.__new__(native.IVFADCIndex)          # the argument checks come before the handle is touched
    with pytest.raises(AssertionError, match="exactly one"):
        fake.maskset(masks=[np.ones(2, bool)], ids=[[1]])
    with pytest.raises(AssertionError, match="exactly one"):
        fake.maskset()
    with pytest.raises(AssertionError, match="at least one"):
        fake.maskset(masks=[])
    with pytest.raises(AssertionError):
        fake.maskset(masks=[np.ones(3, np.int32)])
    with pytest.raises(AssertionError):
        fake.maskset(ids=[[-1]])
    fake.d = 4
    with pytest.raises(AssertionError, match="k >= 1"):
        pkg.knn_search_masked(fake, np.zeros(4, np.float32), 0, None)
    with pytest.raises(AssertionError, match="w >= 1"):
        pkg.knn_search_masked(fake, np.zeros(4, np.float32), 1, None, w=0)
