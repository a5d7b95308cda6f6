"""CPU checks of the subset entries' boundary: both symbols declared and exported, the ABI version unchanged (the change is additive),
the argument validation that needs no device, and the Python surface (IVFADCIndex.subset, the bitmap packing)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("ivfadc_clone_subset", "ivfadc_clone_subset_device")


def _header():
    return open(os.path.join(ROOT, "include", "ivfadc_hip.h")).read()


def test_both_symbols_are_declared_and_exported(native):
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    lib = native.load_library()
    for s in SYMS:
        m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % s, code)
        assert m, "%s is not declared in include/ivfadc_hip.h" % s
        args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        assert [re.sub(r"\b\w+$", "", a).strip() for a in args] == ["ivfadc_t *", "const uint32_t *", "uint64_t", "ivfadc_t **", "int64_t *"], args
        assert hasattr(lib, s), "libivfadc_hip.so does not export %s" % s


def test_header_comment_states_the_contract():
    """the comment block is documentation: reference behaviour, bitmap convention, view rules, what is out of scope"""
    hdr = _header()
    block = hdr[hdr.index("A SUBSET view"):hdr.index("int ivfadc_clone_subset(")]
    for needle in ("utils.jl:98-99", "_shift_inverse_index!", "index.jl:204-258", "i < nbits", "bits[i >> 5]", "(i & 31)", "read-only",
                   "IVFADC_ERR_STATE", "IVFADC_ERR_INVALID", "before any device call", "Not covered"):
        assert needle in block, needle


def test_abi_version_is_still_4(native):
    assert int(re.search(r"#define\s+IVFADC_ABI_VERSION\s+(\d+)", _header()).group(1)) == 4
    from ivfadc_jl_amd import _native as nat
    assert nat.ABI_VERSION == 4
    jl = open(os.path.join(ROOT, "julia", "IVFADCHip.jl")).read()
    assert int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1)) == 4
    assert native.load_library().ivfadc_abi_version() == 4


@pytest.mark.parametrize("entry", SYMS)
def test_argument_validation_needs_no_gpu(native, entry):
    """IVFADC_ERR_INVALID (2) for a NULL out_view, nbits > 2^32, NULL bits with nbits > 0 and a NULL handle -- each named in the message,
    each decided before the handle is looked at or the device is touched (there is no handle here to look at)."""
    lib = native.load_library()
    fn = getattr(lib, entry)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    words = np.zeros(4, np.uint32)
    bits = C.c_void_p(words.ctypes.data)
    out = C.c_void_p(0x1234)
    n = C.c_int64(-7)
    assert fn(None, bits, 128, None, C.byref(n)) == 2 and b"null out_view" in lib.ivfadc_last_error()
    assert fn(None, bits, 2 ** 32 + 1, C.byref(out), C.byref(n)) == 2 and b"2^32" in lib.ivfadc_last_error()
    assert out.value is None, "out_view is cleared on failure"
    assert fn(None, None, 1, C.byref(out), C.byref(n)) == 2 and b"null bitmap" in lib.ivfadc_last_error()
    assert fn(None, bits, 128, C.byref(out), C.byref(n)) == 2 and b"null handle" in lib.ivfadc_last_error()
    assert fn(None, None, 0, C.byref(out), None) == 2 and b"null handle" in lib.ivfadc_last_error()       # (nbits == 0 needs no bitmap)
    assert fn(None, bits, 2 ** 32, C.byref(out), None) == 2 and b"null handle" in lib.ivfadc_last_error()  # (2^32 itself is allowed)
    assert n.value == -7 and out.value is None


def test_python_surface(native):
    from ivfadc_jl_amd import index as ix
    assert callable(getattr(native.IVFADCIndex, "subset", None))
    words, nbits = ix.pack_bitmap(ids=[0, 31, 32, 63])
    assert words.dtype == np.uint32 and words.tolist() == [0x80000001, 0x80000001] and nbits == 64
    mask = np.zeros(70, bool)
    mask[[0, 31, 32, 63, 69]] = True
    words, nbits = ix.pack_bitmap(mask=mask)
    assert words.tolist() == [0x80000001, 0x80000001, 1 << 5] and nbits == 70
    words, nbits = ix.pack_bitmap(ids=np.zeros(0, np.int64))
    assert words.shape == (0,) and nbits == 0
    assert ix.pack_bitmap(ids=np.array([5, 5, 2], np.uint32))[0].tolist() == [0b100100]
    fake = native.IVFADCIndex.__new__(native.IVFADCIndex)          # the argument checks come before the handle is touched
    with pytest.raises(AssertionError, match="exactly one"):
        fake.subset(ids=[1], mask=np.ones(2, bool))
    with pytest.raises(AssertionError, match="exactly one"):
        fake.subset()
    with pytest.raises(AssertionError):
        fake.subset(mask=np.ones(3, np.int32))
    with pytest.raises(AssertionError):
        fake.subset(ids=[-1])
