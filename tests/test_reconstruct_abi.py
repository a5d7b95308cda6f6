"""CPU checks of the boundary of locate / reconstruct: the four symbols declared and exported, the change additive (ABI version unchanged
in header, binding and shim), every argument error returned before the handle is looked at or the device is touched, the header comment's
contract, and the Python and Julia surfaces."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "ivfadc_locate": ["ivfadc_t *", "int64_t", "const uint32_t *", "int32_t *", "int64_t *"],
    "ivfadc_reconstruct": ["ivfadc_t *", "int64_t", "const uint32_t *", "float *", "uint8_t *"],
    "ivfadc_locate_device": ["ivfadc_t *", "int64_t", "const uint32_t *", "int32_t *", "int64_t *"],
    "ivfadc_reconstruct_device": ["ivfadc_t *", "int64_t", "const uint32_t *", "float *", "uint8_t *"],
}


def _header():
    return open(os.path.join(ROOT, "include", "ivfadc_hip.h")).read()


def test_the_four_entries_are_declared_and_exported(native):
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    lib = native.load_library()
    for s, want in PROTOS.items():
        m = re.search(r"\bint\s+%s\s*\(([^()]*)\)\s*;" % s, code)
        assert m, "%s is not declared in include/ivfadc_hip.h" % s
        args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        assert [re.sub(r"\b\w+$", "", a).strip() for a in args] == want, (s, args)
        assert hasattr(lib, s), "libivfadc_hip.so does not export %s" % s


def test_the_change_is_additive():
    """no prototype changed in place and no struct grew: by the header's own rule the ABI version stays, in all three places"""
    hdr = _header()
    ver = int(re.search(r"#define\s+IVFADC_ABI_VERSION\s+(\d+)", hdr).group(1))
    from ivfadc_jl_amd import _native as nat
    jl = open(os.path.join(ROOT, "julia", "IVFADCHip.jl")).read()
    assert nat.ABI_VERSION == ver == int(re.search(r"const ABI_VERSION = (\d+)", jl).group(1)) == 4
    stats = hdr[hdr.index("typedef struct {", hdr.index("scan_ms") - 200):hdr.index("} ivfadc_stats;")]
    assert "locate" not in stats and "reconstruct" not in stats, "ivfadc_stats is as it was"


def test_header_comment_states_the_contract():
    hdr = _header()
    block = hdr[hdr.index("LOCATE and RECONSTRUCT"):hdr.index("int ivfadc_reconstruct_device(")]
    for needle in ("utils.jl:49-55", "utils.jl:58-59", "71-81", "list_len", "stale rows", "LAST list", "does not break", "FIRST position",
                   "findfirst", "unique", "ONE IEEE Float32 addition", "bit-identical", "subnormal", "signed-zero", "large-magnitude",
                   "rotation", ":opq", "NOT applied", "out_list = -1", "out_pos = -1", "found = 0", "+0.0", "Not an error", "slot by slot",
                   "request order", "0xFFFFFFFF", "unsigned 32-bit", "out_found", "may be NULL", "UInt16", "ivfadc_clone_view", "subset views",
                   "dropped", "device-synthesised", "push!", "laid out first", "IVFADC_ERR_STATE", "block", "ivfadc_search_device",
                   "asynchronous", "IVFADC_ERR_INVALID", "before the handle is looked at", "null", "n < 0", "n == 0", "Not covered",
                   "ivfadc_mg_", "list-partitioned"):
        assert needle in block, needle


def test_argument_validation_needs_no_gpu(native):
    """each error decided before the handle is looked at or the device is touched, each named in ivfadc_last_error()"""
    lib = native.load_library()
    ids = np.arange(4, dtype=np.uint32)
    buf = np.zeros(64, np.int64)
    ip, bp = C.c_void_p(ids.ctypes.data), C.c_void_p(buf.ctypes.data)
    fake = C.c_void_p(0x10)                      # never dereferenced: every call below fails on an argument first
    for entry in ("ivfadc_locate", "ivfadc_locate_device"):
        fn = getattr(lib, entry)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        assert fn(None, 4, ip, bp, bp) == 2 and b"null handle" in lib.ivfadc_last_error() and entry.encode() in lib.ivfadc_last_error()
        assert fn(None, 0, ip, bp, bp) == 2 and b"null handle" in lib.ivfadc_last_error()
        assert fn(fake, -1, ip, bp, bp) == 2 and b"n = -1" in lib.ivfadc_last_error()
        assert fn(fake, 4, None, bp, bp) == 2 and b"null ids" in lib.ivfadc_last_error()
        assert fn(fake, 4, ip, None, bp) == 2 and b"null out_list" in lib.ivfadc_last_error()
        assert fn(fake, 4, ip, bp, None) == 2 and b"null out_pos" in lib.ivfadc_last_error()
        assert fn(fake, 0, None, None, bp) == 2 and b"null out_list" in lib.ivfadc_last_error()       # (outputs are checked at n == 0 too)
    for entry in ("ivfadc_reconstruct", "ivfadc_reconstruct_device"):
        fn = getattr(lib, entry)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        assert fn(None, 4, ip, bp, None) == 2 and b"null handle" in lib.ivfadc_last_error() and entry.encode() in lib.ivfadc_last_error()
        assert fn(fake, -5, ip, bp, None) == 2 and b"n = -5" in lib.ivfadc_last_error()
        assert fn(fake, 4, None, bp, None) == 2 and b"null ids" in lib.ivfadc_last_error()
        assert fn(fake, 4, ip, None, bp) == 2 and b"null out_vectors" in lib.ivfadc_last_error()


def test_python_and_julia_surfaces(native):
    import ivfadc_jl_amd as pkg
    from ivfadc_jl_amd import index as ix
    for name in ("locate_raw", "reconstruct_raw", "locate_device", "reconstruct_device"):
        assert callable(getattr(native.IVFADCIndex, name, None)), name
    for name in ("locate", "reconstruct"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__
    import inspect
    src = inspect.getsource(ix._pop)
    assert "_lists()" not in src and "reconstruct(" in src and "_delete_ids(" in src, "_pop is reconstruct, then delete: no host mirror"
    jl = open(os.path.join(ROOT, "julia", "IVFADCHip.jl")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for text in (jl, doc):
        assert "ccall((:ivfadc_locate, LIBIVFADC)" in text and "ccall((:ivfadc_reconstruct, LIBIVFADC)" in text
        assert "hip_locate" in text and "hip_reconstruct" in text
    for name in ("ivfadc_locate_device", "ivfadc_reconstruct_device"):
        assert name in doc, name


def test_reconstruct_raises_for_an_absent_id():
    """the Python entry names the first missing id (no GPU: the handle's method is replaced)"""
    import ivfadc_jl_amd as pkg

    class Fake:
        d = 3

        def reconstruct_raw(self, ids):
            return np.zeros((len(ids), 3), np.float32), np.array([True, False, True, False])[:len(ids)]

    with pytest.raises(AssertionError, match="id 4000000000 is not stored"):
        pkg.reconstruct(Fake(), np.array([7, 4000000000, 9, 11], np.uint32))
    assert pkg.reconstruct(Fake(), np.array([7], np.uint32)).shape == (1, 3)
