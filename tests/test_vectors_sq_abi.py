"""CPU checks of the boundary of the 8-bit scalar-quantised vector store: the new symbols exported and bound, and every refusal that is
decided on the arguments alone returned as IVFADC_ERR_INVALID with its message, without a device.  (The range refusals that read d need a
handle: tests/test_gpu_vectors_sq.py.)"""
import ctypes as C

import numpy as np
import pytest

INVALID, VP = 2, C.c_void_p
FAKE = VP(0x10)                                   # never dereferenced: every call below is decided before the objects are read
P, OUT = VP(np.zeros(64, np.float32).ctypes.data), VP(5)
SQ, PLAIN = [VP, C.c_int64, VP, VP, VP, VP], [VP, C.c_int64, VP, C.c_int, VP]
CASES = [(e, SQ, a, w) for e in ("ivfadc_vectors_create_sq", "ivfadc_vectors_create_sq_device") for a, w in (
    ((FAKE, 2, P, None, None, None), b"null out"), ((None, 2, P, None, None, C.byref(OUT)), b"null handle"),
    ((FAKE, -1, P, None, None, C.byref(OUT)), b"n = -1"), ((FAKE, (1 << 32) + 1, P, None, None, C.byref(OUT)), b"2^32"),
    ((FAKE, 2, None, P, P, C.byref(OUT)), b"null data"), ((FAKE, 2, P, P, None, C.byref(OUT)), b"only one of lo and hi"),
    ((FAKE, 2, P, None, P, C.byref(OUT)), b"only one of lo and hi"))]
# store_type 3 is no longer refused for its number: the call goes on to the next check; 2 and 4 still are
CASES += [(e, PLAIN, a, w) for e in ("ivfadc_vectors_create", "ivfadc_vectors_create_device") for a, w in (
    ((FAKE, 2, None, 3, C.byref(OUT)), b"null data"), ((FAKE, 2, P, 4, C.byref(OUT)), b"store_type = 4"), ((FAKE, 2, P, 2, C.byref(OUT)), b"store_type = 2"))]


@pytest.mark.parametrize("entry,argtypes,args,word", CASES)
def test_argument_errors_need_no_device(native, entry, argtypes, args, word):
    lib = native.load_library()
    fn = getattr(lib, entry)
    fn.argtypes = argtypes
    OUT.value = 5                                     # (a refused call must put NULL here again)
    assert fn(*args) == INVALID
    assert word in lib.ivfadc_last_error() and entry.split("_device")[0].encode() in lib.ivfadc_last_error()
    assert args[-1] is None or OUT.value is None, "a refused call hands out no store"


def test_read_back_symbol_and_python_surface(native):
    lib = native.load_library()
    lib.ivfadc_vectors_get_sq.argtypes = [VP] * 5
    assert lib.ivfadc_vectors_get_sq(None, None, None, None, None) == INVALID and b"null store" in lib.ivfadc_last_error()
    assert all(callable(getattr(native.IVFADCIndex, name)) for name in ("vectors_sq", "vectors_sq_device"))
    assert callable(native.VectorStore.sq_arrays) and "vectors_sq" not in native.__all__
