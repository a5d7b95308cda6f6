"""Every refusal of ivfadc_vectors_create_pq that is decided on the arguments alone, by status and by its word in ivfadc_last_error(),
without a device.  (The refusals that read the handle or the data: tests/test_gpu_vectors_pq.py.)"""
import ctypes as C

import numpy as np
import pytest

INVALID, VP = 2, C.c_void_p
FAKE = VP(0x10)                                   # never dereferenced: every call below is decided before the handle is read
P, OUT = VP(np.zeros(64, np.float32).ctypes.data), VP(5)
CREATE = [VP, C.c_int64, VP, C.c_int, C.c_int, VP, C.c_int, C.c_uint64, C.c_int64, VP]
CASES = [(e, a, w) for e in ("ivfadc_vectors_create_pq", "ivfadc_vectors_create_pq_device") for a, w in (
    ((FAKE, 2, P, 8, 256, None, 25, 0, 0, None), b"null out"), ((None, 2, P, 8, 256, None, 25, 0, 0, C.byref(OUT)), b"null handle"),
    ((FAKE, -1, P, 8, 256, None, 25, 0, 0, C.byref(OUT)), b"n = -1"), ((FAKE, (1 << 32) + 1, P, 8, 256, None, 25, 0, 0, C.byref(OUT)), b"2^32"),
    ((FAKE, 2, None, 8, 256, None, 25, 0, 0, C.byref(OUT)), b"null data"), ((FAKE, 2, P, 0, 256, None, 25, 0, 0, C.byref(OUT)), b"m2 = 0"),
    ((FAKE, 2, P, 8, 0, None, 25, 0, 0, C.byref(OUT)), b"k2 = 0 outside 1..256"), ((FAKE, 2, P, 8, 257, P, 25, 0, 0, C.byref(OUT)), b"k2 = 257"),
    ((FAKE, 2, P, 8, 256, None, 0, 0, 0, C.byref(OUT)), b"maxiter = 0"))]


@pytest.mark.parametrize("entry,args,word", CASES)
def test_argument_errors_need_no_device(native, entry, args, word):
    lib = native.load_library()
    fn = getattr(lib, entry)
    fn.argtypes = CREATE
    OUT.value = 5                                     # (a refused call must put NULL here again)
    assert fn(*args) == INVALID
    assert word in lib.ivfadc_last_error() and b"ivfadc_vectors_create_pq" in lib.ivfadc_last_error()
    assert args[9] is None or OUT.value is None, "a refused call hands out no store"
