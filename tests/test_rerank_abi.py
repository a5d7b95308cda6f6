"""CPU checks of the boundary of the vector store and the re-rank entries: every new symbol exported and bound, every argument error that
is decided on the arguments alone returned as IVFADC_ERR_INVALID with its message, without a device.  (A store of another d needs a real
store: tests/test_gpu_rerank.py.)"""
import ctypes as C

import numpy as np
import pytest

INVALID = 2
VP = C.c_void_p
FAKE = VP(0x10)                                   # never dereferenced: every call below is decided before the objects are read
BUF = np.zeros(64, np.float32)
P = VP(BUF.ctypes.data)
RERANK = [VP, VP, C.c_int64, VP, C.c_int64, VP, VP, C.c_int, VP, VP, VP]
FUSED = [VP, VP, C.c_int64, VP, C.c_int, C.c_int, C.c_int, VP, VP, VP]
CASES = [(e, RERANK, a, w) for e in ("ivfadc_rerank", "ivfadc_rerank_device") for a, w in (
    ((None, FAKE, 2, P, 4, P, None, 3, P, P, P), b"null handle"), ((FAKE, None, 2, P, 4, P, None, 3, P, P, P), b"null vector store"),
    ((FAKE, FAKE, -1, P, 4, P, None, 3, P, P, P), b"nq = -1"), ((FAKE, FAKE, 2, P, -4, P, None, 3, P, P, P), b"C = -4"),
    ((FAKE, FAKE, 2, P, 4, P, None, 0, P, P, P), b"K = 0"), ((FAKE, FAKE, 1 << 31, P, 1, P, None, 3, P, P, P), b"2^31 - 1"),
    ((FAKE, FAKE, 46341, P, 46341, P, None, 3, P, P, P), b"pairs"), ((FAKE, FAKE, 2, None, 4, P, None, 3, P, P, P), b"null queries"),
    ((FAKE, FAKE, 2, P, 4, None, None, 3, P, P, P), b"null ids"), ((FAKE, FAKE, 2, P, 4, P, None, 3, None, P, P), b"null out_ids"),
    ((FAKE, FAKE, 2, P, 4, P, None, 3, P, None, P), b"null out_dists"), ((FAKE, FAKE, 2, P, 4, P, None, 3, P, P, None), b"null out_counts"))]
CASES += [(e, FUSED, a, w) for e in ("ivfadc_search_refined", "ivfadc_search_device_refined") for a, w in (
    ((None, FAKE, 2, P, 3, 9, 1, P, P, P), b"null handle"), ((FAKE, None, 2, P, 3, 9, 1, P, P, P), b"null vector store"),
    ((FAKE, FAKE, 2, P, 3, 2, 1, P, P, P), b"Kc = 2 < K = 3"), ((FAKE, FAKE, 2, P, 0, 9, 1, P, P, P), b"K = 0"),
    ((FAKE, FAKE, 1 << 31, P, 3, 9, 1, P, P, P), b"2^31 - 1"), ((FAKE, FAKE, 2, None, 3, 9, 1, P, P, P), b"null queries"))]
STORE = [VP, C.c_int64, VP, C.c_int, VP]
OUT = VP(5)
CASES += [(e, STORE, a, w) for e in ("ivfadc_vectors_create", "ivfadc_vectors_create_device") for a, w in (
    ((FAKE, 2, P, 0, None), b"null out"), ((None, 2, P, 0, C.byref(OUT)), b"null handle"), ((FAKE, -1, P, 0, C.byref(OUT)), b"n = -1"),
    ((FAKE, (1 << 32) + 1, P, 0, C.byref(OUT)), b"2^32"), ((FAKE, 2, P, 2, C.byref(OUT)), b"store_type = 2"),
    ((FAKE, 2, None, 1, C.byref(OUT)), b"null data"))]


@pytest.mark.parametrize("entry,argtypes,args,word", CASES)
def test_argument_errors_need_no_device(native, entry, argtypes, args, word):
    lib = native.load_library()
    fn = getattr(lib, entry)
    fn.argtypes = argtypes
    OUT.value = 5                                     # (a store entry must put NULL here again)
    assert fn(*args) == INVALID
    assert word in lib.ivfadc_last_error() and entry.split("_device")[0].encode() in lib.ivfadc_last_error()
    assert argtypes is not STORE or args[4] is None or OUT.value is None, "a refused call hands out no store"


def test_symbols_counts_and_python_surface(native):
    lib = native.load_library()
    assert hasattr(lib, "ivfadc_vectors_destroy")
    lib.ivfadc_vectors_sizes.argtypes = [VP] * 4
    assert lib.ivfadc_vectors_sizes(None, None, None, None) == INVALID and b"null store" in lib.ivfadc_last_error()
    lib.ivfadc_rerank.argtypes = RERANK
    assert lib.ivfadc_rerank(FAKE, FAKE, 0, None, 4, None, None, 3, None, None, None) == 0, "no queries: nothing is looked at"
    counts = np.array([4, 5, 0], np.int32)                                # the host entry reads the counts
    assert lib.ivfadc_rerank(FAKE, FAKE, 3, P, 4, P, VP(counts.ctypes.data), 3, P, P, P) == INVALID
    assert b"query 1" in lib.ivfadc_last_error() and b"counts = 5" in lib.ivfadc_last_error() and b"[0, 4]" in lib.ivfadc_last_error()
    assert all(callable(getattr(native, name)) and name in native.__all__ for name in ("rerank", "knn_search_refined"))
