"""CPU checks of the seam between coarse_search and the rest of knn_search (include/ivfadc_hip.h: ivfadc_coarse_search*,
ivfadc_search*_preassigned): the symbols and wrappers exist, a null handle is refused before any device call, and the numpy
restatement the GPU tests compare against -- pre_knn, index.jl:220-257 given ANY coarse result -- is itself checked here:
fed with the true coarse order it is helpers.numpy_knn, and on the test inputs it tells "skip a list above the bound" from
"stop at the first list above the bound" (the rule of a plain search, whose probes ascend)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import helpers

f32 = np.float32
SYMBOLS = ("ivfadc_coarse_search", "ivfadc_coarse_search_device", "ivfadc_search_preassigned", "ivfadc_search_device_preassigned")


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _probe_sums(oidx, q, cl, dc):
    """ADC sums of list cl for query q seeded with dc (index.jl:229-244), reference order; None for an empty list."""
    lo, hi = int(oidx.offsets[cl]), int(oidx.offsets[cl + 1])
    if hi <= lo:
        return None, None
    r = q - oidx.centroids[cl]
    tab = np.zeros((oidx.m, 256), f32)
    for i in range(oidx.m):
        tab[i, oidx.labels[i]] = helpers.ref_table(oidx, i, r)
    return helpers.ref_adc(f32(dc), [tab[ii, oidx.codes[lo:hi, ii]] for ii in range(oidx.m)]), oidx.ids[lo:hi]


def pre_knn(oidx, q, K, lists, dcs, stop_at_first_above=False):
    """knn_search behind its coarse_search call: the supplied probes in the supplied order, every sum seeded with the SUPPLIED
    distance, residuals against the supplied list's centroid; an exhaustive (dist, visit order) list, then a lexicographic sort.
    stop_at_first_above: emulates the plain search's pruning rule on these probes -- the query ends at the first probe whose
    distance bits exceed those of the K-th best distance found so far (right only when the probes ascend)."""
    q = np.asarray(q, f32)
    cand_d, cand_id = [], []
    for cl, dc in zip(np.asarray(lists).tolist(), np.asarray(dcs, f32).tolist()):
        if stop_at_first_above and cand_d:
            sofar = np.sort(np.concatenate(cand_d).view(np.uint32))
            if sofar.shape[0] >= K and int(np.array([dc], f32).view(np.uint32)[0]) > int(sofar[K - 1]):
                break
        dd, ii = _probe_sums(oidx, q, cl, dc)
        if dd is not None:
            cand_d.append(dd)
            cand_id.append(ii)
    cd = np.concatenate(cand_d) if cand_d else np.zeros(0, f32)
    ci = np.concatenate(cand_id) if cand_id else np.zeros(0, np.uint32)
    sel = np.lexsort((np.arange(cd.shape[0]), cd.view(np.uint32)))[:K]
    return ci[sel], cd[sel]


def pre_knn_batch(oidx, qs, K, lists, dcs, **kw):
    qs = np.asarray(qs, f32).reshape(-1, oidx.d)
    ids = np.zeros((qs.shape[0], K), np.uint32)
    dists = np.full((qs.shape[0], K), np.inf, f32)
    counts = np.zeros(qs.shape[0], np.int32)
    for r in range(qs.shape[0]):
        i, dd = pre_knn(oidx, qs[r], K, lists[r], dcs[r], **kw)
        counts[r] = len(i)
        ids[r, :len(i)] = i
        dists[r, :len(i)] = dd
    return ids, dists, counts


def true_coarse(oidx, qs, w):
    """coarse_search of every query: (lists (nq, w) int32, dists (nq, w) float32), ascending, ties to the lower cell."""
    lists = np.zeros((qs.shape[0], w), np.int32)
    dists = np.zeros((qs.shape[0], w), f32)
    for r in range(qs.shape[0]):
        acc = helpers.ref_coarse(oidx, qs[r])
        o = np.lexsort((np.arange(oidx.kc), acc))[:w]
        lists[r], dists[r] = o, acc[o]
    return lists, dists


def interleave(oidx, qs, w):
    """nearest, farthest, 2nd nearest, 2nd farthest, ... of ALL the cells of every query (w / 2 from either end of the true coarse
    order), each probe with its true distance"""
    lists, dists = true_coarse(oidx, qs, oidx.kc)
    perm = []
    for j in range((w + 1) // 2):
        perm.append(j)
        if len(perm) < w:
            perm.append(oidx.kc - 1 - j)
    return np.ascontiguousarray(lists[:, perm]), np.ascontiguousarray(dists[:, perm])


_TEETH = {}


def teeth_input(shape="m8"):
    """The input the pruning rule is judged on: 40 queries, w = 8, probes interleaved near / far with their true distances.
    m8: build_index(7, 4000, 32, 32, 8) and default_rng(5).random queries -- the query-major exact rounds.
    m16: m = 16, d = 96, where the matrix-core lower-bound rounds are instantiated (no m = 8 shape has them).  Uniform data in 96
    dimensions never prunes (every ADC sum exceeds the farthest coarse distance), so the centroids come in close pairs and the
    queries lie near a centroid: the two nearest lists share the top-K, every far list lies above the bound."""
    if shape not in _TEETH:
        rng = np.random.default_rng(5)
        if shape == "m8":
            oidx, _ = helpers.build_index(7, 4000, 32, 32, 8, mode="random")
            qs = rng.random((40, oidx.d), dtype=f32)
        else:
            oidx, _ = helpers.build_index(7, 4000, 96, 32, 16, mode="random")
            oidx.centroids[1::2] = oidx.centroids[0::2] + f32(0.05) * (rng.random((16, 96), dtype=f32) - f32(0.5))
            qs = oidx.centroids[rng.integers(0, 32, 40)] + f32(0.1) * (rng.random((40, 96), dtype=f32) - f32(0.5))
            qs = np.ascontiguousarray(qs, f32)
        lists, dists = interleave(oidx, qs, 8)
        _TEETH[shape] = (oidx, qs, lists, dists)
    return _TEETH[shape]


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported(native):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ivfadc_hip.h")).read(), flags=re.S)
    lib = native.load_library()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, txt), "%s is not declared in include/ivfadc_hip.h" % s
        assert hasattr(lib, s), "libivfadc_hip.so does not export %s" % s
        assert getattr(lib, s).argtypes is not None, "%s has no argtypes in _native.py" % s
    assert int(re.search(r"#define\s+IVFADC_ABI_VERSION\s+(\d+)", txt).group(1)) == 4      # no existing prototype changed


def test_null_handle_is_refused_without_a_device_call(native):
    lib = native.load_library()
    z = np.zeros(8, f32)
    zi = np.zeros(8, np.int32)
    zu = np.zeros(8, np.uint32)
    fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    pf, pi, pu = z.ctypes.data_as(fp), zi.ctypes.data_as(ip), zu.ctypes.data_as(up)
    assert lib.ivfadc_coarse_search(None, 1, pf, 1, pi, pf) == 2 and b"null handle" in lib.ivfadc_last_error()
    assert lib.ivfadc_coarse_search_device(None, 1, None, 1, None, None) == 2 and b"null handle" in lib.ivfadc_last_error()
    assert lib.ivfadc_search_preassigned(None, 1, pf, 1, 1, pi, pf, pu, pf, pi) == 2 and b"null handle" in lib.ivfadc_last_error()
    assert lib.ivfadc_search_device_preassigned(None, 1, None, 1, 1, None, None, None, None, None) == 2
    assert b"null handle" in lib.ivfadc_last_error()


def test_python_wrappers_exist(native):
    for name in ("coarse_search_raw", "search_preassigned_raw", "coarse_search_device", "search_device_preassigned"):
        assert callable(getattr(native.IVFADCIndex, name, None)), name
    for name in ("coarse_search", "knn_search_preassigned"):
        assert callable(getattr(native, name, None)), name
        assert name in native.__all__
    # the assertion texts of knn_search (index.jl:210-211), before anything native is touched
    with pytest.raises(AssertionError, match="k >= 1"):
        native.knn_search_preassigned(None, np.zeros(4, f32), 0, [0], [0.0])
    with pytest.raises(AssertionError, match="w >= 1"):
        native.coarse_search(None, np.zeros(4, f32), 0)


@pytest.mark.parametrize("K,w", [(1, 1), (10, 8), (300, 5)])
def test_pre_knn_with_the_true_coarse_order_is_numpy_knn(K, w):
    oidx, qs, _, _ = teeth_input("m8")
    lists, dists = true_coarse(oidx, qs[:12], w)
    for r in range(12):
        gi, gd = pre_knn(oidx, qs[r], K, lists[r], dists[r])
        ei, ed = helpers.numpy_knn(oidx, qs[r], K, w)
        assert np.array_equal(gi, ei) and np.array_equal(gd.view(np.uint32), ed.view(np.uint32)), r


@pytest.mark.parametrize("shape", ["m8", "m16"])
def test_the_inputs_tell_skip_from_stop(shape):
    """Teeth.  On the interleaved probes, ending a query at the first probe above the K-th best distance (what a plain search
    does, rightly, on ascending probes) changes the result of at least one query for each K the GPU tests use: if this ever
    fails, the inputs no longer exercise the rule and the GPU comparison with pre_knn proves nothing about it.
    Measured on the m8 input: 5 / 14 / 19 of 40 queries at K = 1 / 3 / 10."""
    oidx, qs, lists, dists = teeth_input(shape)
    assert not (np.diff(dists.view(np.uint32).astype(np.int64), axis=1) >= 0).all(axis=1).any(), "a row of the interleaved distances ascends"
    changed = {}
    for K in (1, 3, 10):
        full = pre_knn_batch(oidx, qs, K, lists, dists)
        cut = pre_knn_batch(oidx, qs, K, lists, dists, stop_at_first_above=True)
        changed[K] = sum(1 for r in range(qs.shape[0])
                         if full[2][r] != cut[2][r] or not np.array_equal(full[0][r], cut[0][r]) or
                         not np.array_equal(full[1][r].view(np.uint32), cut[1][r].view(np.uint32)))
    print("queries changed by stopping at the first probe above the bound (%s): %s" % (shape, changed))
    for K in (1, 3, 10):
        assert changed[K] >= 1, (shape, changed)
    if shape == "m8":
        assert changed == {1: 5, 3: 14, 10: 19}, changed
