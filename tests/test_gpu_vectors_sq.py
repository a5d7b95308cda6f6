"""The 8-bit scalar-quantised vector store on the GPU against plain numpy.  Integer data with the range [0, 255] makes step = inv = 1, the
codes the data and every partial sum exact in Float32: ids, order and distances must EQUAL a float64 computation with a stable sort on
(distance, slot).  Gaussian data with a trained range is checked bit for bit: range, codes and the chain on the reconstruction in numpy Float32."""
import ctypes as C

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu
N, F32, MAX_D = 3000, np.float32, 10240                    # MAX_D: csrc/vstore_sq_plan.h


def handle(native, d):
    return native.IVFADCIndex.from_arrays(np.zeros((1, d), F32), np.zeros((1, 2, d), F32), np.arange(2, dtype=np.uint8)[None, :])


def reference(data, qs, ids, counts, k, chain32=False):
    """per query: (ids, distances) of the k live slots with id < n smallest under (distance, slot)"""
    out = []
    for q in range(len(qs)):
        row = ids[q][:len(ids[q]) if counts is None else counts[q]]
        row = row[row < len(data)]
        s = np.zeros(len(row), F32) if chain32 else ((data[row].astype(np.float64) - qs[q].astype(np.float64)) ** 2).sum(1)
        for t in range(data.shape[1] if chain32 else 0):
            u = data[row, t] - qs[q, t]
            s = s + u * u
        order = np.argsort(s, kind="stable")[:k]
        out.append((row[order], s[order]))
    return out


def assert_equal(got, exp, bits=False):
    ids, dists, counts = got
    for q, (ei, ed) in enumerate(exp):
        gd = dists[q, :counts[q]]
        assert counts[q] == len(ei) and np.array_equal(ids[q, :counts[q]], ei), (q, counts[q], ids[q, :counts[q]], ei)
        assert np.array_equal(gd.view(np.uint32), ed.view(np.uint32)) if bits else np.array_equal(gd.astype(np.float64), ed), (q, gd, ed)


def exact_case(d, C, K, n):
    """integer data with a tied pair across the 64-slot boundary and one across the K boundary (ids n-8.. are spare copies)"""
    rng = np.random.default_rng(7 * d + C)
    top = 256 if d < 768 else 101 if d == 768 else 41       # every partial sum below 2^24: 272 * 255^2, 768 * 100^2, 10240 * 40^2
    data, qs = rng.integers(0, top, (n, d)).astype(F32), rng.integers(0, top, (3, d)).astype(F32)
    ids = rng.integers(0, n - 8, (3, C)).astype(np.uint32)
    if C >= 65:
        data[n - 1] = data[n - 2]
        ids[:, 63], ids[:, 64] = n - 2, n - 1
    for q in range(3 if K < C else 0):
        s = ((data[ids[q]].astype(np.float64) - qs[q]) ** 2).sum(1)
        order = np.argsort(s, kind="stable")
        b = next(int(j) for j in order[K:] if j not in (63, 64))
        data[n - 8 + q], ids[q, b] = data[ids[q, order[K - 1]]], n - 8 + q
        s[b] = s[order[K - 1]]
        assert np.sort(s)[K - 1] == np.sort(s)[K]
    return data, qs, ids


def restate(data, lo, inv):
    return np.clip(np.rint((data - lo) * inv), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("d,C,n", [(d, 257, N) for d in (1, 10, 16, 33, 128, 129, 144, 272, 768)] + [(32, C, N) for C in (1, 63, 64, 65, 4096, 4097)]
                         + [(MAX_D, 65, 80)])
def test_exact_against_float64(native, d, C, n):
    data, qs, ids = exact_case(d, C, 10, n)
    g, stride = handle(native, d), -(-d // 16) * 16
    store = g.vectors_sq(data, lo=0, hi=255)
    assert (len(store), store.d, store.dtype, store.bytes_per_row, store.nbytes) == (n, d, "sq8", stride, n * stride + 3 * 4 * (-(-d // 4) * 4))
    lo, step, inv, codes = store.sq_arrays()
    assert not lo.any() and (step == 1).all() and (inv == 1).all() and np.array_equal(codes, data.astype(np.uint8))
    assert_equal(g.rerank_raw(store, qs, ids, 10), reference(data, qs, ids, None, 10))


def test_encoder_rounds_half_to_even_and_clamps(native):
    """inv = 0.5 exactly: every odd integer lands on a half"""
    data = (2 * np.random.default_rng(1).integers(-20, 280, (N, 16)) + 1).astype(F32)
    data[0, :4] = -1, 1, 509, 511
    lo, step, inv, codes = handle(native, 16).vectors_sq(data, lo=0, hi=510).sq_arrays()
    assert (step == 2).all() and (inv == 0.5).all() and data.min() < 0 and data.max() > 510
    assert np.array_equal(codes, restate(data, lo, inv)) and list(codes[0, :4]) == [0, 0, 254, 255]


@pytest.mark.parametrize("d", (10, 128))
def test_bit_for_bit_on_gaussian_data_with_a_trained_range(native, d):
    rng = np.random.default_rng(d)
    data, qs = rng.standard_normal((N, d)).astype(F32), rng.standard_normal((3, d)).astype(F32)
    data[:, 3] = F32(0.375)                                 # a constant column: range == 0
    ids = rng.integers(0, N, (3, 257)).astype(np.uint32)
    g = handle(native, d)
    store = g.vectors(data, "sq8")
    lo, step, inv, codes = store.sq_arrays()
    span = data.max(0) - data.min(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_step, e_inv = np.where(span == 0, F32(0), span / F32(255)), np.where(span == 0, F32(0), F32(255) / span)
    assert np.array_equal(lo, data.min(0)) and np.array_equal(step, e_step.astype(F32)) and np.array_equal(inv, e_inv.astype(F32)) and step[3] == 0 == inv[3]
    assert np.array_equal(codes, restate(data, lo, inv)) and codes.max() == 255 and not codes[:, 3].any()
    assert_equal(g.rerank_raw(store, qs, ids, 257), reference(lo + codes.astype(F32) * step, qs, ids, None, 257, chain32=True), bits=True)


@pytest.mark.parametrize("d", (33, 128))
def test_device_entries_give_the_same_bytes(native, d):
    import torch
    data = np.random.default_rng(d).standard_normal((N, d)).astype(F32)
    dv = torch.from_numpy(data).to("cuda:0")
    torch.cuda.synchronize()
    g, lo, hi = handle(native, d), np.full(d, -1.5, F32), np.full(d, 2.0, F32)
    pairs = ((g.vectors_sq(data), g.vectors_sq_device(dv.data_ptr(), N)), (g.vectors(data, "sq8"), g.vectors_device(dv.data_ptr(), N, "sq8")),
             (g.vectors_sq(data, lo, hi), g.vectors_sq_device(dv.data_ptr(), N, lo, hi)))
    for host, dev in pairs:
        assert all(np.array_equal(a, b) for a, b in zip(host.sq_arrays(), dev.sq_arrays())) and host.nbytes == dev.nbytes
    assert np.array_equal(pairs[0][0].sq_arrays()[3], pairs[1][0].sq_arrays()[3])


def test_fused_call_on_8_bit_and_uint16_handles(native):
    oidx, data = helpers.build_index(5, 2000, 32, 16, 8)
    g8 = native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)
    g16 = native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels.astype(np.uint16), oidx.offsets, oidx.codes.astype(np.uint16), oidx.ids)
    data = np.round(data * 255).astype(F32)                 # integer-valued originals in the range: the re-rank is exact
    qs = np.round(np.random.default_rng(9).random((5, 32)) * 255).astype(F32)
    for g in (g8, g16):
        store = g.vectors_sq(data, lo=0, hi=255)
        c_ids, _, c_counts = g.search_raw(qs, 100, 4)
        exp = reference(data, qs, c_ids, c_counts, 10)
        assert_equal(g.search_refined_raw(store, qs, 10, 100, 4), exp)
        assert all(np.array_equal(i, e[0]) for i, e in zip(native.knn_search_refined(g, store, qs, 10, w=4, kc=100)[0], exp))


def test_slices_and_slots(native):
    """a call cut into slices by the workspace limit equals the uncut call; ragged counts with a zero, ids at n and 0xFFFFFFFF dropped"""
    rng = np.random.default_rng(4)
    data, qs = rng.integers(0, 256, (N, 10)).astype(F32), rng.integers(0, 256, (65, 10)).astype(F32)
    ids, counts = rng.integers(0, N, (65, 4096)).astype(np.uint32), rng.integers(0, 4097, 65).astype(np.int32)
    ids[:, 3], ids[:, 70], counts[0], counts[-1] = N, 0xFFFFFFFF, 0, 4096
    g = handle(native, 10)
    store = g.vectors_sq(data, lo=0, hi=255)
    whole, ragged = g.rerank_raw(store, qs, ids, 20), g.rerank_raw(store, qs, ids, 4096, counts)
    g.set_workspace_limit(1 << 20)                          # 32 queries of 4096 keys: three slices
    cut = g.rerank_raw(store, qs, ids, 20)
    assert all(np.array_equal(a, b) for a, b in zip(whole, cut)) and ragged[2][0] == 0 and ragged[2][-1] == 4094
    assert_equal(cut, reference(data, qs, ids, None, 20))
    assert_equal(ragged, reference(data, qs, ids, counts, 4096))


def test_refusals(native):
    g, good = handle(native, 4), np.ones((10, 4), F32)
    for bad in (np.nan, np.inf):
        data = good.copy()
        data[7, 2] = bad
        for kw in ({}, {"lo": 0, "hi": 2}):
            with pytest.raises(native.IVFADCError, match="not finite"):
                g.vectors_sq(data, **kw)
    for kw, word in (({"lo": 1, "hi": 0}, "hi = 0 < lo = 1"), ({"lo": -3e38, "hi": 3e38}, "not finite"), ({"lo": 0, "hi": np.inf}, "not finite"),
                     ({"lo": 0}, "only one of lo and hi"), ({"hi": 0}, "only one of lo and hi")):
        with pytest.raises(native.IVFADCError, match=word):
            g.vectors_sq(good, **kw)
    with pytest.raises(native.IVFADCError, match="d = %d" % (MAX_D + 1)):
        handle(native, MAX_D + 1).vectors_sq(np.zeros((1, MAX_D + 1), F32))
    lib, store = native.load_library(), g.vectors_sq(good)
    lib.ivfadc_vectors_get_pq.argtypes = [C.c_void_p] * 7
    assert lib.ivfadc_vectors_get_pq(store._s, None, None, None, None, None, None) == 2 and b"not a PQ store" in lib.ivfadc_last_error()
