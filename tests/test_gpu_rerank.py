"""Exact re-ranking on the GPU against plain numpy.  Integer-valued data keeps every partial sum below 2^24, so Float32 is exact and ids,
order and distances must EQUAL a float64 computation with a stable sort on (distance, slot); Gaussian data is checked bit for bit
against the same chain in numpy Float32; the fused call must equal search_raw(K = Kc) followed by the float64 reference."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu
N = 3000
F32, F16 = np.float32, np.float16


def handle(native, d):
    return native.IVFADCIndex.from_arrays(np.zeros((1, d), F32), np.zeros((1, 2, d), F32), np.arange(2, dtype=np.uint8)[None, :])


def reference(data, qs, ids, counts, k, chain32=False):
    """per query: (ids, distances) of the k live slots with id < n smallest under (distance, slot)"""
    out = []
    for q in range(len(qs)):
        row = ids[q][:len(ids[q]) if counts is None else counts[q]]
        row = row[row < len(data)]
        x = data[row]
        if chain32:
            s = np.zeros(len(row), F32)
            for t in range(data.shape[1]):
                u = x[:, t] - qs[q, t]
                s = s + u * u
        else:
            s = ((x.astype(np.float64) - qs[q].astype(np.float64)) ** 2).sum(1)
        order = np.argsort(s, kind="stable")[:k]
        out.append((row[order], s[order]))
    return out


def assert_equal(got, exp, bits=False):
    ids, dists, counts = got
    for q, (ei, ed) in enumerate(exp):
        assert counts[q] == len(ei), (q, counts[q], len(ei))
        assert np.array_equal(ids[q, :counts[q]], ei), (q, ids[q, :counts[q]], ei)
        gd = dists[q, :counts[q]]
        assert np.array_equal(gd.view(np.uint32), ed.view(np.uint32)) if bits else np.array_equal(gd.astype(np.float64), ed), (q, gd, ed)


def exact_case(d, C, K, seed):
    """integer data with a tied pair across the 64-slot boundary and one across the K boundary (ids N-8.. are spare copies)"""
    rng = np.random.default_rng(seed)
    hi = 101 if d == 768 else 256
    data, qs = rng.integers(0, hi, (N, d)).astype(F32), rng.integers(0, hi, (3, d)).astype(F32)
    ids = rng.integers(0, N - 8, (3, C)).astype(np.uint32)
    if C >= 65:
        data[N - 1] = data[N - 2]
        ids[:, 63], ids[:, 64] = N - 2, N - 1
    if K < C:
        for q in range(3):
            s = ((data[ids[q]].astype(np.float64) - qs[q]) ** 2).sum(1)
            order = np.argsort(s, kind="stable")
            b = next(int(j) for j in order[K:] if j not in (63, 64))
            data[N - 8 + q] = data[ids[q, order[K - 1]]]
            ids[q, b] = N - 8 + q
            s[b] = s[order[K - 1]]
            assert np.sort(s)[K - 1] == np.sort(s)[K]
    return data, qs, ids


EXACT = ([(d, 257, 10, t) for d in (1, 10, 32, 33, 128, 768) for t in (F32, F16)]
         + [(32, C, 10, F32) for C in (1, 63, 64, 65, 4096, 4097)] + [(10, 4097, 10, F16)]
         + [(32, 65, K, F32) for K in (1, 65, 70)])


@pytest.mark.parametrize("d,C,K,dtype", EXACT)
def test_exact_against_float64(native, d, C, K, dtype):
    data, qs, ids = exact_case(d, C, K, 7 * d + C + K)
    g = handle(native, d)
    store = g.vectors(data, dtype)
    assert (len(store), store.d, store.dtype) == (N, d, dtype)
    assert_equal(g.rerank_raw(store, qs, ids, K), reference(data, qs, ids, None, K))


@pytest.mark.parametrize("d", (10, 128))
@pytest.mark.parametrize("dtype", (F32, F16))
def test_bit_for_bit_on_gaussian_data(native, d, dtype):
    rng = np.random.default_rng(d)
    data, qs = rng.standard_normal((N, d)).astype(F32), rng.standard_normal((3, d)).astype(F32)
    ids = rng.integers(0, N, (3, 257)).astype(np.uint32)
    g = handle(native, d)
    kept = data.astype(dtype).astype(F32)
    assert_equal(g.rerank_raw(g.vectors(data, dtype), qs, ids, 257), reference(kept, qs, ids, None, 257, chain32=True), bits=True)


@pytest.mark.parametrize("nq", (1, 65))
def test_slots(native, nq):
    """ragged counts with a zero, ids at n and 0xFFFFFFFF dropped, a repeated id returned twice"""
    rng = np.random.default_rng(nq)
    d, C = 32, 130
    data, qs = rng.integers(0, 256, (N, d)).astype(F32), rng.integers(0, 256, (nq, d)).astype(F32)
    ids = rng.integers(0, N, (nq, C)).astype(np.uint32)
    ids[:, 3], ids[:, 70], ids[:, 5], ids[:, 100] = N, 0xFFFFFFFF, ids[:, 66], ids[:, 2]
    counts = rng.integers(0, C + 1, nq).astype(np.int32)
    counts[0], counts[-1] = 0 if nq > 1 else C, C
    g = handle(native, d)
    store = g.vectors(data)
    got = g.rerank_raw(store, qs, ids, C, counts)
    assert_equal(got, reference(data, qs, ids, counts, C))
    assert got[2][-1] == C - 2 and np.count_nonzero(got[0][-1, :C - 2] == ids[-1, 5]) >= 2
    assert_equal(g.rerank_raw(store, qs, ids, 10), reference(data, qs, ids, None, 10))
    assert np.array_equal(native.rerank(g, store, qs[0], ids[0], 10)[0], reference(data, qs, ids, None, 10)[0][0])


def test_float16_overflow_is_refused(native):
    g = handle(native, 4)
    data = np.ones((10, 4), F32)
    data[7, 2] = 70000.0
    with pytest.raises(native.IVFADCError, match="overflows Float16"):
        g.vectors(data, F16)
    data[7, 2] = np.inf                                     # not finite: kept as it is
    store = g.vectors(data, F16)
    assert len(store) == 10
    with pytest.raises(native.IVFADCError, match="d = 4, the handle of d = 8"):
        handle(native, 8).rerank_raw(store, np.zeros((1, 8), F32), np.zeros((1, 3), np.uint32), 2)


def indexes(native):
    oidx, data = helpers.build_index(5, 2000, 32, 16, 8)
    g8 = native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)
    g16 = native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels.astype(np.uint16), oidx.offsets,
                                         oidx.codes.astype(np.uint16), oidx.ids)
    data = np.round(data * 255).astype(F32)                 # integer-valued originals: the re-rank is exact whatever the codes say
    return {"8-bit": g8, "UInt16": g16, "view": g8.clone_view(), "subset": g8.subset(mask=np.arange(2000) % 3 != 0)}, data


@pytest.mark.parametrize("kc,w", ((10, 1), (100, 4), (100, 1), (10, 4)))
def test_fused_call(native, kc, w):
    gs, data = indexes(native)
    qs = np.round(np.random.default_rng(kc + w).random((5, 32)) * 255).astype(F32)
    for name, g in gs.items():
        store = g.vectors(data)
        c_ids, _, c_counts = g.search_raw(qs, kc, w)
        exp = reference(data, qs, c_ids, c_counts, 10)
        assert_equal(g.search_refined_raw(store, qs, 10, kc, w), exp)
        assert all(np.array_equal(i, e[0]) for i, e in zip(native.knn_search_refined(g, store, qs, 10, w=w, kc=kc)[0], exp)), name


def test_device_entries_on_the_search_outputs(native):
    import torch
    gs, data = indexes(native)
    g = gs["8-bit"]
    nq, kc, k = 65, 100, 10
    qs = np.round(np.random.default_rng(3).random((nq, 32)) * 255).astype(F32)
    dev = torch.device("cuda:0")
    dq, dv = torch.from_numpy(qs).to(dev), torch.from_numpy(data).to(dev)

    def block(width):
        return [torch.zeros(shape, dtype=t, device=dev) for shape, t in (((nq, width), torch.int32), ((nq, width), torch.float32), (nq, torch.int32))]

    (ci, cd, cc), outs = block(kc), [block(k), block(k)]
    torch.cuda.synchronize()
    store = g.vectors_device(dv.data_ptr(), len(data), F16)
    g.search_device(nq, dq.data_ptr(), kc, 4, ci.data_ptr(), cd.data_ptr(), cc.data_ptr())
    g.rerank_device(store, nq, dq.data_ptr(), kc, ci.data_ptr(), cc.data_ptr(), k, *(t.data_ptr() for t in outs[0]))
    g.search_device_refined(store, nq, dq.data_ptr(), k, kc, 4, *(t.data_ptr() for t in outs[1]))
    g.sync()
    exp = reference(data, qs, ci.cpu().numpy().view(np.uint32), cc.cpu().numpy(), k)
    for o in outs:
        assert_equal((o[0].cpu().numpy().view(np.uint32), o[1].cpu().numpy(), o[2].cpu().numpy()), exp)


@pytest.mark.parametrize("C", (4096, 4097))
def test_workspace_limit_cuts_the_call_into_slices(native, C):
    """1 MB of workspace holds 32 (LDS form) or 15 (sort form) queries of C keys: 65 queries take at least three slices"""
    rng = np.random.default_rng(C)
    data, qs = rng.integers(0, 256, (N, 10)).astype(F32), rng.integers(0, 256, (65, 10)).astype(F32)
    ids = rng.integers(0, N, (65, C)).astype(np.uint32)
    g = handle(native, 10)
    store = g.vectors(data)
    whole = g.rerank_raw(store, qs, ids, 20)
    g.set_workspace_limit(1 << 20)
    cut = g.rerank_raw(store, qs, ids, 20)
    assert all(np.array_equal(a, b) for a, b in zip(whole, cut))
    assert_equal(cut, reference(data, qs, ids, None, 20))
