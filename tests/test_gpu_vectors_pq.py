"""The PQ vector store (IVFADCIndex.vectors_pq) against plain numpy: records bit for bit against a restatement of the creation steps, the
re-rank against float64 on the reconstructions (integer data: every sum below 2^24) and against the Float32 chain (Gaussian data)."""
import functools
import os
import re

import numpy as np
import pytest

import helpers
from test_gpu_rerank import assert_equal, reference

pytestmark = pytest.mark.gpu
N, KC, F32, INVALID, STATE = 3000, 5, np.float32, 2, 4
STORES = [s + k for s in ((6, 1, 1), (10, 2, 5), (32, 8, 8), (32, 8, 2), (96, 16, 8), (128, 8, 16)) for k in ((256, 256), (5, 3))]
ROUTED = STORES + [(144, 2, 4, 256, 256), (144, 2, 4, 5, 3)]  # codewords of 72 and 36 components across chunks of 32, a last chunk of 16
ROUTED = [s + (0,) for s in ROUTED] + [s + (1,) for s in ROUTED if (s[0] // s[1]) % 4 == 0 and (s[0] // s[2]) % 4 == 0]


def chain_argmin(books, x):
    """per sub-space the first codeword of smallest sum_t (R[c][t] - x[t])^2, the sum a Float32 chain sequential in t"""
    nsub, k, dsub = books.shape
    out = np.zeros((len(x), nsub), np.uint8)
    for j in range(nsub):
        s = np.zeros((len(x), k), F32)
        for t in range(dsub):
            df = books[j, :, t][None, :] - x[:, j * dsub + t][:, None]
            s = s + df * df
        out[:, j] = np.argmin(s, axis=1)
    return out


def decode(books, codes):
    return np.concatenate([books[j][codes[:, j]] for j in range(len(books))], axis=1)


def restate(cent, books, refine, data):
    """steps 1 to 5: (lists, base codes, refinement codes) of every row"""
    lists = chain_argmin(cent[None], data)[:, 0].astype(np.int32)
    codes = chain_argmin(books, data - cent[lists])
    e = data - (cent[lists] + decode(books, codes))
    return lists, codes, chain_argmin(refine, e)


def reconstruct(cent, books, refine, lists, codes, codes2):
    return (cent[lists] + decode(books, codes)) + decode(refine, codes2)


def make(native, d, m, m2, ksub, k2, gauss=False):
    rng = np.random.default_rng(d + m + m2 + ksub)
    draw = (lambda hi, shape: rng.standard_normal(shape).astype(F32)) if gauss else (lambda hi, shape: rng.integers(0, hi, shape).astype(F32))
    cent, books, refine, data = draw(16, (KC, d)), draw(8, (m, ksub, d // m)), draw(4, (m2, k2, d // m2)), draw(32, (N, d))
    refine[:, -1] = refine[:, 0]                                 # a duplicated codeword: the lower index wins
    g = native.IVFADCIndex.from_arrays(cent, books, np.tile(np.arange(ksub, dtype=np.uint8)[::-1], (m, 1)))
    return g, g.vectors_pq(data, m2, k2, codebooks=refine), (cent, books, refine), data


@functools.lru_cache(maxsize=None)
def integer_store(native, d, m, m2, ksub, k2):
    g, store, q, data = make(native, d, m, m2, ksub, k2)
    return g, store, reconstruct(*q, *store.pq_arrays()[1:]), q, data


@pytest.mark.parametrize("d,m,m2,ksub,k2", STORES)
def test_records_bit_for_bit(native, d, m, m2, ksub, k2):
    g, store, _, (cent, books, refine), data = integer_store(native, d, m, m2, ksub, k2)
    stride = max(8, 1 << (4 + m + m2 - 1).bit_length())
    assert (len(store), store.d, store.dtype, store.m2, store.k2, store.bytes_per_row) == (N, d, "pq", m2, k2, stride)
    for name, a, b in zip(("books", "lists", "codes", "codes2"), store.pq_arrays(), (refine,) + restate(cent, books, refine, data)):
        assert np.array_equal(a, b), (name, np.argwhere(a != b)[:5])


@pytest.mark.parametrize("C,K", [(C, 10) for C in (1, 63, 64, 65, 257, 4097)] + [(257, 1), (257, 65)])
@pytest.mark.parametrize("d,m,m2,ksub,k2,route", ROUTED)
def test_rerank_exact(native, d, m, m2, ksub, k2, route, C, K):
    """a repeated id is an exact tie: one across the 64-slot boundary, one across the K boundary; dead slots and ids >= n.
    route 1 (a chunk's codebook slices staged in LDS) serves the stores whose d / m and d / m2 are multiples of four"""
    g, store, recon, _, _ = integer_store(native, d, m, m2, ksub, k2)
    store.set_pq_route(route)
    rng = np.random.default_rng(C + K)
    qs, ids = rng.integers(0, 48, (3, d)).astype(F32), rng.integers(0, N, (3, C)).astype(np.uint32)
    counts = np.array([C, C, C // 2], np.int32)
    if C >= 65:
        ids[:, 64], ids[:, 5], ids[0, 3] = ids[:, 63], 0xFFFFFFFF, N
    if K < C:
        for q in range(2):
            order = [int(j) for j in np.argsort(((recon[np.minimum(ids[q], N - 1)].astype(np.float64) - qs[q]) ** 2).sum(1), kind="stable")
                     if ids[q, j] < N and j not in (63, 64)]
            ids[q, order[K]] = ids[q, order[K - 1]]
    assert_equal(g.rerank_raw(store, qs, ids, K, counts), reference(recon, qs, ids, counts, K))


@pytest.mark.parametrize("d,m,m2,route", ((10, 2, 5, 0), (128, 8, 16, 0), (128, 8, 16, 1)))
def test_bit_for_bit_on_gaussian_data(native, d, m, m2, route):
    g, store, q, _ = make(native, d, m, m2, 256, 256, gauss=True)
    store.set_pq_route(route)
    rng = np.random.default_rng(d)
    qs, ids = rng.standard_normal((3, d)).astype(F32), rng.integers(0, N, (3, 257)).astype(np.uint32)
    assert_equal(g.rerank_raw(store, qs, ids, 257), reference(reconstruct(*q, *store.pq_arrays()[1:]), qs, ids, None, 257, chain32=True), bits=True)


def test_trained_store(native):
    cent, books, labels = helpers.make_quantizers(5, 32, 16, 8, 256)
    g = native.IVFADCIndex.from_arrays(cent, books, labels)
    rng = np.random.default_rng(11)                              # 3000 points around 40 sub-centres around the index's centroids
    sub = cent[rng.integers(0, len(cent), 40)] + 0.5 * rng.standard_normal((40, 32))
    data = (sub[rng.integers(0, 40, N)] + 0.02 * rng.standard_normal((N, 32))).astype(F32)
    a, b = (g.vectors_pq(data, 8, 16, seed=3).pq_arrays() for _ in range(2))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "one seed, one store"
    for name, x, y in zip(("lists", "codes", "codes2"), a[1:], restate(cent, books, a[0], data)):
        assert np.array_equal(x, y), name
    base = ((data - (cent[a[1]] + decode(books, a[2]))) ** 2).sum(1).mean()
    fine = ((data - reconstruct(cent, books, *a)) ** 2).sum(1).mean()
    print("mean squared reconstruction error: base %.4f, refined %.4f" % (base, fine))
    # on the CPU with sklearn.KMeans(16, n_init=1) in the trainer's place (three seeds): base 4.005, refined 0.440 .. 0.453 -- a factor of 9
    assert fine < base / 2


def trained(native):
    oidx, data = helpers.build_index(5, 2000, 32, 16, 8)
    return oidx, native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids), data


@pytest.mark.parametrize("kc,w", ((10, 1), (100, 4)))
def test_fused_call(native, kc, w):
    oidx, g, data = trained(native)
    store = g.vectors_pq(data, 8, 16)
    recon = reconstruct(oidx.centroids, oidx.codebooks, *store.pq_arrays())
    qs = np.random.default_rng(kc + w).random((5, 32)).astype(F32)
    c_ids, _, c_counts = g.search_raw(qs, kc, w)
    exp = reference(recon, qs, c_ids, c_counts, 10, chain32=True)
    assert_equal(g.search_refined_raw(store, qs, 10, kc, w), exp, bits=True)
    assert all(np.array_equal(i, e[0]) for i, e in zip(native.knn_search_refined(g, store, qs, 10, w=w, kc=kc)[0], exp))


def test_refusals(native):
    import torch
    oidx, g, data = trained(native)
    u16 = native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels.astype(np.uint16))
    bad = np.where(np.arange(data.size).reshape(data.shape) == 7 * 32 + 3, F32(np.inf), data)
    opq = native.load_ivfadc_index(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "persistency_hand_f32_u16_opq.bin"))
    part = g.clone_view()
    part.set_list_partition(2, 1)
    wide = native.IVFADCIndex.from_arrays(np.zeros((1, 128), F32), np.zeros((64, 2, 2), F32), np.tile(np.arange(2, dtype=np.uint8), (64, 1)))
    long = native.IVFADCIndex.from_arrays(np.zeros((1, 16385), F32), np.zeros((1, 2, 16385), F32), np.arange(2, dtype=np.uint8)[None])
    dbad = torch.from_numpy(bad).cuda()
    odd = g.vectors_pq(data, 16)                                 # d / m2 = 2: the staged route does not serve it
    for call, args, status, word in (
            (u16.vectors_pq, (data, 8), STATE, "UInt16"), (opq.vectors_pq, (np.zeros((4, opq.d), F32), 1, 2), STATE, ":opq"),
            (part.vectors_pq, (data, 8), STATE, "list-partitioned"), (g.vectors_pq, (data, 5), INVALID, "d % m2"),
            (g.vectors_pq, (data, 8, 257), INVALID, "k2 = 257"), (g.vectors_pq, (data[:9], 8, 16), INVALID, "rows trained on"),
            (g.vectors_pq, (data, 8, 16, None, 25, 0, 15), INVALID, "rows trained on"),
            (g.vectors_pq, (bad, 8), INVALID, "not finite: row 7, component 3"), (g.vectors_pq_device, (dbad.data_ptr(), len(bad), 8), INVALID, "not finite"),
            (wide.vectors_pq, (np.zeros((4, 128), F32), 64, 2), INVALID, "m + m2"), (long.vectors_pq, (np.zeros((4, 16385), F32), 1, 2), INVALID, "d = 16385"),
            (odd.set_pq_route, (1,), INVALID, "staged route"), (odd.set_pq_route, (2,), INVALID, "route = 2")):
        with pytest.raises(native.IVFADCError, match=re.escape(word)) as err:
            call(*args)
        assert err.value.code == status, word


@pytest.mark.parametrize("args", ((8, 256, "given"), (8, 16, None, 25, 3)))
def test_device_entry_builds_the_same_store(native, args):
    """ivfadc_vectors_create_pq_device from rows in device memory: the records and codebooks of the host entry, supplied and trained"""
    import torch
    g, _, (_, _, refine), data = make(native, 32, 8, 8, 256, 256)
    args = tuple(refine if a == "given" else a for a in args)
    dv = torch.from_numpy(data).cuda()
    store, dstore = g.vectors_pq(data, *args), g.vectors_pq_device(dv.data_ptr(), len(data), *args)
    assert all(np.array_equal(a, b) for a, b in zip(dstore.pq_arrays(), store.pq_arrays())) and dstore.bytes_per_row == store.bytes_per_row
