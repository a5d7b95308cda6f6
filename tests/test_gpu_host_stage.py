"""The host-pointer service entries share one staging arena per handle (csrc/host_stage.h): on ONE handle the arena grows
(rerank), is carved again far smaller (locate, score_ids: a 15-byte part in front of a float part), grows again (reconstruct: 384 KB
at d = 32, over the bounce threshold at a non-zero arena offset), serves coarse_search, range_search and search_refined, and the first
rerank once more.  Every result equals, byte for byte, the same call on a fresh handle of the same index and the device-pointer entry fed
torch tensors (result rows: up to each query's count); the repeated rerank equals its first run.  No tolerance anywhere."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu
N, KC, M = 3000, 16, 2
F32, U32, I32 = np.float32, np.uint32, np.int32
_CASES = {}


def handle(native, c):
    o = c["oidx"]
    return native.IVFADCIndex.from_arrays(o.centroids, o.codebooks, o.labels, o.offsets, o.codes, o.ids)


def case(native, d):
    """the index, the vector store and every call's arguments: made once per d, never changed"""
    if d not in _CASES:
        oidx, data = helpers.build_index(40 + d, N, d, KC, M)
        rng = np.random.default_rng(d)
        c = {"oidx": oidx, "d": d}
        c["q"] = rng.random((70, d), dtype=F32)
        c["cand"] = rng.integers(0, N + 5, (70, 300)).astype(U32)          # (an id at or past N is dropped)
        c["cand_counts"] = rng.integers(0, 301, 70).astype(I32)
        c["cand_counts"][:2] = 0, 300
        c["few"] = rng.integers(0, N + 5, (3, 5)).astype(U32)
        c["few_counts"] = np.array([5, 0, 2], I32)
        c["all_ids"] = rng.permutation(N + 7).astype(U32)                   # every stored id and seven that no list holds
        g = handle(native, c)
        c["store"] = g.vectors(data)
        c["radii"] = np.ascontiguousarray(g.search_raw(c["q"], 25, 4)[1][:, 24])
        c["radii"][:3] = -1.0, np.inf, 0.0
        _CASES[d] = c
    return _CASES[d]


def host_calls(c):
    st, q = c["store"], c["q"]
    rerank = lambda g: g.rerank_raw(st, q, c["cand"], 10, c["cand_counts"])
    return [("rerank", rerank),
            ("locate", lambda g: g.locate_raw(c["all_ids"][:1])),
            ("score_ids", lambda g: g.score_raw(q[:3], c["few"], c["few_counts"])),
            ("reconstruct", lambda g: g.reconstruct_raw(c["all_ids"])),
            ("coarse_search", lambda g: g.coarse_search_raw(q, 5)),
            ("range_search", lambda g: g.range_search_raw(q, c["radii"], 4)),
            ("search_refined", lambda g: g.search_refined_raw(st, q, 3, 40, 4)),
            ("rerank again", rerank)]


def device_results(g, c):
    """the device-pointer entry of every call, on torch tensors, in the shape the host entry's binding returns"""
    import torch
    from ivfadc_jl_amd import index as ix
    dev, d, st = "cuda:0", c["d"], c["store"]
    up = lambda a: torch.from_numpy(a.view(I32) if a.dtype == U32 else a).to(dev)
    new = lambda shape, dtype, fill=0: torch.full(shape, fill, dtype=dtype, device=dev)
    rows = lambda k: (new((70, k), torch.int32), new((70, k), torch.float32, np.inf), new((70,), torch.int32))
    q, cand, cand_counts, few, few_counts, ids, radii = (up(c[k]) for k in ("q", "cand", "cand_counts", "few", "few_counts", "all_ids", "radii"))
    n = ids.shape[0]
    rr, rf = rows(10), rows(3)
    one = (new((1,), torch.int32), new((1,), torch.int64))
    sc = (new((3, 5), torch.float32), new((3, 5), torch.uint8))
    rec = (new((n, d), torch.float32), new((n,), torch.uint8))
    co = (new((70, 5), torch.int32), new((70, 5), torch.float32))
    torch.cuda.synchronize()
    g.rerank_device(st, 70, q.data_ptr(), 300, cand.data_ptr(), cand_counts.data_ptr(), 10, *(t.data_ptr() for t in rr))
    g.locate_device(1, ids.data_ptr(), *(t.data_ptr() for t in one))
    g.score_device(3, q.data_ptr(), 5, 5, few.data_ptr(), few_counts.data_ptr(), *(t.data_ptr() for t in sc))
    g.reconstruct_device(n, ids.data_ptr(), *(t.data_ptr() for t in rec))
    g.coarse_search_device(70, q.data_ptr(), 5, *(t.data_ptr() for t in co))
    res = g.range_search_device(70, q.data_ptr(), radii.data_ptr(), 4)
    g.search_device_refined(st, 70, q.data_ptr(), 3, 40, 4, *(t.data_ptr() for t in rf))
    g.sync()
    rng_rows = ix.range_result_copy(res)
    ix.range_result_destroy(res)
    host = lambda ts: tuple(t.cpu().numpy() for t in ts)
    result_rows = lambda ts: (host(ts)[0].view(U32),) + host(ts)[1:]
    flagged = lambda ts: (host(ts)[0], host(ts)[1].astype(bool))
    return {"rerank": result_rows(rr), "locate": host(one), "score_ids": flagged(sc), "reconstruct": flagged(rec), "coarse_search": host(co),
            "range_search": rng_rows, "search_refined": result_rows(rf), "rerank again": result_rows(rr)}


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def found_slots(name, r):
    """result rows (ids, distances, counts): the slots at or behind a query's count are not part of the result"""
    if name.split()[0] not in ("rerank", "search_refined"):
        return r
    ids, dists, counts = (np.array(x) for x in r)
    dead = np.arange(ids.shape[1])[None, :] >= counts[:, None]
    ids[dead], dists[dead] = 0, np.inf
    return ids, dists, counts


@pytest.mark.parametrize("d", (10, 32))
def test_one_handle_serves_the_sequence_as_fresh_handles_do(native, d):
    c = case(native, d)
    calls = host_calls(c)
    g = handle(native, c)
    got = [f(g) for _, f in calls]                       # the sequence, on one handle
    dev = device_results(handle(native, c), c)
    for (name, f), r in zip(calls, got):
        assert same(r, f(handle(native, c))), "%s: differs from the same call on a fresh handle" % name
        assert same(found_slots(name, r), found_slots(name, dev[name])), "%s: differs from the device-pointer entry" % name
    assert same(got[-1], got[0]), "the repeated rerank differs from its first run"
    assert got[0][2].max() == 10 and got[0][2][0] == 0 and got[3][1].sum() == N and len(got[5][1]) > 70   # (the calls found something)
