"""The latency path of the masked search (ivfadc_set_masked_latency(h, 1); csrc/sqmask.hip.h, sq_masked_kernel): one launch whose
point loop reads the mask first and consumes selected positions 64 at a time from a pending queue.  Every result is compared bit for
bit with the model of tests/masked.py, with the same call on the path the setting leaves alone (masked_scan_kernel), and with subset
views or the plain search.  Handles, mask sets and models are the ones tests/test_gpu_masked.py builds once."""
import numpy as np
import pytest

import helpers
import list_end as le
import masked as mk
import write_path as wp
from oracle import oracle as ora
from test_gpu_masked import check_all, model_of, refuses, setup_of

pytestmark = pytest.mark.gpu
same = helpers.assert_same_results


def search(g, on, *args, chunk=0, **kw):
    """(result, stats) of g.search_masked_raw with the setting on / off; the handle is left as it was found"""
    g.set_masked_latency(on)
    g.set_tuning(0, chunk)
    try:
        return g.search_masked_raw(*args, **kw), g.get_stats()
    finally:
        g.set_tuning(0, 0)
        g.set_masked_latency(0)


# ---- 1. read-back at the edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 64])
@pytest.mark.parametrize("w", [1, mk.KC])
@pytest.mark.parametrize("K", [1, 10, 64])
@pytest.mark.parametrize("stride", mk.U8_STRIDES)
def test_read_back_at_the_edges(native, stride, K, w, chunk):
    """chunk 64 cuts the 1025-point list into 17 work items: the last arriver merges many partial results, the last of one point"""
    c = mk.case(stride)
    g, ms = setup_of(native, stride)
    got, st = search(g, 1, c.qs, K, ms, mk.MASK_OF_QUERY, w=w, chunk=chunk)
    what = "%s K=%d w=%d chunk=%d" % (stride, K, w, chunk)
    assert st["last_qg"] == -3 and st["last_chunk"] == (chunk or 2048) and st["last_scan_grid"] == mk.NQ * w * (17 if chunk else 1), (what, st)
    same(got, model_of(stride, K, w), what=what + ": the model")
    off, st0 = search(g, 0, c.qs, K, ms, mk.MASK_OF_QUERY, w=w, chunk=chunk)
    assert st0["last_qg"] != -3 and st0["last_striped"] == 8, (what, st0)
    same(got, off, what=what + ": the setting off")
    if w == mk.KC:
        check_all(native, stride, K, got, what)


# ---- 2. queue boundaries -------------------------------------------------------------------------------------------------------------
N2 = 5 * 4096 + 65 + 10          # one list: 321 rounds and 11 points; a work item of 20032 points is two mask loads of its waves (79 rounds each)
SELECTED = {                     # positions of the list (ids are positions)
    "none": np.arange(0),
    "one": np.array([N2 // 2]),
    "63": np.arange(63) * 321,
    "64": np.arange(64) * 321,
    "65": np.arange(65) * 316,
    "all": np.arange(N2),
    "first": np.array([0]),
    "last": np.array([N2 - 1]),
    "last partial round": np.arange(N2 - N2 % 64, N2),
    "every other": np.arange(0, N2, 2),
    "every third": np.arange(0, N2, 3),       # 21 or 22 a round: the queue fills in the middle of a round and the ring wraps unaligned
}


@pytest.fixture(scope="module", params=[(128, 8), (128, 16), (32, 8)], ids=lambda p: "d%d_m%d" % p)
def one_list(native, request):
    d, m = request.param
    rng = np.random.default_rng(5150 + m + d)
    cent, cbs, labels = helpers.make_quantizers(31 + m, d, 2, m, 256)
    codes = rng.integers(0, 256, (N2, m)).astype(np.uint8)
    ref = ora.OracleIndex(cent, cbs, labels, np.array([0, N2, N2], np.int64), codes, np.arange(N2, dtype=np.uint32))
    g = wp.gpu_handle(native, ref)
    masks = [np.isin(np.arange(N2), s) for s in SELECTED.values()]
    qs = rng.random((len(masks), d), dtype=np.float32)
    views = [g.subset(mask=x).search_raw(qs[r:r + 1], 64, 2) for r, x in enumerate(masks)]
    return g, g.maskset(masks=masks), qs, tuple(np.concatenate([v[i] for v in views]) for i in range(3))


@pytest.mark.parametrize("chunk", [0, 20032])
def test_queue_boundaries(one_list, chunk):
    g, ms, qs, views = one_list
    moq = np.arange(len(SELECTED), dtype=np.int32)
    got, st = search(g, 1, qs, 64, ms, moq, w=2, chunk=chunk)
    assert st["last_qg"] == -3 and st["last_chunk"] == (chunk or 4096), st
    assert got[2].tolist() == [min(64, len(s)) for s in SELECTED.values()], got[2]
    same(got, views, what="queue boundaries chunk=%d: subset views" % chunk)
    same(got, search(g, 0, qs, 64, ms, moq, w=2)[0], what="queue boundaries chunk=%d: the setting off" % chunk)


# ---- 3. hostile spare capacity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutated", [True, False])
@pytest.mark.parametrize("kind", ["m8_d128", "m16_d128"])
def test_hostile_spare_capacity(native, kind, mutated):
    """tests/list_end.py's index: what lies behind list_len would be every query's best candidate.  An all-ones mask made after the
    mutations selects every stored id; the bits behind list_len are 0 and the words are cut at the chunk's end all the same."""
    from test_gpu_list_end import Walker
    wk = Walker(native, kind, mutated=mutated)
    if mutated:
        wk.advance("appended")
    g, qs = wk.g, wk.case.qs
    ms = g.maskset(masks=[np.ones(int(wk.lists[2].max()) + 1, bool)])
    for K in (1, 64):
        plain = g.search_raw(qs, K, le.W)
        parts = [search(g, 1, qs[q0:q0 + 64], K, ms, None, w=le.W) for q0 in range(0, len(qs), 64)]
        assert all(st["last_qg"] == -3 for _, st in parts)
        got = tuple(np.concatenate([p[0][i] for p in parts]) for i in range(3))
        same(got, plain, what="hostile %s K=%d: the plain search" % (kind, K))
        same(got, wk.expected(K), what="hostile %s K=%d: the reference" % (kind, K))


# ---- 4. device entry and refusals ------------------------------------------------------------------------------------------------------
def test_device_entry(native):
    import torch
    stride, K = "u8_m10", 64
    c = mk.case(stride)
    g, ms = setup_of(native, stride)
    dq = torch.from_numpy(c.qs).to("cuda:0")
    out = [torch.zeros(s, dtype=t, device="cuda:0") for s, t in (((mk.NQ, K), torch.int32), ((mk.NQ, K), torch.float32), ((mk.NQ,), torch.int32))]
    bad = mk.MASK_OF_QUERY.copy()
    bad[0], bad[1] = 1000, -1000
    clamped = mk.MASK_OF_QUERY.copy()
    clamped[0], clamped[1] = 15, -1
    for what, moq, host_moq in (("as given", mk.MASK_OF_QUERY, mk.MASK_OF_QUERY), ("null", None, None), ("clamped", bad, clamped)):
        dm = torch.from_numpy(moq).to("cuda:0") if moq is not None else None
        torch.cuda.synchronize()
        g.set_masked_latency(1)
        try:
            g.search_device_masked(ms, mk.NQ, dq.data_ptr(), K, mk.KC, dm.data_ptr() if dm is not None else 0, *(o.data_ptr() for o in out))
            g.sync()
            assert g.get_stats()["last_qg"] == -3
        finally:
            g.set_masked_latency(0)
        got = (out[0].cpu().numpy().view(np.uint32), out[1].cpu().numpy(), out[2].cpu().numpy())
        same(got, search(g, 1, c.qs, K, ms, host_moq, w=mk.KC)[0], what="device entry, mask numbers " + what)
        same(got, search(g, 0, c.qs, K, ms, host_moq, w=mk.KC)[0], what="device entry, mask numbers %s: the setting off" % what)


@pytest.mark.parametrize("stride,K,reps,w", [("u16_m8", 64, 1, mk.KC), ("u8_m8", 65, 1, mk.KC), ("u8_m8", 64, 3, 9)],
                         ids=["UInt16 codes", "K = 65", "nq w = 513"])
def test_not_eligible_plans_as_before(native, stride, K, reps, w):
    c = mk.case(stride)
    g, ms = setup_of(native, stride)
    pick = np.arange(mk.NQ * reps)[:57 if reps > 1 else mk.NQ] % mk.NQ
    assert reps == 1 or len(pick) * w == 513
    got, st = search(g, 1, c.qs[pick], K, ms, mk.MASK_OF_QUERY[pick], w=w)
    assert st["last_qg"] != -3, st
    assert mk.same_answer(got, tuple(x[pick] for x in model_of(stride, K, w))), "the model"


def test_setter_refusals(native):
    from ivfadc_jl_amd import _native as nat
    g, _ = setup_of(native, "u8_m8")
    assert nat.lib().ivfadc_set_masked_latency(None, 1) == nat.ERR_INVALID
    refuses(lambda: g.set_masked_latency(2), nat.ERR_INVALID, "mode")
    g.set_masked_latency(1)
    v = g.clone_view()                                    # the view starts from the index's setting
    g.set_masked_latency(0)
    c = mk.case("u8_m8")
    _, ms = setup_of(native, "u8_m8")
    v.search_masked_raw(c.qs, 10, ms, mk.MASK_OF_QUERY, w=1)
    assert v.get_stats()["last_qg"] == -3
