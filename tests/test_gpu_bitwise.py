"""UInt8 codes: every kernel form and every search entry returns the same bytes, on rounding-hostile inputs.

The counterpart of test_gpu_u16.py::test_every_search_entry_returns_the_same_bytes for the product's main path.  Inputs:
helpers.build_stress_index (uniform data, sub-spaces graded over 2^12 in both directions, sums dominated by the coarse distance, tiny
sums around exact hits); tests/test_parity_power.py shows on the CPU that each of them tells the reference's order of additions from every
restated mistake (a contracted multiply-add, a reversed / rotated / pairwise sum, dc added last, float64 tables, an expanded coarse
distance).  Every form is run on a shape it is instantiated for and must SAY that it ran (get_stats()): a silent fallback to another
kernel cannot pass.  Every result equals the oracle's under helpers.assert_same_results (counts, ids, distance bits), and all forms of
a shape agree with each other byte for byte over the first `count` slots."""
import ctypes as C

import numpy as np
import pytest

import helpers
from oracle import oracle as ora

pytestmark = pytest.mark.gpu


def gpu_index(native, oidx):
    return native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)


def _form(qg, chunk=0, table=None, coarse=None, prune=None, **expect):
    return dict(qg=qg, chunk=chunk, table=table, coarse=coarse, prune=prune, expect=expect)


def _list_major(filtered_at_4):
    """List-major with 1 / 2 / 4 queries per code stream, reference-order tables (mode 1) and the automatic tables (mode 0: the filter
    forms -- striped tables at m = 16, the 16-bit integer filter at m = 8 -- exist for four queries per stream)."""
    out = {}
    for qg in (1, 2, 4):
        out["list-major qg=%d reference tables" % qg] = _form(qg, 4096, table=1, last_qg=qg, last_striped=0, last_nf=0)
        out["list-major qg=%d automatic tables" % qg] = _form(qg, 4096, table=0, last_qg=qg, last_nf=0,
                                                               last_striped=1 if (qg == 4 and filtered_at_4) else 0)
    out["list-major qg=4 pruning off"] = _form(4, 0, table=0, prune=0, last_qg=4, last_striped=1 if filtered_at_4 else 0, pruned_points=0)
    return out


COMMON = {
    "query-major": _form(-1, last_qg=0, last_lb=0),
    "query-major, stand-alone top-w": _form(-3, last_qg=0, last_lb=0),
    "query-major pruning off": _form(-1, prune=0, last_qg=0, pruned_points=0),
    "small-batch single launch": _form(0, last_qg=-3),
    "generic (forced)": _form(-2, last_qg=-2),
}

FORMS = {
    "m8": dict(COMMON, **_list_major(True), **{
        "eight-wave, four queries": _form(4, 0, table=6, last_qg=4, last_striped=2),
        "eight-wave, eight queries": _form(4, 0, table=7, last_qg=8, last_striped=3),
        "eight-wave, several chunks": _form(4, 2048, table=6, last_qg=4, last_striped=2),
        "narrow-field": _form(8, 0, last_qg=8, last_nf=1),
        "narrow-field, several chunks": _form(8, 1024, last_qg=8, last_nf=1),
    }),
    "m16": dict(COMMON, **_list_major(True), **{
        "query-major reference tables": _form(-1, table=1, last_qg=0, last_lb=0),
        "lower-bound tables mode 2": _form(-1, table=2, last_qg=0, last_lb=1, lb=True),
        "lower-bound tables mode 2, stand-alone top-w": _form(-3, table=2, last_qg=0, last_lb=1, lb=True),
        "table mode 3 (automatic: no lower-bound rounds at m = 16)": _form(-1, table=3, last_qg=0, last_lb=0),
        "lower-bound tables mode 4": _form(-1, table=4, last_qg=0, last_lb=1, lb=True),
        "lower-bound tables mode 4, stand-alone top-w": _form(-3, table=4, last_qg=0, last_lb=1, lb=True),
    }),
    "m48": {
        "query-major reference tables": _form(-1, table=1, last_qg=0, last_lb=0),
        "query-major reference tables pruning off": _form(-1, table=1, prune=0, last_qg=0, last_lb=0, pruned_points=0),
        "lower-bound tables automatic": _form(-1, table=0, last_qg=0, last_lb=1, lb=True),
        "lower-bound tables mode 2, stand-alone top-w": _form(-3, table=2, last_qg=0, last_lb=1, lb=True),
        "lower-bound tables mode 3": _form(-1, table=3, last_qg=0, last_lb=1, lb=True),
        "lower-bound tables mode 3, stand-alone top-w": _form(-3, table=3, last_qg=0, last_lb=1, lb=True),
        "lower-bound tables mode 4": _form(-1, table=4, last_qg=0, last_lb=1, lb=True),
        "list-major qg=1": _form(1, 0, table=1, last_qg=1),
        "list-major qg=2": _form(2, 0, table=0, last_qg=2),      # (four queries' tables of m = 48 do not fit the LDS)
        "small-batch single launch": _form(0, last_qg=-3),
        "generic (forced)": _form(-2, last_qg=-2),
    },
    "m10": dict(COMMON, **_list_major(False)),
}


def _run(native, oidx, qs, K, w, name, f):
    g = gpu_index(native, oidx)
    g.set_tuning(f["qg"], f["chunk"])
    if f["table"] is not None:
        g.set_table_mode(f["table"])
    if f["coarse"] is not None:
        g.set_coarse_mode(f["coarse"])
    if f["prune"] is not None:
        g.set_pruning(f["prune"])
    g.reset_stats()
    got = g.search_raw(qs, K, w)
    st = g.get_stats()
    for key, val in f["expect"].items():
        if key == "lb":
            assert st["lb_survivors"] > 0, (name, st)
        else:
            assert st[key] == val, "%s did not run as the form it names: %s = %s, expected %s (%s)" % (name, key, st[key], val, st)
    return got


def _same_bytes(a, b, what):
    """counts identical; ids and distance bits identical over the first `count` slots (what lies behind them is unspecified)."""
    assert np.array_equal(a[2], b[2]), what + ": counts differ"
    valid = np.arange(a[0].shape[1])[None, :] < a[2][:, None]
    assert np.array_equal(a[0][valid], b[0][valid]), what + ": ids differ"
    assert np.array_equal(a[1][valid].view(np.uint32), b[1][valid].view(np.uint32)), what + ": distance bits differ"


@pytest.mark.parametrize("shape", sorted(FORMS))
@pytest.mark.parametrize("kind", helpers.STRESS_KINDS)
def test_every_scan_form_returns_the_oracles_bytes(native, kind, shape):
    seed, n, d, kc, m, ksub, K, w = helpers.BITWISE_SHAPES[shape]
    oidx, qs = helpers.build_stress_index(kind, seed, n, d, kc, m, ksub, nq=64, label_perm=(shape == "m10"))
    exp = oidx.knn_search(qs, K, w, nthreads=ora.max_threads())
    assert (exp[2] == K).all()
    first = None
    for name, f in FORMS[shape].items():
        what = "%s / %s / %s" % (kind, shape, name)
        got = _run(native, oidx, qs, K, w, what, f)
        helpers.assert_same_results(got, exp, what=what)
        if first is None:
            first = got
        _same_bytes(got, first, what + " against " + next(iter(FORMS[shape])))
    # K beyond the selection kernels: the generic path on its own; its first K slots are the K-neighbour search's
    big = 2500
    g = gpu_index(native, oidx)
    gen = g.search_raw(qs[:8], big, w)
    assert g.get_stats()["last_qg"] == -2
    helpers.assert_same_results(gen, oidx.knn_search(qs[:8], big, w), what="%s / %s / generic K=%d" % (kind, shape, big))
    assert (gen[2] >= K).all()
    _same_bytes((gen[0][:, :K], gen[1][:, :K], np.minimum(gen[2], K)), tuple(a[:8] for a in first), "generic K=%d, first %d slots" % (big, K))


# coarse mode -> what the statistics must say on the kc = 2048 shape with 8192 queries (coarse_mfma, coarse_f16, last_twolevel) and
# whether the stand-alone top-w reads per-tile records instead of a score matrix (coarse_listed; list-major plan only)
COARSE = {
    1: (0, 0, 0, False),      # exact VALU kernel
    2: (1, 1, 0, True),       # the matrix-core filter from kc >= 128 on: one f16 product per score
    3: (1, 0, 0, False),      # f32 MFMA filter
    4: (1, 1, 0, False),      # always the full score matrix
    8: (1, 0, 0, True),       # three-product bf16 split
    6: (0, 0, 1, False),      # two-level search
}


@pytest.mark.parametrize("kind", helpers.STRESS_KINDS)
def test_every_coarse_form_returns_the_oracles_bytes(native, kind):
    """Coarse modes 1, 2, 3, 4, 8 and 6 on a quantizer and a batch large enough for each (kc = 2048, 8192 queries: the split-operand
    filters need that many tiles, the per-tile records a stand-alone top-w with one wave per query), under the query-major and the
    list-major plan, with pruning on and off."""
    seed, n, d, kc, m, ksub, K, w = helpers.BITWISE_SHAPES["kc2048"]
    w = 8
    nq = 8192
    oidx, qs = helpers.build_stress_index(kind, seed, n, d, kc, m, ksub, nq=nq)
    exp = oidx.knn_search(qs, K, w, nthreads=ora.max_threads())
    first = None
    for mode, (mfma, f16, twolevel, listed) in COARSE.items():
        for plan in (-1, 4):
            for prune in (1, 0):
                what = "%s / coarse mode %d / plan %d / pruning %d" % (kind, mode, plan, prune)
                expect = dict(coarse_mfma=mfma, coarse_f16=f16, last_twolevel=twolevel, last_qg=0 if plan == -1 else 4,
                              coarse_listed=1 if (listed and plan == 4) else 0)
                if not prune:
                    expect["pruned_points"] = 0
                got = _run(native, oidx, qs, K, w, what, _form(plan, coarse=mode, prune=prune, **expect))
                helpers.assert_same_results(got, exp, what=what)
                if first is None:
                    first = got
                _same_bytes(got, first, what + " against the exact kernel")


@pytest.mark.parametrize("kind", helpers.STRESS_KINDS)
def test_every_search_entry_returns_the_oracles_bytes(native, kind):
    """ivfadc_search with memory the library does not know and with registered memory, ivfadc_search_device, ivfadc_search_batches (each
    batch names its successor: the next-batch hint), a view, ivfadc_mg_search on one device, and partial searches + ivfadc_merge_partials
    with two parts played by one handle."""
    import torch
    from ivfadc_jl_amd import _native as nat
    seed, n, d, kc, m, ksub, K, w = helpers.BITWISE_SHAPES["m8"]
    nq = 264
    oidx, qs = helpers.build_stress_index(kind, seed, n, d, kc, m, ksub, nq=nq)
    exp = oidx.knn_search(qs, K, w, nthreads=ora.max_threads())
    g = gpu_index(native, oidx)
    res = {}
    # memory the library does not know
    res["ivfadc_search, pageable"] = g.search_raw(qs, K, w)
    # registered memory: queries read in place, results written into the caller's arrays
    blocks = (qs.copy(), np.zeros((nq, K), np.uint32), np.zeros((nq, K), np.float32), np.zeros(nq, np.int32))
    for a in blocks:
        nat.host_register(a)
    try:
        nat.check(nat.lib().ivfadc_search(g._h, nq, nat.ptr(blocks[0], C.c_float), K, w, nat.ptr(blocks[1], C.c_uint32),
                                          nat.ptr(blocks[2], C.c_float), nat.ptr(blocks[3], C.c_int32)))
        res["ivfadc_search, registered"] = tuple(a.copy() for a in blocks[1:])
    finally:
        for a in blocks:
            nat.host_unregister(a)
    # device pointers
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(qs).to(dev)

    def outputs():
        o = (torch.zeros(nq * K, dtype=torch.int32, device=dev), torch.zeros(nq * K, dtype=torch.float32, device=dev),
             torch.zeros(nq, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()       # (torch fills the outputs on ITS stream: finished before the library's stream writes into them)
        return o

    def host(o):
        torch.cuda.synchronize()
        return o[0].cpu().numpy().view(np.uint32).reshape(nq, K), o[1].cpu().numpy().reshape(nq, K), o[2].cpu().numpy()

    o = outputs()
    g.search_device(nq, qd.data_ptr(), K, w, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
    g.sync()
    res["ivfadc_search_device"] = host(o)
    # a run of batches, query-major: every batch after the first starts from coarse rows that rode behind its predecessor's scan
    gb = gpu_index(native, oidx)
    gb.set_tuning(-1, 0)
    parts = gb.search_batches_raw([qs[:100], qs[100:200], qs[200:]], K, w)
    st = gb.get_stats()
    assert st["coarse_prefetched"] == 1 and st["last_rider"] == 0, st
    res["ivfadc_search_batches"] = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
    # a view
    v = g.clone_view()
    res["clone_view"] = v.search_raw(qs, K, w)
    # the multi-device front end on one device
    L = nat.lib()
    mg = C.c_void_p()
    devs = np.array([0], np.int32)
    nat.check(L.ivfadc_mg_create(C.byref(mg), 1, nat.ptr(devs, C.c_int32), d, kc, m, ksub, nat.ptr(oidx.centroids, C.c_float),
                                 nat.ptr(oidx.codebooks, C.c_float), nat.ptr(oidx.labels, C.c_uint8)))
    try:
        nat.check(L.ivfadc_mg_set_lists(mg, nat.ptr(oidx.offsets, C.c_int64), nat.ptr(oidx.codes, C.c_uint8), nat.ptr(oidx.ids, C.c_uint32)))
        ids = np.zeros((nq, K), np.uint32); dists = np.zeros((nq, K), np.float32); counts = np.zeros(nq, np.int32)
        nat.check(L.ivfadc_mg_search(mg, nq, nat.ptr(qs, C.c_float), K, w, nat.ptr(ids, C.c_uint32), nat.ptr(dists, C.c_float),
                                     nat.ptr(counts, C.c_int32)))
        res["ivfadc_mg_search"] = (ids, dists, counts)
    finally:
        L.ivfadc_mg_destroy(mg)
    # list-partitioned: the handle plays both ranks in turn, then the merge
    gp = gpu_index(native, oidx)
    keys_all = torch.zeros((2, nq, K), dtype=torch.int64, device=dev)
    cnts_all = torch.zeros((2, nq), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for part in range(2):
        gp.set_list_partition(2, part)
        gp.search_device_partial(nq, qd.data_ptr(), K, w, keys_all[part].data_ptr(), cnts_all[part].data_ptr())
        torch.cuda.synchronize()
    o = outputs()
    gp.merge_partials_device(nq, K, 2, keys_all.data_ptr(), cnts_all.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
    gp.sync()
    res["partial searches + merge_partials"] = host(o)
    first = res["ivfadc_search, pageable"]
    for name, got in res.items():
        helpers.assert_same_results(got, exp, what="%s / %s" % (kind, name))
        _same_bytes(got, first, "%s / %s against ivfadc_search" % (kind, name))
