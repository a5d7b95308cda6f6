"""The coarse stage on the tables of tests/coarse_edges.py (the CPU side, with the premises and the mutants, is
tests/test_coarse_edges_model.py): the w-th cell where each certificate is weakest, compared at PROBE level.

Every comparison covers every row of the batch -- lists equal, distance bits identical, nothing sampled -- against the oracle's
coarse_search (hostile rows and the uniform filler alike; the filler is 1024 distinct queries repeated, so its reference is computed
once per table, coarse_edges.filler_of).  The h <= 16 hostile queries of a batch stand in four blocks of it: from row 0, up to row 127,
from the first row of the last, ragged 128-row tile, up to the last row -- every hostile query within h rows of each of the four
anchors, ONE of them on the anchor row itself; the blocks are rotated from call to call, so which one changes.

a. coarse_search_raw in every form the entry reaches, named beforehand and confirmed through get_stats(); on the pool-edge family the
   score-matrix readers' coarse_fallbacks EQUAL the number of rows with t >= P near-ties, and are 0 on a batch of t <= P - 1 rows and
   filler; every mode returns the bytes of mode 1.
b. a revealing index -- one stored point per cell, id = cell, K = w: the ids of a search ARE its probe set -- under the fused top-w
   (set_tuning(-1, 0)), the stand-alone one (-3) and the small-batch launch with the coarse search inside (coarse mode 5), pruning on
   and off, against the oracle's knn_search: the pool table in every score form, and the gap (rounding ties included), records, big-norm
   and 127 / 128 / 129-tile tables under -1 and under -3 -- the latter at 8192 + 37 queries, where the records' reader runs.
c. the two-level search on the clump quantizers: every row, the group count, and -- single-query batches -- coarse_visited against the
   model's visit of the clumps.  Not known to be tested on the GPU: the break on `bound > threshold` against `>=`.  The model tells them
   apart only on the twins table, whose two overlapping groups are handed to it; the library puts the twins into one group.

Measured on an MI355X (printed by the tests): every score-matrix reader -- f32 in all three tile shapes, bf16 split, f16, stand-alone
(workgroup per query, wave per query, tile minima) and fused -- shows exactly the designed 12 fallbacks on a pool-edge batch (three
rows with t >= P, four copies each) at every w and 0 on the t <= P - 1 batch; the records show 0 on both.  In the gap sweep every
form falls back for k <= 1 (gap <= 2 eps) and passes from k = 2 on.  The library's grouping finds the 16 clumps: coarse_visited equals
the model's count on every row (and on the twins; with the stray cell, which it puts into the big clump, 130 against 129).

Each test prints its wall time."""
import time

import numpy as np
import pytest

import coarse_edges as ce
import helpers
from oracle import oracle as ora

pytestmark = pytest.mark.gpu
f32 = np.float32
FILL = 1024                  # distinct filler queries per table
CHUNK = 16                   # hostile queries per batch (four blocks of them must fit the 37 rows of the ragged tile twice)
NQ_WG, NQ_WAVE = 4096 + 37, 8192 + 37      # workgroup-per-query top-w below 8 x 256 x 4 queries, a wave per query from there on
NUM_CU = 256
_G, _REF = {}, {}


def bench(native, name):
    """the table as a revealing index on the device, and the oracle's copy of it: built once, settings put back by every test"""
    if name not in _G:
        tab = ce.table(name)
        rng = np.random.default_rng(5)
        m = 8
        cbs = ((rng.random((m, 256, tab.d // m), dtype=f32) - 0.5) * 0.5).astype(f32)
        labels = np.tile(np.arange(256, dtype=np.uint8), (m, 1))
        codes = rng.integers(0, 256, (tab.kc, m)).astype(np.uint8)
        oidx = ora.OracleIndex(tab.cent, cbs, labels, np.arange(tab.kc + 1, dtype=np.int64), codes, np.arange(tab.kc, dtype=np.uint32))
        _G[name] = (native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids), oidx)
    return _G[name]


def defaults(g):
    g.set_coarse_mode(0)
    g.set_tuning(0, 0)
    g.set_pruning(1)


def filler(tab, wmax):
    key = (tab.name, wmax)
    if key not in _REF:
        fq = ce.filler_of(tab, FILL)
        _REF[key] = (fq, ce.oracle_rows(tab.cent, fq, wmax))
    return _REF[key]


def batch(tab, nq, rows, wmax, turn=0):
    """(queries, expected lists, expected distances at wmax, positions of the hostile rows)"""
    fq, (fl, fd) = filler(tab, wmax)
    idx = np.arange(nq) % FILL
    if rows:
        qs, pos = ce.place(fq[idx], [r.q for r in rows], turn)
    else:
        qs, pos = fq[idx].copy(), []
    el, ed = fl[idx].copy(), fd[idx].copy()
    for r, p in zip(rows, pos):
        cl, dd = ce.top_of(ce.context(tab, r).O, wmax)
        el[p], ed[p] = cl, dd
    return qs, el, ed, pos


def chunks(rows):
    return [rows[i:i + CHUNK] for i in range(0, len(rows), CHUNK)]


def same_coarse(got, el, ed, w, what, names=None):
    assert got[0].shape == (el.shape[0], w) and got[0].dtype == np.int32 and got[1].dtype == f32, what
    bad = np.nonzero((got[0] != el[:, :w]).any(1) | (got[1].view(np.uint32) != ed[:, :w].view(np.uint32)).any(1))[0]
    if bad.size:
        r = int(bad[0])
        raise AssertionError("%s: %d of %d rows differ, first row %d (%s): lists %s vs %s, dists %s vs %s" % (
            what, bad.size, el.shape[0], r, (names or {}).get(r, "filler"), got[0][r], el[r, :w], got[1][r], ed[r, :w]))


def ran(g, expect, what):
    st = g.get_stats()
    for key, val in expect.items():
        assert st[key] == val, "%s did not run as the form it names: %s = %s, expected %s (%s)" % (what, key, st[key], val, st)
    return st


def names_of(rows, pos):
    return {p: r.name for r, ps in zip(rows, pos) for p in ps}


def expect_of(tab, mode, nq, w):
    """run_coarse / coarse_dev restated: the stats a stand-alone coarse search of this shape must show"""
    if mode == 1 or w > 48 or tab.kc < (128 if mode == 2 else 2048):
        return dict(coarse_mfma=0, last_twolevel=0)
    big128 = ((tab.kc + 127) // 128) * ((nq + 127) // 128) >= 2 * NUM_CU
    wpq4 = nq < 8 * NUM_CU * 4 and tab.kc >= 512
    bf16 = big128 and mode != 3
    f16 = bf16 and mode != 8
    listed = bf16 and not wpq4 and mode != 4 and (tab.kc + 63) // 64 >= 4 * w
    return dict(coarse_mfma=1, last_twolevel=0, coarse_f16=int(f16), coarse_listed=int(listed))


# ---- a. stand-alone selection -----------------------------------------------------------------------------------------------------------
def _a(name, table, mode, nq, ws, **expect):
    return pytest.param(dict(name=name, table=table, mode=mode, nq=nq, ws=ws, expect=expect), id=name)


STANDALONE = [
    _a("exact VALU kernels", "pool", 1, 300, ce.POOL_WS, coarse_mfma=0),
    _a("coarse_mfma_kernel<64,16>", "small", 2, 300, (1, 8), coarse_mfma=1, coarse_f16=0, coarse_listed=0),
    _a("coarse_mfma_kernel<64,64>", "small64", 2, 300, (1, 8), coarse_mfma=1, coarse_f16=0, coarse_listed=0),
    _a("coarse_mfma_kernel<128,16>, workgroup per query", "pool", 3, NQ_WG, ce.POOL_WS, coarse_mfma=1, coarse_f16=0, coarse_listed=0),
    _a("coarse_mfma_kernel<128,16>, tile minima", "pool", 3, NQ_WAVE, ce.POOL_WS, coarse_mfma=1, coarse_f16=0, coarse_listed=0),
    _a("bf16 split, workgroup per query", "pool", 8, NQ_WG, ce.POOL_WS, coarse_mfma=1, coarse_f16=0, coarse_listed=0),
    _a("bf16 split, wave per query (listed at w <= 8)", "pool", 8, NQ_WAVE, ce.POOL_WS, coarse_mfma=1, coarse_f16=0),
    _a("f16, workgroup per query", "pool", 0, NQ_WG, ce.POOL_WS, coarse_mfma=1, coarse_f16=1, coarse_listed=0),
    _a("f16, wave per query (listed at w <= 8)", "pool", 0, NQ_WAVE, ce.POOL_WS, coarse_mfma=1, coarse_f16=1),
    _a("f16 with the score matrix", "pool", 4, NQ_WAVE, ce.POOL_WS, coarse_mfma=1, coarse_f16=1, coarse_listed=0),
    _a("records: bf16 listed", "records", 8, NQ_WAVE, (1, 2, 8), coarse_mfma=1, coarse_f16=0, coarse_listed=1),
    _a("records: f16 listed", "records", 0, NQ_WAVE, (1, 2, 8), coarse_mfma=1, coarse_f16=1, coarse_listed=1),
    _a("records: f32 tile minima", "records", 3, NQ_WAVE, (1, 2, 8), coarse_mfma=1, coarse_f16=0, coarse_listed=0),
    _a("tiles: bf16 listed, kc = 8320", "tiles", 8, NQ_WAVE, (1, 8), coarse_mfma=1, coarse_f16=0, coarse_listed=1, last_twolevel=0),
    _a("tiles: f16 listed, kc = 8320", "tiles", 0, NQ_WAVE, (1, 8), coarse_mfma=1, coarse_f16=1, coarse_listed=1, last_twolevel=0),
    _a("gap: f32 tile minima", "gap", 3, NQ_WAVE, (1, 8), coarse_mfma=1, coarse_f16=0, coarse_listed=0),
    _a("gap: f16 score matrix, wave per query", "gap", 4, NQ_WAVE, (1, 8), coarse_mfma=1, coarse_f16=1, coarse_listed=0),
    _a("gap: bf16 listed", "gap", 8, NQ_WAVE, (1, 8), coarse_mfma=1, coarse_f16=0, coarse_listed=1),
    _a("gap: f16 listed", "gap", 0, NQ_WAVE, (1, 8), coarse_mfma=1, coarse_f16=1, coarse_listed=1),
    _a("big norm: f32", "norm", 3, NQ_WG, (1, 8, 48), coarse_mfma=1, coarse_f16=0),
    _a("big norm: bf16", "norm", 8, NQ_WAVE, (1, 8, 48), coarse_mfma=1, coarse_f16=0),
    _a("big norm: f16", "norm", 0, NQ_WAVE, (1, 8, 48), coarse_mfma=1, coarse_f16=1),
]


def _mode1(g, key, qs, w):
    """the bytes of mode 1 on this very batch, once"""
    if key not in _REF:
        g.set_coarse_mode(1)
        _REF[key] = g.coarse_search_raw(qs, w)
        assert g.get_stats()["coarse_mfma"] == 0
    return _REF[key]


@pytest.mark.parametrize("f", STANDALONE)
def test_stand_alone_selection(native, f):
    t0 = time.time()
    tab = ce.table(f["table"])
    g, _ = bench(native, f["table"])
    mode, nq = f["mode"], f["nq"]
    wmax = 48
    calls, record = 0, []
    try:
        for wi, w in enumerate(f["ws"]):
            mine = [r for r in tab.rows if w in r.ws]
            pool = [r for r in mine if r.meta["family"] == "pool"]
            passing = [r for r in pool if r.meta["t"] < r.meta["P"]]
            sets = [("pool edge", pool), ("pool edge, t <= P - 1 only", passing)] if pool else []
            sets += [("rows %d" % i, c) for i, c in enumerate(chunks([r for r in mine if r.meta["family"] != "pool"]))]
            for si, (tag, rows) in enumerate(sets):
                qs, el, ed, pos = batch(tab, nq, rows, wmax, turn=wi + si)
                what = "%s, %s, nq = %d, w = %d, %s" % (tab.name, f["name"], nq, w, tag)
                one = _mode1(g, ("mode 1", f["table"], nq, w, tag), qs, w)
                g.set_coarse_mode(mode)
                g.reset_stats()
                got = g.coarse_search_raw(qs, w)
                calls += 1
                exp = dict(expect_of(tab, mode, nq, w), **f["expect"])
                st = ran(g, exp, what)
                same_coarse(got, el, ed, w, what, names_of(rows, pos))
                assert np.array_equal(got[0], one[0]) and np.array_equal(got[1].view(np.uint32), one[1].view(np.uint32)), what + ": differs from mode 1"
                if tag.startswith("pool edge"):
                    designed = 4 * sum(1 for r in rows if r.meta["t"] >= r.meta["P"])
                    record.append("w=%d %s: coarse_fallbacks %d, designed %d%s" % (w, tag, st["coarse_fallbacks"], designed,
                                                                                " (listed: not asserted)" if st["coarse_listed"] else ""))
                    if st["coarse_mfma"] and not st["coarse_listed"]:       # the score-matrix readers: the premise decides
                        assert st["coarse_fallbacks"] == designed, "%s: coarse_fallbacks = %d, designed %d" % (what, st["coarse_fallbacks"], designed)
                    if not st["coarse_mfma"]:
                        assert st["coarse_fallbacks"] == 0, what
    finally:
        defaults(g)
    print("\n%s on %s: %d searches of %d queries, %.2f s\n  %s" % (f["name"], tab.name, calls, nq, time.time() - t0, "\n  ".join(record)))


GAP_FORMS = [("f32", 3), ("bf16", 8), ("f16", 4)]


@pytest.mark.parametrize("form,mode", GAP_FORMS)
def test_gap_sweep_records_where_each_form_begins_to_fall_back(native, form, mode):
    """One batch per gap row -- the row's four copies among the filler -- through the score-matrix reader of the row's own form: the result
    is exact on both sides of the certificate; whether the row passed (0 fallbacks) or fell back (4) is printed, not asserted."""
    t0 = time.time()
    tab = ce.table("gap")
    g, _ = bench(native, "gap")
    seen = []
    try:
        g.set_coarse_mode(mode)
        qs, el, ed, _ = batch(tab, NQ_WG, [], 48)
        g.reset_stats()
        same_coarse(g.coarse_search_raw(qs, 8), el, ed, 8, "filler alone")
        base = ran(g, dict(coarse_mfma=1, coarse_f16=int(form == "f16"), coarse_listed=0), "filler alone")["coarse_fallbacks"]
        for row in tab.rows:
            if row.meta["family"] != "gap" or row.meta.get("form", form) != form:
                continue
            qs, el, ed, pos = batch(tab, NQ_WG, [row], 48, turn=0)
            g.reset_stats()
            got = g.coarse_search_raw(qs, 8)
            st = ran(g, dict(coarse_mfma=1, coarse_f16=int(form == "f16"), coarse_listed=0), row.name)
            same_coarse(got, el, ed, 8, "%s through the %s form" % (row.name, form), names_of([row], pos))
            seen.append((row.name, st["coarse_fallbacks"] - base))
            assert 0 <= st["coarse_fallbacks"] - base <= 4, (row.name, st["coarse_fallbacks"], base)
    finally:
        defaults(g)
    print("\ngap sweep, %s form (filler alone: %d fallbacks), %.2f s: %s" % (form, base, time.time() - t0, ", ".join("%s -> %d" % s for s in seen)))


# ---- b. fused and in-launch selection ---------------------------------------------------------------------------------------------------
def _b(name, table, tuning, mode, nq, ws, **expect):
    return pytest.param(dict(name=name, table=table, tuning=tuning, mode=mode, nq=nq, ws=ws, expect=expect), id=name)


FUSED = [
    _b("fused top-w, f32 64-wide tiles", "pool", -1, 0, 300, ce.POOL_WS, last_qg=0, coarse_mfma=1, coarse_f16=0),
    _b("fused top-w, f16", "pool", -1, 0, NQ_WG, ce.POOL_WS, last_qg=0, coarse_mfma=1, coarse_f16=1),
    _b("fused top-w, bf16 split", "pool", -1, 8, NQ_WG, ce.POOL_WS, last_qg=0, coarse_mfma=1, coarse_f16=0),
    _b("fused top-w, f32 128-wide tiles", "pool", -1, 3, NQ_WG, ce.POOL_WS, last_qg=0, coarse_mfma=1, coarse_f16=0),
    _b("fused top-w, exact", "pool", -1, 1, 300, ce.POOL_WS, last_qg=0, coarse_mfma=0),
    _b("stand-alone top-w behind the query-major scan", "pool", -3, 0, NQ_WG, ce.POOL_WS, last_qg=0, coarse_mfma=1, coarse_f16=1),
    _b("gap: fused top-w, f16", "gap", -1, 0, NQ_WG, (1, 8), last_qg=0, coarse_mfma=1, coarse_f16=1, coarse_listed=0),
    _b("gap: fused top-w, bf16 split", "gap", -1, 8, NQ_WG, (1, 8), last_qg=0, coarse_mfma=1, coarse_f16=0, coarse_listed=0),
    _b("gap: stand-alone top-w, f16 listed", "gap", -3, 0, NQ_WAVE, (1, 8), last_qg=0, coarse_mfma=1, coarse_f16=1, coarse_listed=1),
    _b("gap: stand-alone top-w, bf16 listed", "gap", -3, 8, NQ_WAVE, (1, 8), last_qg=0, coarse_mfma=1, coarse_f16=0, coarse_listed=1),
    _b("records: fused top-w, f16", "records", -1, 0, NQ_WG, (1, 2, 8), last_qg=0, coarse_mfma=1, coarse_f16=1, coarse_listed=0),
    _b("records: stand-alone top-w, f16 listed", "records", -3, 0, NQ_WAVE, (1, 2, 8), last_qg=0, coarse_mfma=1, coarse_f16=1, coarse_listed=1),
    _b("records: stand-alone top-w, bf16 listed", "records", -3, 8, NQ_WAVE, (1, 2, 8), last_qg=0, coarse_mfma=1, coarse_f16=0, coarse_listed=1),
    _b("big norm: fused top-w, f16", "norm", -1, 0, NQ_WG, (1, 8, 48), last_qg=0, coarse_mfma=1, coarse_f16=1),
    _b("big norm: stand-alone top-w, f16", "norm", -3, 0, NQ_WG, (1, 8, 48), last_qg=0, coarse_mfma=1, coarse_f16=1),
    _b("tiles: query-major scan at kc = 8320 (top-w stand-alone), f16", "tiles", -1, 0, NQ_WG, (1, 8), last_qg=0, coarse_mfma=1, coarse_f16=1, last_twolevel=0),
    _b("tiles: stand-alone top-w, f16 listed", "tiles", -3, 0, NQ_WAVE, (1, 8), last_qg=0, coarse_mfma=1, coarse_f16=1, coarse_listed=1, last_twolevel=0),
    _b("small-batch launch, coarse search inside", "small", 0, 5, 48, (1, 8), last_qg=-3, coarse_mfma=0),
    _b("small-batch launch, coarse search inside, d = 64", "small64", 0, 5, 48, (1, 8), last_qg=-3, coarse_mfma=0),
]


@pytest.mark.parametrize("prune", [1, 0])
@pytest.mark.parametrize("f", FUSED)
def test_fused_and_in_launch_selection(native, f, prune):
    t0 = time.time()
    tab = ce.table(f["table"])
    g, oidx = bench(native, f["table"])
    nq = f["nq"]
    calls, record = 0, []
    try:
        g.set_tuning(f["tuning"], 0)
        g.set_coarse_mode(f["mode"])
        g.set_pruning(prune)
        for wi, w in enumerate(f["ws"]):
            mine = [r for r in tab.rows if w in r.ws]
            pool = [r for r in mine if r.meta["family"] == "pool"]
            rest = [r for r in mine if r.meta["family"] != "pool"]
            if nq <= 64:       # the small-batch launch serves nq w <= 512
                sets = [("rows %d" % i, c) for i, c in enumerate(chunks(pool + rest))]
            else:
                sets = ([("pool edge", pool)] if pool else []) + [("rows %d" % i, c) for i, c in enumerate(chunks(rest))]
            for si, (tag, rows) in enumerate(sets):
                qs, el, _, pos = batch(tab, nq, rows, 48, turn=wi + si)
                what = "%s, %s, pruning %d, nq = %d, w = %d, %s" % (tab.name, f["name"], prune, nq, w, tag)
                key = ("knn", f["table"], nq, w, tag, wi + si)
                if key not in _REF:
                    _REF[key] = oidx.knn_search(qs, w, w, nthreads=ora.max_threads())
                g.reset_stats()
                got = g.search_raw(qs, w, w)
                calls += 1
                st = ran(g, f["expect"], what)
                if not prune and f["expect"]["last_qg"] == 0:
                    assert st["pruned_points"] == 0, (what, st)
                helpers.assert_same_results(got, _REF[key], what=what)
                # one point per cell, id = cell, K = w: the ids ARE the probe set
                assert (got[2] == w).all() and np.array_equal(np.sort(got[0].astype(np.int64), 1), np.sort(el[:, :w].astype(np.int64), 1)), what
                if tag == "pool edge" and st["coarse_mfma"]:
                    designed = 4 * sum(1 for r in rows if r.meta["t"] >= r.meta["P"])
                    record.append("w=%d: coarse_fallbacks %d, designed %d" % (w, st["coarse_fallbacks"], designed))
                    assert st["coarse_fallbacks"] == designed, "%s: coarse_fallbacks = %d, designed %d" % (what, st["coarse_fallbacks"], designed)
    finally:
        defaults(g)
    print("\n%s, pruning %d: %d searches of %d queries, %.2f s%s" % (f["name"], prune, calls, nq, time.time() - t0,
                                                                    "".join("\n  " + r for r in record)))


# ---- c. two-level -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["clumps", "twins", "stray"])
def test_two_level_on_the_clumps(native, name):
    t0 = time.time()
    tab = ce.table(name)
    g, _ = bench(native, name)
    nq = 128 + 37
    seen = []
    try:
        g.set_coarse_mode(6)
        for wi, w in enumerate((1, 2, 8, 64, 65)):
            rows = [r for r in tab.rows if w in r.ws]
            qs, el, ed, pos = batch(tab, nq, rows[:CHUNK], 65, turn=wi)
            g.reset_stats()
            got = g.coarse_search_raw(qs, w)
            what = "%s, two-level, w = %d" % (tab.name, w)
            st = ran(g, dict(last_twolevel=int(w <= 64), coarse_mfma=0), what)
            assert st["twolevel_groups"] >= len(ce.CLUMPS), (what, st)
            same_coarse(got, el, ed, w, what, names_of(rows[:CHUNK], pos))
            # single-query batches: the exact distances computed = the members of the clumps the model visits.  (A stand-alone coarse
            # search sends its counters to the sink: the count is read from a search of the revealing index, query-major, K = w.)
            for row in rows:
                if w > 64:
                    continue
                g.set_tuning(-1, 0)
                g.reset_stats()
                ids, _, cnt = g.search_raw(row.q[None, :], w, w)
                g.set_tuning(0, 0)
                cl, _ = ce.top_of(ce.context(tab, row).O, w)
                assert cnt[0] == w and np.array_equal(np.sort(ids[0].astype(np.int64)), np.sort(cl.astype(np.int64))), (what, row)
                st1 = ran(g, dict(last_twolevel=1, last_qg=0), "%s, single query" % what)
                seen.append((row.name, w, st1["coarse_visited"], ce.run(tab, row, w, "twolevel", "exact")[2]))
        print("\n%s: %d groups; (row, w, coarse_visited, the model's)\n  %s" % (tab.name, st["twolevel_groups"], "\n  ".join(map(str, seen))))
        for rn, w, visited, model in seen:
            assert 0 < visited < tab.kc, (rn, w, visited)
            if name == "clumps":       # (twins / stray hand the model a grouping the library cannot be expected to find)
                assert visited == model, "%s, w = %d: coarse_visited %d, the model's visit of the clumps %d" % (rn, w, visited, model)
    finally:
        defaults(g)
    print("%s: %.2f s" % (tab.name, time.time() - t0))


def test_two_level_after_64_groups(native):
    """Unstructured N(0, 1) centroids, kc = 4160: more than 64 groups, no bound closes, and at w = 64 every query looks at more than
    64 x 64 centroids -- the branch behind the 64 best groups ran."""
    t0 = time.time()
    tab = ce.table("normal")
    g, _ = bench(native, "normal")
    rng = np.random.default_rng(21)
    qs = rng.standard_normal((64 + 37, tab.d)).astype(f32)
    qs[:3] = [r.q for r in tab.rows]
    qs[-3:] = [r.q for r in tab.rows]
    try:
        g.set_coarse_mode(6)
        for w in (1, 8, 64):
            exp = ce.oracle_rows(tab.cent, qs, w)
            g.reset_stats()
            got = g.coarse_search_raw(qs, w)
            st = ran(g, dict(last_twolevel=1, coarse_mfma=0), "normal, w = %d" % w)
            same_coarse(got, exp[0], exp[1], w, "normal, two-level, w = %d" % w)
            print("\nnormal kc = %d, w = %d: %d groups, %.1f centroids visited per query" % (tab.kc, w, st["twolevel_groups"], st["coarse_visited"] / qs.shape[0]))
            assert st["twolevel_groups"] > 64, st
        # (a stand-alone coarse search sends its counters to the sink: the count is read from a query-major search, K = w = 64)
        g.set_tuning(-1, 0)
        g.reset_stats()
        ids, _, cnt = g.search_raw(qs, 64, 64)
        st = ran(g, dict(last_twolevel=1, last_qg=0), "normal, search, w = 64")
        assert (cnt == 64).all() and np.array_equal(np.sort(ids.astype(np.int64), 1), np.sort(exp[0].astype(np.int64), 1))
        print("normal kc = %d, search at w = 64: %.1f centroids visited per query" % (tab.kc, st["coarse_visited"] / qs.shape[0]))
        assert st["coarse_visited"] > 64 * 64 * qs.shape[0], st
        for r in (0, 1, 2, 50, qs.shape[0] - 1):       # ... and per query: single-query searches
            g.reset_stats()
            ids, _, cnt = g.search_raw(qs[r:r + 1], 64, 64)
            st = ran(g, dict(last_twolevel=1, last_qg=0), "normal, single query %d" % r)
            assert cnt[0] == 64 and np.array_equal(np.sort(ids[0].astype(np.int64)), np.sort(exp[0][r].astype(np.int64))), r
            assert st["coarse_visited"] > 64 * 64, (r, st)
    finally:
        defaults(g)
    print("normal: %.2f s" % (time.time() - t0))
