"""Every scan form on lists whose rank by position is prescribed (tests/placement.py; the CPU side is tests/test_placement_model.py).

Every scan kernel prunes with a bound whose proof counts over its own work decomposition, and with codes drawn at random the K best
points are spread evenly over waves, steps, chunks and lanes -- the one arrangement in which such a bound cannot fail.  On
placement.placed_case the winners of every list stand where a placement says: ascending, descending, all in one wave / step / chunk
(first, middle, last), one per granule, all in one lane, split between the ends, behind their near misses, tied across the K boundary,
and shuffled as a control; lists of 6203 and of 299 points, eight queries per list, w = 3.  One handle per kind, never mutated.

Every form of tests/test_gpu_sequences.py as tests/test_gpu_list_end.py arranges them (the forced chunks 1024 / 2048 and the matrix-core
lower-bound rounds of m16_d96 included), the masked scan with an all-ones mask and with a mask that keeps exactly the winners and their
near misses, and a subset view of every second stored id search ALL queries.  Every search names its form beforehand and asserts it
through get_stats(); every result is compared exactly (counts, ids, distance bits) with the reference.  A failure names the
placement, the list length, K and the form.

A test is one (kind, K slot): slot i runs the register-selector and eight-wave forms at placement.K_REG[i], slots 0 .. 5 the wide pool
at K_WIDE[i] as well, slots 6 .. 10 the LDS selectors at K_LDS[i - 6].  Form count and wall time per test are printed."""
import time

import numpy as np
import pytest

import helpers
import list_end as le
import masked as mk
import placement as pl
import sequences as sq
import subset as sb
import write_path as wp
from oracle import oracle as ora
from test_gpu_list_end import settings_of
from test_gpu_sequences import apply, ran

pytestmark = pytest.mark.gpu
SMALL_BATCH = 64             # the single-launch form serves up to 64 queries: it runs in slices
VIEW_FORMS = 3               # forms the subset view runs per slot, dealt in turn from the kind's table


def k_of(kind, f, slot):
    """The K a form of settings_of runs in this slot, or None: forms the table lists at K > 64 take the wide pool's K (m = 8 under
    table modes 8 / 9) or the LDS selectors'."""
    d, m, ksub, bits = pl.KINDS[kind]
    if f["K"] <= 64:
        return pl.K_REG[slot]
    if bits == 8 and m == 8 and f["table"] in (8, 9):
        return pl.K_WIDE[slot] if slot < len(pl.K_WIDE) else None
    return lds_k(slot)


def lds_k(slot):
    """the LDS selectors' K of a slot: the slots behind the wide pool's"""
    i = slot - len(pl.K_WIDE)
    return pl.K_LDS[i] if 0 <= i < len(pl.K_LDS) else None


def forms_of(kind, slot, n, kc, nq_all):
    """test_gpu_list_end.forms_of on this file's shape and K values: each search with the stats it must show, from
    sequences.expected_form -- the plan's rules restated --; what that leaves open (last_lb, pruned_points) from the imported form."""
    d, m, ksub, bits = pl.KINDS[kind]
    shape = dict(m=m, dsub=d // m, ksub=ksub, kc=kc, n=n, u16=bits == 16)
    out = []
    for f in settings_of(kind):
        K = k_of(kind, f, slot)
        if K is None:
            continue
        nq = SMALL_BATCH if f["qg"] == 0 and not shape["u16"] else nq_all
        exp = sq.expected_form(shape, dict(table=f["table"], qg=f["qg"]), K, pl.W, nq)
        assert exp is not None, f["name"]
        exp = dict(exp)
        for key in ("last_lb", "pruned_points"):
            if key in f["expect"]:
                exp[key] = f["expect"][key]
        if f["chunk"]:
            exp["last_chunk"] = f["chunk"]
        if exp.get("last_striped") in (2, 3):
            exp["lds_max"] = 80 * 1024
        out.append(dict(f, K=K, w=pl.W, nq=nq, expect=exp))
    return out


def check(case, got, exp, q0, what):
    """Exact comparison; a failure names the first differing query's placement and list length."""
    r = le.first_difference(got, exp)
    if r is None:
        return
    try:
        helpers.assert_same_results(le.part(got, slice(r, r + 1)), le.part(exp, slice(r, r + 1)))
        detail = "?"
    except AssertionError as e:
        detail = str(e)
    raise AssertionError("%s: first differing %s: %s" % (what, case.what(q0 + r), detail))


class Lists:
    """A reference over lists with the case's quantizers: the C oracle (8-bit) or placement.Sorted (UInt16), per K, computed once."""

    def __init__(self, case, lists=None):
        self.case = case
        self.ref = case.ref if lists is None else case.with_lists(*lists)
        self.n = int(self.ref.offsets[-1])
        self.cache = {}
        self.sorted = pl.Sorted(case, self.ref) if case.u16 else None

    def expected(self, K):
        if K not in self.cache:
            if self.case.u16:
                self.cache[K] = self.sorted.top(K)
            else:
                self.cache[K] = self.ref.knn_search(self.case.qs, K, pl.W, nthreads=ora.max_threads())
        return self.cache[K]


class Bench:
    """One kind's handle, its mask set and subset view, and the references of all three."""

    def __init__(self, native, kind):
        self.kind, self.case = kind, pl.placed_case(kind)
        case = self.case
        self.nq = case.qs.shape[0]
        self.kc = len(case.lists)
        self.g = wp.gpu_handle(native, case.ref)
        self.g.search_raw(case.qs[-1:], 1, 1)
        self.whole = Lists(case)
        lists = wp.lists_of(case.ref)
        self.masks = [np.ones(int(case.ref.ids.max()) + 1, bool), pl.winners_mask(case)]
        self.ms = self.g.maskset(masks=self.masks)
        kept = 256 * self.kc
        assert list(self.ms.kept) == [self.whole.n, kept], (self.ms.kept, kept)
        self.winners = Lists(case, sb.filtered_lists(*lists, self.masks[1]))
        half = pl.every_second_id(case)
        self.view = self.g.subset(mask=half)
        self.halved = Lists(case, sb.filtered_lists(*lists, half))
        assert len(self.view) == self.halved.n
        assert np.array_equal(self.view.list_sizes(), np.diff(self.halved.ref.offsets))

    def search_form(self, h, f, lists, what, plain=True):
        """one form on handle h (the index or the view), in slices where the form serves 64 queries; returns the searches made"""
        case = self.case
        if plain:
            apply(h, f, case.u16)
        else:       # a view: the settings are its own; it takes no list partition
            h.set_tuning(f["qg"], f["chunk"])
            h.set_table_mode(f["table"])
            h.set_pruning(f["prune"])
            h.set_workspace_limit(f["ws"])
        exp = lists.expected(f["K"])
        made = 0
        for q0 in range(0, self.nq, f["nq"]):
            sl = slice(q0, min(self.nq, q0 + f["nq"]))
            where = "%s, queries %d..%d" % (what, sl.start, sl.stop - 1)
            if "pruned_points" in f["expect"]:
                h.reset_stats()
            got = h.search_raw(case.qs[sl], f["K"], pl.W)
            made += 1
            ran(h, f["expect"], where)
            check(case, got, le.part(exp, sl), q0, where)
        return made

    def masked(self, K, widths, searches):
        """the masked scan (8-bit: the masked kernel at one and at four queries per stream, chunk 1024; UInt16: the masked generic
        path) under the all-ones mask and under the mask that keeps the winners and their near misses"""
        case, g = self.case, self.g
        g.set_table_mode(0)
        g.set_pruning(1)
        g.set_workspace_limit(sq.WS_DEFAULT)
        for qg in ((0,) if case.u16 else widths):
            g.set_tuning(qg, 1024 if qg else 0)
            try:
                for r, lists in enumerate((self.whole, self.winners)):
                    what = "%s, masked scan qg=%d, mask %d (%s), K=%d" % (self.kind, qg, r, ("all ones", "winners and near misses")[r], K)
                    got = g.search_masked_raw(case.qs, K, self.ms, np.full(self.nq, r, np.int32), w=pl.W)
                    searches += 1
                    st = g.get_stats()
                    if case.u16:
                        assert st["last_qg"] == -2, (what, st)
                    else:
                        d, m, _, _ = pl.KINDS[self.kind]
                        want = qg
                        while want > 1 and mk.scan_lds_bytes(m, d, want, K) > sq.LDS_MAX:      # (masked.forced_qg on this file's shapes)
                            want >>= 1
                        assert st["last_striped"] == 8 and st["last_qg"] == want and st["last_chunk"] == 1024, (what, st)
                    check(case, got, lists.expected(K), 0, what)
            finally:
                g.set_tuning(0, 0)
        return searches

    def run(self, slot):
        t0 = time.time()
        forms = forms_of(self.kind, slot, self.whole.n, self.kc, self.nq)
        searches = 0
        for f in forms:
            searches += self.search_form(self.g, f, self.whole, "%s, [%s] K=%d" % (self.kind, f["name"], f["K"]))
        searches = self.masked(pl.K_REG[slot], (1, 4), searches)
        if lds_k(slot) is not None:
            searches = self.masked(lds_k(slot), (4,), searches)
        vforms = forms_of(self.kind, slot, self.halved.n, self.kc, self.nq)
        table = [f["name"] for f in settings_of(self.kind)]
        names = [table[(VIEW_FORMS * slot + i) % len(table)] for i in range(VIEW_FORMS)]       # (a form without a K in this slot is passed over)
        for f in vforms:
            if f["name"] in names:
                searches += self.search_form(self.view, f, self.halved, "%s, subset view of every second id, [%s] K=%d" % (self.kind, f["name"], f["K"]), plain=False)
        print("placement %s slot %d: %d forms, %d searches, %.2f s wall" % (self.kind, slot, len(forms), searches, time.time() - t0))


_BENCHES = {}


@pytest.mark.parametrize("slot", range(len(pl.K_REG)))
@pytest.mark.parametrize("kind", list(pl.KINDS))
def test_forms_on_placed_lists(native, kind, slot):
    if kind not in _BENCHES:
        _BENCHES[kind] = Bench(native, kind)
    _BENCHES[kind].run(slot)


# ---- probe placement -----------------------------------------------------------------------------------------------------------------
# (name, set_tuning's first argument): the query-major plan with the fused and with the stand-alone top-w, the small-batch single launch
# (the first 512 // w queries, at most 64: what it serves), list-major at four queries per stream, the generic path
PROBE_SETTINGS = (("query-major, fused top-w", -1), ("query-major, stand-alone top-w", -3), ("small-batch single launch", 0),
                  ("list-major qg=4", 4), ("generic", -2))
COARSE_MODES = (1, 2, 6)     # exact VALU kernels; the matrix-core filter from kc >= 128; the two-level search on request
_PROBE_HANDLES = {}


def coarse_stats(qg, mode, w, planned):
    """what get_stats() must say about the coarse stage (plan.h: coarse_form): the small-batch launch and the generic path have a coarse
    stage of their own and report no filter; a planned search takes the filter under mode 2 up to w = 48 and the two-level search under
    mode 6 up to w = 64"""
    if not planned:
        return {"coarse_mfma": 0}
    return {"coarse_mfma": 1 if mode == 2 and w <= 48 else 0, "last_twolevel": 1 if mode == 6 and w <= 64 else 0}


@pytest.mark.parametrize("w", pl.PROBE_WS)
@pytest.mark.parametrize("mode", pl.PROBE_MODES)
def test_winners_by_probe(native, mode, w):
    """placement.probe_case: the all-zero-code points, which beat every ordinary point, sit only in the designer query's first probe, only
    in its last one -- the list probe pruning would drop first --, or one in every probe.  Every setting above under coarse modes 1, 2
    and 6 with pruning on and off at K = 1 / 10 / 17 / 64: the form and the coarse stage asserted through get_stats(), the oracle's
    bytes with pruning on and with pruning off.  The query-major plan ends a query when the next probe's coarse distance exceeds its
    K-th key: with the winners in probe 0 and K within them it must have pruned (the list-major items of different probes run side
    by side and prune by a bound another item publishes, or not: their count is printed, not asserted).  ivfadc_search_preassigned
    with the oracle's probes runs every K once."""
    t0 = time.time()
    c = pl.probe_case(mode, w)
    ref = c.ref
    key = id(ref)
    if key not in _PROBE_HANDLES:
        if mode == "last":
            _PROBE_HANDLES.clear()          # (one index per w: the one before is not needed again)
        _PROBE_HANDLES[key] = wp.gpu_handle(native, ref)
    g = _PROBE_HANDLES[key]
    shape = dict(m=ref.m, dsub=ref.dsub, ksub=ref.ksub, kc=ref.kc, n=int(ref.offsets[-1]), u16=False)
    searches, seen = 0, {}
    g.set_table_mode(0)
    g.set_workspace_limit(sq.WS_DEFAULT)
    try:
        for K in pl.PROBE_KS:
            exp_all = ref.knn_search(c.qs, K, w, nthreads=ora.max_threads())
            for name, qg in PROBE_SETTINGS:
                nq = min(pl.PROBE_NQ, SMALL_BATCH, 512 // w) if qg == 0 else pl.PROBE_NQ
                qs, exp = c.qs[:nq], le.part(exp_all, slice(0, nq))
                form = sq.expected_form(shape, dict(table=0, qg=qg), K, w, nq)
                assert form is not None or (qg == 0 and w > 64), name
                planned = form is None or form["last_qg"] >= 0
                g.set_tuning(qg, 0)
                for cm in COARSE_MODES:
                    g.set_coarse_mode(cm)
                    res = {}
                    for prune in (1, 0):
                        what = "winners in the %s probe, w=%d K=%d, %s, coarse mode %d, pruning %d" % (mode, w, K, name, cm, prune)
                        g.set_pruning(prune)
                        g.reset_stats()
                        res[prune] = g.search_raw(qs, K, w)
                        searches += 1
                        st = g.get_stats()
                        ran(g, dict(form or {}, **coarse_stats(qg, cm, w, planned)), what)
                        helpers.assert_same_results(res[prune], exp, what=what)
                        if prune == 0:
                            assert st["pruned_points"] == 0, (what, st)
                        else:
                            seen[(name, K)] = seen.get((name, K), 0) + int(st["pruned_points"] > 0)
                            if mode == "first" and w >= 2 and K <= 10 and qg in (-1, -3):
                                assert st["pruned_points"] > 0, (what, st)
                    assert all(np.array_equal(a, b) for a, b in zip(res[0], res[1])), what
            g.set_tuning(0, 0)
            g.set_coarse_mode(0)
            g.set_pruning(1)
            lists, dcs = le.probes_of(ref.centroids, c.qs, w)
            got = g.search_preassigned_raw(c.qs, K, lists.astype(np.int32), dcs)
            searches += 1
            helpers.assert_same_results(got, exp_all, what="winners in the %s probe, w=%d K=%d, preassigned probes" % (mode, w, K))
    finally:
        g.set_tuning(0, 0)
        g.set_coarse_mode(0)
        g.set_pruning(1)
    pruned = {name: [seen.get((name, K), 0) for K in pl.PROBE_KS] for name, _ in PROBE_SETTINGS}
    print("probe placement %s w=%d: %d searches, %.2f s wall; searches of %d that pruned, per K %s: %s" % (
        mode, w, searches, time.time() - t0, len(COARSE_MODES), pl.PROBE_KS, pruned))
