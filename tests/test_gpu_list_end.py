"""Every scan form at a list's end, with hostile spare capacity (tests/list_end.py; the CPU side is tests/test_list_end_model.py).

What lies behind `list_len` -- the zero slack, the stale rows and ids a delete leaves, the next list's block -- would be the BEST
candidate of the list's own queries on list_end.hostile_case, and the lists have every length on both sides of every granularity a
form reads in.  One handle per kind walks four states (decoys live; decoys deleted in place; ordinary points appended in place into
part of the freed room; three lists deleted whole), and a second index that is never mutated has lists of exactly those lengths, with
the zero slack alone behind them.  In each state every form of tests/test_gpu_sequences.py (without the list partition and the
generic-by-K duplicates), the matrix-core lower-bound rounds of m16_d96 and the forced chunks 1024 / 2048 of every list-major form
search ALL 256 queries at K = 1 / 10 / 64 (wide forms: 65 / 100 / 128), w = 3.  Every search names its form beforehand and asserts it
through get_stats(); every result is compared exactly (counts, ids, distance bits) with the reference over the MODEL's lists
(write_path.np_delete / np_append; never the handle's mirror).  test_list_end_model.py shows on the same lists and queries that
a form which counts anything behind the end -- as a result or into a bound -- fails this comparison.

A test is one (kind, state, K slot): slot i runs K = (1, 10, 64)[i] and the wide forms at (65, 100, 128)[i], at most 40 searches.
The handle of a kind is advanced from state to state as the tests ask for it (in file order: once).  Wall time per test is printed."""
import time

import numpy as np
import pytest

import helpers
import list_end as le
import sequences as sq
import write_path as wp
from oracle import oracle as ora
from test_gpu_sequences import _form, apply, forms_8bit, forms_u16, ran

pytestmark = pytest.mark.gpu
K_SMALL, K_WIDE = (1, 10, 64), (65, 100, 128)
NQ = len(le.LENS) * le.QPL
SMALL_BATCH = 64             # the single-launch form serves up to 64 queries: it runs in slices


def shape_of(kind, n):
    d, m, ksub, bits = le.KINDS[kind]
    return dict(m=m, dsub=d // m, ksub=ksub, kc=len(le.LENS), n=n, u16=bits == 16)


def settings_of(kind):
    """The distinct settings (qg, chunk, table, prune, workspace limit, wide K?) of the imported form tables -- list-partition forms and
    generic-by-K forms dropped -- plus the lower-bound rounds of m16_d96, then chunks 1024 and 2048 for every list-major one."""
    d, m, ksub, bits = le.KINDS[kind]
    base = forms_u16(m, d // m, NQ, 4) if bits == 16 else forms_8bit(m, d // m)       # (kc = 4: the table's own index, for its asserts)
    if kind == "m16_d96":
        base.append(_form("matrix-core lower-bound rounds", -1, table=2, last_qg=0, last_lb=1))
    seen, out = set(), []
    for f in base:
        if f["parts"] or (f["expect"].get("last_qg") == -2 and f["qg"] != -2):
            continue
        chunks = (f["chunk"],)
        if f["qg"] in (1, 2, 4, 8) or (bits == 16 and f["qg"] == 0):                 # list-major: takes a chunk
            chunks = tuple(dict.fromkeys((f["chunk"], 1024, 2048)))
        for chunk in chunks:
            # (a 16-bit handle plans K <= 64 alike under table modes 0 and 10, and the wide forms all ask for 10: an added chunk once per width)
            key = (f["qg"], chunk, f["table"] if bits == 8 or chunk == f["chunk"] else None, f["prune"], f["ws"], f["K"] > 64)
            if key not in seen:
                seen.add(key)
                out.append(dict(f, chunk=chunk, name="%s [qg=%d chunk=%d table=%d]" % (f["name"], f["qg"], chunk, f["table"])))
    return out


def forms_of(kind, slot, n):
    """The searches of one K slot: settings_of at K_SMALL[slot] (wide forms: K_WIDE[slot]), each with the stats it must show -- from
    sequences.expected_form, the plan's rules restated; what that leaves open (last_lb, pruned_points) from the imported form."""
    shape = shape_of(kind, n)
    out = []
    for f in settings_of(kind):
        K = (K_WIDE if f["K"] > 64 else K_SMALL)[slot]
        nq = SMALL_BATCH if f["qg"] == 0 and not shape["u16"] else NQ
        exp = sq.expected_form(shape, dict(table=f["table"], qg=f["qg"]), K, le.W, nq)
        assert exp is not None, f["name"]
        exp = dict(exp)
        for key in ("last_lb", "pruned_points"):
            if key in f["expect"]:
                exp[key] = f["expect"][key]
        if f["chunk"]:
            exp["last_chunk"] = f["chunk"]
        if exp.get("last_striped") in (2, 3):
            exp["lds_max"] = 80 * 1024
        out.append(dict(f, K=K, w=le.W, nq=nq, expect=exp))
    return out


def check(got, exp, lens, what):
    """Exact comparison; a failure names the first differing query's own list and its length."""
    r = le.first_difference(got, exp)
    if r is None:
        return
    l = r // le.QPL
    try:
        helpers.assert_same_results(le.part(got, slice(r, r + 1)), le.part(exp, slice(r, r + 1)))
        detail = "?"
    except AssertionError as e:
        detail = str(e)
    raise AssertionError("%s: first differing query %d, of list %d (length %d): %s" % (what, r, l, lens[l], detail))


class Walker:
    """One kind's handle and the model lists of the state it is in."""

    def __init__(self, native, kind, mutated=True):
        self.kind, self.case = kind, le.hostile_case(kind)
        ref = self.case.ref
        self.lists = wp.lists_of(ref) if mutated else le.plain_lists(self.case)
        self.ref = wp.ref_with_lists(ref, *self.lists)
        self.g = wp.gpu_handle(native, self.ref)
        self.state = 0 if mutated else None
        self.cache = {}
        self.g.search_raw(self.case.qs[-1:], 1, 1)                             # a search: the device layout is current from here on

    def _set(self, lists):
        self.lists = tuple(lists)
        self.ref = wp.ref_with_lists(self.case.ref, *self.lists)
        self.cache = {}
        assert len(self.g) == int(self.lists[0][-1])
        assert np.array_equal(self.g.list_sizes(), np.diff(self.lists[0]))

    def _delete(self, dele, what):
        *lists, removed = wp.np_delete(*self.lists, dele)
        assert removed == len(dele) > 0
        assert self.g._delete_ids(dele) == removed, what
        self._set(lists)

    def advance(self, state):
        target = le.STATES.index(state)
        assert self.state is not None and self.state <= target
        while self.state < target:
            nxt = le.STATES[self.state + 1]
            before = self.g.get_stats()["inplace_appends"]
            if nxt == "decoys_deleted":
                self._delete(le.all_decoy_ids(self.case), nxt)
                assert np.array_equal(np.diff(self.lists[0]), le.LENS)
            elif nxt == "appended":
                # in place -- into blocks whose capacity dates from before the deletion: test_list_end_model.py shows that one list takes
                # more points than a re-layout after the deletion would have left room for, so the stale rows behind are still there
                pts, lst, codes, ids = le.append_batch(self.kind)
                self.g._append(pts, ids)
                assert self.g.get_stats()["inplace_appends"] == before + 1, "the append must go in place"
                self._set(wp.np_append(*self.lists, lst, codes, ids))
            else:
                self._delete(le.emptied_ids(self.lists[0], self.lists[2]), nxt)
                assert all(np.diff(self.lists[0])[le.LENS.index(x)] == 0 for x in le.EMPTIED)
            if nxt != "appended":
                assert self.g.get_stats()["inplace_appends"] == before
            self.state += 1

    def expected(self, K):
        if K not in self.cache:
            if self.case.u16:
                self.cache[K] = wp.ref_knn(self.ref, self.case.qs, K, le.W)
            else:
                self.cache[K] = self.ref.knn_search(self.case.qs, K, le.W, nthreads=ora.max_threads())
        return self.cache[K]

    def run(self, slot, state):
        t0 = time.time()
        lens = np.diff(self.lists[0])
        forms = forms_of(self.kind, slot, int(self.lists[0][-1]))
        searches = 0
        for f in forms:
            K = f["K"]
            exp = self.expected(K)
            apply(self.g, f, self.case.u16)
            for q0 in range(0, NQ, f["nq"]):
                what = "%s, %s, [%s] K=%d, queries %d..%d" % (self.kind, state, f["name"], K, q0, q0 + f["nq"] - 1)
                if "pruned_points" in f["expect"]:
                    self.g.reset_stats()
                sl = slice(q0, q0 + f["nq"])
                got = self.g.search_raw(self.case.qs[sl], K, le.W)
                searches += 1
                ran(self.g, f["expect"], what)
                check(got, le.part(exp, sl), lens[q0 // le.QPL:], what)
                if state == "fresh":            # positive control: the decoys are live, and the device returns them
                    for r in range(f["nq"]):
                        l = (q0 + r) // le.QPL
                        want = self.case.decoys[l][:min(K, le.decoys_of(l))]
                        assert np.array_equal(got[0][r, :len(want)], want), "%s: query %d does not return the decoys of list %d" % (what, q0 + r, l)
        assert searches <= 40, searches
        print("list end %s %s slot %d: %d forms, %d searches, %.2f s wall" % (self.kind, state, slot, len(forms), searches, time.time() - t0))


_WALKERS = {}


def walker(native, kind, state):
    """The kind's handle in `state`: advanced if it is behind, built anew if it is already past it (tests run out of file order)."""
    w = _WALKERS.get(kind)
    if w is None or w.state > le.STATES.index(state):
        w = _WALKERS[kind] = Walker(native, kind)
    w.advance(state)
    return w


@pytest.mark.parametrize("slot", (0, 1, 2))
@pytest.mark.parametrize("state", le.STATES)
@pytest.mark.parametrize("kind", list(le.KINDS))
def test_forms_at_the_list_end(native, kind, state, slot):
    walker(native, kind, state).run(slot, state)


_PLAIN = {}


@pytest.mark.parametrize("slot", (0, 1, 2))
@pytest.mark.parametrize("kind", list(le.KINDS))
def test_forms_on_a_never_mutated_index(native, kind, slot):
    """Lists of exactly the lengths list_end.LENS, created and searched, nothing else: the zero slack alone is the decoy."""
    if kind not in _PLAIN:
        _PLAIN[kind] = Walker(native, kind, mutated=False)
    w = _PLAIN[kind]
    assert np.array_equal(w.g.list_sizes(), le.LENS)
    w.run(slot, "never mutated")
