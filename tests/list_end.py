"""Support for the list-end tests (tests/test_list_end_model.py on the CPU, tests/test_gpu_list_end.py on the GPU); not a test.

What lies behind a list's `list_len` on the device -- the zero-filled spare capacity, the stale code rows and ids a delete leaves, the
next list's block -- is never a result and never enters a bound.  Every scan form reads past the end by design and
masks the tail in its own way.  Three things live here:

* hostile_case: an index on which whatever lies behind the end of a list would be the BEST candidate of that list's queries.  In every
  sub-space the codeword whose stored code is zero bytes is the zero vector and every other codeword is 4 .. 5 times longer than the
  longest residual slice, so a point with the all-zero code (a "decoy": the zero slack, and the rows a delete of the decoys leaves
  stale) has the sum dc + |r|^2 ~ 2 dc while every live point's sum is at least dc + m (3 rmax)^2.  One list per length of LENS, the
  lengths on both sides of every granularity a form reads in, and decoys at each list's end.
* Scan / select: the reference restated on the RAW rows and id slots of write_path.DeviceModel, with the ways a form could be wrong:
  overread(g) scans every probed list up to its length rounded up to a multiple of g (capped at the capacity), reach_one_more one
  slot more, tightened(g) returns live points only but cuts them at the K-th smallest sum of live and over-read points together.
* the states the CPU file and the GPU file walk (fresh, decoys deleted, appended into the freed room, three lists emptied) and the
  batch of ordinary points the third state appends.
"""
import functools

import numpy as np

import helpers
import u16_ref
import write_path as wp
from oracle import oracle as ora

f32 = np.float32
W = 3
QPL = 8                      # queries per list: query r belongs to list r // QPL
# one list per value: the live length after the deletion of the decoys
LENS = (0, 1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 265, 266, 267, 511, 512, 513, 1023, 1024, 1025,
        2047, 2048, 2049, 2111, 2112, 2113, 4095, 4096, 4097)
R_CYCLE = (1, 2, 3, 31, 32, 64, 200)
ONLY_DECOYS = 40             # the list of live length 0
GRANULES = (2, 4, 64, 128, 256, 1024)
EMPTIED = (1, 257, 2049)     # live lengths of the lists the last state deletes whole
# name -> (d, m, ksub, code bits)
KINDS = {
    "m8_d32": (32, 8, 256, 8),
    "m8_d128": (128, 8, 256, 8),
    "m16_d128": (128, 16, 256, 8),
    "m16_d96": (96, 16, 256, 8),
    "u16": (32, 4, 1024, 16),
}
STATES = ("fresh", "decoys_deleted", "appended", "lists_emptied")
NEW_ID0 = 10_000_000         # ids of the appended points


def decoys_of(l):
    """How many decoys list l starts with, at its end."""
    return ONLY_DECOYS if LENS[l] == 0 else R_CYCLE[(l - 1) % len(R_CYCLE)]


def coarse_sums(cent, qs):
    """Coarse distances of every query to every centroid in the reference's order (ascending dimension, one rounding per operation)."""
    acc = np.zeros((qs.shape[0], cent.shape[0]), f32)
    for t in range(cent.shape[1]):
        df = cent[None, :, t] - qs[:, t, None]
        acc = acc + df * df
    return acc


def probes_of(cent, qs, w=W):
    """(probed lists (nq, w) in visit order, their coarse sums): top-w by (distance, cluster id)."""
    acc = coarse_sums(cent, qs)
    order = np.stack([np.lexsort((np.arange(cent.shape[0]), acc[r]))[:w] for r in range(qs.shape[0])])
    return order, np.take_along_axis(acc, order, 1)


class Case:
    """hostile_case's result; unpacks as (reference index, queries, decoy ids per list)."""

    def __init__(self, kind, ref, qs, decoys, probes, zero_labels):
        self.kind, self.ref, self.qs, self.decoys, self.probes, self.zero_labels = kind, ref, qs, decoys, probes, zero_labels
        self.u16 = wp.is_u16(ref)

    def __iter__(self):
        return iter((self.ref, self.qs, self.decoys))


@functools.lru_cache(maxsize=None)
def hostile_case(kind):
    """See the module's docstring.  Built once per kind and left unchanged by everyone."""
    d, m, ksub, bits = KINDS[kind]
    dsub = d // m
    kc = len(LENS)
    rng = np.random.default_rng(7300 + sorted(KINDS).index(kind))
    cent = rng.random((kc, d), dtype=f32)
    qs = (cent[np.repeat(np.arange(kc), QPL)] + f32(0.02) * rng.standard_normal((kc * QPL, d)).astype(f32)).astype(f32)
    probes, _ = probes_of(cent, qs)
    assert np.array_equal(probes[:, 0], np.repeat(np.arange(kc), QPL)), "every list must be the first probe of its own queries"
    res = (qs[:, None, :] - cent[probes]).reshape(qs.shape[0], W, m, dsub).astype(np.float64)
    rmax = float(np.sqrt((res ** 2).sum(-1)).max())
    # codebooks: the zero vector where the stored code is zero bytes, every other codeword of norm 4 .. 5 rmax
    if bits == 8:
        labels = np.stack([rng.permutation(256)[:ksub] for _ in range(m)]).astype(np.uint8)
        zero = np.array([int(np.nonzero(labels[i] == 0)[0][0]) for i in range(m)])
    else:       # device codes of a 16-bit handle are codeword indices: index 0, whose label is made 0 too so that a raw zero row of the
        # model (labels) and of the device (indices) name the same codeword; the other labels are scattered over 1 .. 65535
        labels = np.stack([np.concatenate([[0], rng.permutation(65535)[:ksub - 1] + 1]) for _ in range(m)]).astype(np.uint16)
        zero = np.zeros(m, np.int64)
    dirs = rng.standard_normal((m, ksub, dsub))
    dirs /= np.sqrt((dirs ** 2).sum(-1, keepdims=True))
    cbs = (dirs * (rmax * rng.uniform(4.01, 4.99, (m, ksub, 1)))).astype(f32)
    cbs[np.arange(m), zero] = 0
    norms = np.sqrt((cbs.astype(np.float64) ** 2).sum(-1))
    assert all(norms[i, zero[i]] == 0 and np.delete(norms[i], zero[i]).min() >= 4 * rmax and norms[i].max() <= 5 * rmax for i in range(m))
    # lists: LENS[l] live points (codes from the other codewords only), then the decoys (the all-zero code)
    sizes = np.array([LENS[l] + decoys_of(l) for l in range(kc)], np.int64)
    offsets = np.zeros(kc + 1, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    n = int(offsets[-1])
    pick = rng.integers(0, ksub - 1, (n, m))
    pick += pick >= zero[None, :]
    codes = np.stack([labels[i][pick[:, i]] for i in range(m)], 1)
    is_decoy = np.zeros(n, bool)
    for l in range(kc):
        is_decoy[offsets[l] + LENS[l]:offsets[l + 1]] = True
    codes[is_decoy] = 0
    ids = rng.permutation(n).astype(np.uint32)
    decoys = tuple(ids[offsets[l] + LENS[l]:offsets[l + 1]].copy() for l in range(kc))
    if bits == 8:
        ref = ora.OracleIndex(cent, cbs, labels, offsets, np.ascontiguousarray(codes, np.uint8), ids)
    else:
        ref = u16_ref.U16Index(cent, cbs, labels, offsets, codes, ids)
    assert all((codes[~is_decoy][:, i] != labels[i][zero[i]]).all() for i in range(m))
    return Case(kind, ref, qs, decoys, probes, np.array([labels[i][zero[i]] for i in range(m)]))


def own_queries(l):
    return slice(l * QPL, (l + 1) * QPL)


# ---- the reference's sums on raw rows ------------------------------------------------------------------------------------------------
def row_sums(ref, q, cl, dc, rows):
    """The reference-order f32 sums dc + t0 + .. + t(m-1) of one query over raw code rows (labels, (n, m)) of list cl."""
    r = q - ref.centroids[cl]
    dd = np.full(rows.shape[0], dc, f32)
    if wp.is_u16(ref):
        tab = u16_ref.tables(ref, r)
        for i in range(ref.m):
            col = ref.inv[i, rows[:, i]]
            assert (col >= 0).all(), "a raw row holds a code that is no label"
            dd = dd + tab[i, col]
    else:
        for i in range(ref.m):
            tab = np.zeros(256, f32)
            tab[ref.labels[i]] = helpers.ref_table(ref, i, r)
            dd = dd + tab[rows[:, i]]
    return dd


class Scan:
    """Every query's sums over EVERY slot (live, stale and zero) of its probed lists, from a DeviceModel: computed once per state, then
    selected from by select() with whatever reach a restatement gives each list."""

    MAXK = 256

    def __init__(self, case, model):
        ref = case.ref
        self._sorted = {}
        self.lens = np.array(model.len, np.int64)
        self.caps = np.array(model.cap, np.int64)
        self.probes, dcs = probes_of(ref.centroids, case.qs)
        rows = [np.ascontiguousarray(model.rows[l][:, :model.cb]).view(model.code_dtype).reshape(-1, model.m) for l in range(ref.kc)]
        self.ids = [model.ids[l].copy() for l in range(ref.kc)]
        self.sums = [[row_sums(ref, case.qs[r], int(cl), dcs[r, j], rows[int(cl)]) for j, cl in enumerate(self.probes[r])]
                     for r in range(case.qs.shape[0])]

    def reach_exact(self):
        return self.lens.copy()

    def reach_overread(self, g):
        """Every list read up to its length rounded up to a multiple of g, capped at its capacity."""
        return np.minimum(self.caps, -(-self.lens // g) * g)

    def reach_one_more(self):
        return np.minimum(self.caps, self.lens + 1)

    def select(self, K, reach, queries=None, live_only=False):
        """(ids, dists, counts) of the K smallest (sum, visit order) keys over slots [0, reach[l]) of every probed list.  live_only:
        the slots behind the length take part in the selection -- they tighten the bound -- and are then dropped from the result."""
        assert K <= self.MAXK
        rs = range(len(self.sums)) if queries is None else range(queries.start, queries.stop)
        ids = np.zeros((len(rs), K), np.uint32)
        dists = np.full((len(rs), K), np.inf, f32)
        counts = np.zeros(len(rs), np.int32)
        key = reach.tobytes()
        for o, r in enumerate(rs):
            if (key, r) not in self._sorted:                                     # one sort per (reach, query) serves every K
                ls = [int(cl) for cl in self.probes[r]]
                dd = np.concatenate([self.sums[r][j][:reach[l]] for j, l in enumerate(ls)])
                ii = np.concatenate([self.ids[l][:reach[l]] for l in ls])
                live = np.concatenate([np.arange(reach[l]) < self.lens[l] for l in ls])
                top = np.argsort(dd, kind="stable")[:self.MAXK]                  # stable: ties in visit order
                self._sorted[(key, r)] = (ii[top], dd[top], live[top])
            ii, dd, live = (a[:K] for a in self._sorted[(key, r)])
            if live_only:
                ii, dd = ii[live], dd[live]
            counts[o] = len(ii)
            ids[o, :len(ii)] = ii
            dists[o, :len(ii)] = dd
        return ids, dists, counts

    def overread(self, g, K, queries=None):
        return self.select(K, self.reach_overread(g), queries)

    def tightened(self, g, K, queries=None):
        return self.select(K, self.reach_overread(g), queries, live_only=True)


def part(res, queries):
    return tuple(a[queries] for a in res)


def ordering_holds(case, model):
    """The construction's consequence, on the reference-order f32 sums: for every (query, probed list) the all-zero code's sum is below
    every live non-decoy point's of that list, and the all-zero code's sum in a query's FIRST list is below every live non-decoy point's
    of any of its probed lists."""
    ref = case.ref
    zero_row = np.ascontiguousarray(case.zero_labels[None, :]).astype(model.code_dtype)
    probes, dcs = probes_of(ref.centroids, case.qs)
    for r in range(case.qs.shape[0]):
        dec, live = [], []
        for j, cl in enumerate(probes[r]):
            cl = int(cl)
            rows = np.ascontiguousarray(model.rows[cl][:model.len[cl], :model.cb]).view(model.code_dtype).reshape(-1, model.m)
            rows = rows[~(rows == zero_row).all(1)]
            dec.append(row_sums(ref, case.qs[r], cl, dcs[r, j], zero_row)[0])
            live.append(row_sums(ref, case.qs[r], cl, dcs[r, j], rows).min() if rows.shape[0] else f32(np.inf))
        if not (all(d_ < l_ for d_, l_ in zip(dec, live)) and dec[0] < min(live)):
            return False
    return True


# ---- the states ----------------------------------------------------------------------------------------------------------------------
def all_decoy_ids(case):
    return np.concatenate(case.decoys).astype(np.uint32)


def append_quota():
    """Points per list the third state appends: half of the room the deleted decoys freed (none where one decoy went)."""
    return np.array([decoys_of(l) // 2 for l in range(len(LENS))], np.int64)


@functools.lru_cache(maxsize=None)
def append_batch(kind):
    """(points, lists, codes, ids) of the third state's append: ordinary points -- a centroid plus one non-zero codeword per sub-space --
    encoded by the REFERENCE's encoder, kept while their list still has quota and none of their codes is the zero codeword's (a point
    next to a centroid would be a live decoy).  In call order, as one batch."""
    case = hostile_case(kind)
    ref = case.ref
    rng = np.random.default_rng(7400 + sorted(KINDS).index(kind))
    ncand = 6000
    zero = np.array([int(np.nonzero(ref.labels[i] == case.zero_labels[i])[0][0]) for i in range(ref.m)])
    pick = rng.integers(0, ref.ksub - 1, (ncand, ref.m))
    pick += pick >= zero[None, :]
    pts = (ref.centroids[rng.integers(0, ref.kc, ncand)] + ref.codebooks[np.arange(ref.m), pick].reshape(ncand, ref.d)).astype(f32)
    lst, codes = wp.ref_encode(ref, pts)
    left = append_quota()
    keep = []
    for i in range(ncand):
        if left[lst[i]] > 0 and (codes[i] != case.zero_labels).all():
            left[lst[i]] -= 1
            keep.append(i)
    keep = np.array(keep)
    return pts[keep], lst[keep], codes[keep], (NEW_ID0 + np.arange(len(keep))).astype(np.uint32)


def emptied_ids(offsets, ids):
    """The ids of every remaining point of the lists whose live length is one of EMPTIED, in the current numbering."""
    return np.concatenate([ids[offsets[l]:offsets[l + 1]] for l in (LENS.index(x) for x in EMPTIED)]).astype(np.uint32)


def walk_states(case, upto):
    """The lists (offsets, codes, ids) of state `upto` by the restatements of the reference's list maintenance (np_delete / np_append),
    and the DeviceModel in that state.  Yields nothing; returns (lists, model, removed counts per deletion)."""
    ref = case.ref
    lists = wp.lists_of(ref)
    model = wp.DeviceModel(*lists)
    removed = []
    for state in STATES[1:STATES.index(upto) + 1]:
        if state == "decoys_deleted":
            dele = all_decoy_ids(case)
        elif state == "lists_emptied":
            dele = emptied_ids(lists[0], lists[2])
        if state == "appended":
            _, lst, codes, new_ids = append_batch(case.kind)
            lists = wp.np_append(*lists, lst, codes, new_ids)
            model.append(lst, codes, new_ids)
        else:
            *lists, cnt = wp.np_delete(*lists, dele)
            lists = tuple(lists)
            removed.append(cnt)
            model.compact(dele)
        got = model.arrays()
        assert all(np.array_equal(a, b) for a, b in zip(got, lists)), "the device model and the list maintenance disagree in state %s" % state
    return lists, model, removed


def plain_lists(case):
    """Lists of exactly the lengths LENS: the hostile index without its decoys (never mutated: a handle is created from these)."""
    return tuple(wp.np_delete(*wp.lists_of(case.ref), all_decoy_ids(case))[:3])


def first_difference(got, exp):
    """The first query whose (count, ids, distance bits) differ, or None."""
    gi, gd, gc = got
    ei, ed, ec = exp
    for r in range(len(gc)):
        c = int(ec[r])
        if int(gc[r]) != c or not np.array_equal(gi[r, :c], ei[r, :c]) or \
                not np.array_equal(np.ascontiguousarray(gd[r, :c]).view(np.uint32), np.ascontiguousarray(ed[r, :c]).view(np.uint32)):
            return r
    return None
