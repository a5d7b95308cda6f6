"""Support for the range-search tests (tests/test_range_model.py on the CPU, tests/test_gpu_range.py on the GPU); not a test.  Plain numpy.

A range search (ivfadc_range_search) has no reference counterpart: it is DEFINED as knn_search (index.jl:204-258) with K at least the
number of probed points, cut after the last entry whose Float32 distance d satisfies d <= r.  Three things live here:

* range_reference: that sentence in numpy -- helpers.numpy_knn with K = every stored point, and the prefix with d <= r.
* the case table: masked.case(stride) for every 8-bit stride (kc = 12, list lengths 0, 1, 31 .. 257, 1025, code rows from a pool of 61,
  ids a permutation; the chunk set_tuning(0, 1024) forces cuts the 1025-point list), with two edits of the quantizers that the lists,
  codes and ids do not see:
    - cell TWIN_B gets cell TWIN_A's centroid, so the two cells give the same dc, the same residual and the same tables: every code row
      the two lists share is an exact tie ACROSS two lists, which only the probe rank orders;
    - cell HIT's centroid and the codewords of its first point are rounded to multiples of 2^-10, and the last query is that centroid plus
      those codewords: the sums are exact, the residual IS the codeword row, every table entry of that row is +0 and the point's distance
      is dc itself -- the one place where "skip the probe when dc > r" and "... when dc >= r" differ.
  Six queries, and for each the radii -1, 0, D[0], D[0]-, D[j], D[j]- for a j strictly inside a tie run and for a j whose run spans two
  lists, dc_2, dc_2-, dc_hit, dc_hit-, D[-1], +inf (x-: nextafter(x, -inf); D: the reference's full sorted distance list at that w; dc_2:
  the coarse distance of the third probe; dc_hit: of cell HIT), at w in {1, 3, kc, kc + 5}.
* MUTANTS: wrong implementations, as edits of a second statement of the same thing (every probed entry with its distance, probe rank and
  position; filter; sort).  test_range_model.py shows that each of them differs from the reference on the table.
"""
import functools

import numpy as np

import helpers
import masked as mk
from oracle import oracle as ora

KC = mk.KC
N = mk.N
STRIDES = mk.U8_STRIDES
WS = (1, 3, KC, KC + 5)
CHUNK = 1024                     # the forced chunk of the table: the 1025-point list is two work items
TWIN_A, TWIN_B = 7, 8            # lists of 65 and 129 points
HIT = 11                         # the 1025-point list
NQ = 6
KINDS = ("neg", "zero", "d0", "d0-", "in_run", "in_run-", "cross_run", "cross_run-", "dc2", "dc2-", "dchit", "dchit-", "dlast", "inf")
assert mk.LENS[TWIN_A] == 65 and mk.LENS[TWIN_B] == 129 and mk.LENS[HIT] == 1025


def _prev(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


@functools.lru_cache(maxsize=None)
def case(stride):
    """(ref, qs): masked.case(stride) with the twin centroid and the exact hit (module docstring); ref is never changed."""
    base = mk.case(stride)
    r = base.ref
    cent, cbs = r.centroids.copy(), r.codebooks.copy()
    cent[TWIN_B] = cent[TWIN_A]
    grid = np.float32(1024.0)
    cent[HIT] = np.round(cent[HIT] * grid) / grid
    row = r.codes[int(r.offsets[HIT])]
    cw = []
    for ii in range(r.m):
        c = int(np.nonzero(r.labels[ii] == row[ii])[0][0])
        cbs[ii, c] = np.round(cbs[ii, c] * grid) / grid
        cw.append(cbs[ii, c])
    ref = ora.OracleIndex(cent, cbs, r.labels, r.offsets, r.codes, r.ids)
    hitq = (cent[HIT] + np.concatenate(cw)).astype(np.float32)
    assert np.array_equal((hitq - cent[HIT]).astype(np.float32), np.concatenate(cw)), "the hit query's residual is the codeword row, exactly"
    qs = np.ascontiguousarray(np.concatenate([base.qs[:NQ - 1], hitq[None]]), np.float32)
    return ref, qs


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def full_sorted(stride, qi, w):
    """(ids, D): knn_search of query qi with K = every stored point -- the reference's full sorted list at w probes"""
    ref, qs = case(stride)
    return helpers.numpy_knn(ref, qs[qi], N, w)


def cut(ids, dd, r):
    """the prefix with d <= r (dd ascending; NaN and negative radii keep nothing)"""
    n = int(np.count_nonzero(dd <= np.float32(r)))
    assert n == 0 or bool((dd[:n] <= np.float32(r)).all())
    return ids[:n], dd[:n]


def range_reference(ref, q, r, w):
    """(ids, dists) of range_search(ref, q, r; w): knn_search with K = every stored point, cut after the last entry with d <= r"""
    i, dd = helpers.numpy_knn(ref, q, max(1, int(ref.offsets[-1])), w)
    return cut(i, dd, r)


def pack(rows):
    """[(ids, dists)] per query -> (lims, ids, dists), the CSR form the entries return"""
    lims = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(i) for i, _ in rows], out=lims[1:])
    ids = np.concatenate([i for i, _ in rows]).astype(np.uint32) if rows else np.zeros(0, np.uint32)
    dd = np.concatenate([d for _, d in rows]).astype(np.float32) if rows else np.zeros(0, np.float32)
    return lims, ids, dd


# ---- a second statement of the same thing, which the mutants are edits of ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def entries(stride, qi):
    """Every stored entry as query qi sees it at w = kc, in visit order: distance, probe rank, position, list, id; and per rank the
    cell and its coarse distance.  (The entries of w probes are those with rank < w.)"""
    ref, qs = case(stride)
    q = qs[qi]
    acc = helpers.ref_coarse(ref, q)
    order = np.lexsort((np.arange(ref.kc), acc))
    dd, rank, pos, lst, ids = [], [], [], [], []
    for j, cl in enumerate(order):
        lo, hi = int(ref.offsets[cl]), int(ref.offsets[cl + 1])
        if hi == lo:
            continue
        res = q - ref.centroids[cl]
        tab = np.zeros((ref.m, 256), np.float32)
        for i in range(ref.m):
            tab[i, ref.labels[i]] = helpers.ref_table(ref, i, res)
        dd.append(helpers.ref_adc(acc[cl], [tab[ii, ref.codes[lo:hi, ii]] for ii in range(ref.m)]))
        rank.append(np.full(hi - lo, j))
        pos.append(np.arange(hi - lo))
        lst.append(np.full(hi - lo, cl))
        ids.append(ref.ids[lo:hi])
    cat = lambda x, t: np.concatenate(x).astype(t)
    return dict(d=cat(dd, np.float32), rank=cat(rank, np.int64), pos=cat(pos, np.int64), lst=cat(lst, np.int64), id=cat(ids, np.uint32),
                cells=order, dcs=acc[order].astype(np.float32))


def model_one(stride, qi, r, w, strict=False, skip_ge=False, no_rank=False, drop_last_round=False, phantoms=False, per_query_fill=False,
              restart_visit=False, no_clamp=False, chunk=CHUNK):
    """(ids, dists) of one query by the second statement; every keyword is one mistake"""
    ref, _ = case(stride)
    E = entries(stride, qi)
    r = np.float32(r)
    lens = np.diff(ref.offsets)
    d, rank, pos, lst, ids = E["d"], E["rank"], E["pos"], E["lst"], E["id"]
    take = rank < min(w, KC)
    d, rank, pos, lst, ids = d[take], rank[take], pos[take], lst[take], ids[take]
    if no_clamp and w > KC:       # the probes behind the row's end: the row is read on, round again from its start
        again = rank < w - KC
        d, pos, lst, ids = (np.concatenate([x, x[again]]) for x in (d, pos, lst, ids))
        rank = np.concatenate([rank, rank[again] + KC])
    if phantoms:                  # one row behind list_len wherever the list does not end on a round: the last entry's code row
        last = (pos + 1 == lens[lst]) & (lens[lst] % 64 != 0)
        d, rank, lst = (np.concatenate([x, x[last]]) for x in (d, rank, lst))
        ids = np.concatenate([ids, (0xFFFFFF00 + lst[-int(last.sum()):]).astype(np.uint32) if last.any() else ids[:0]])
        pos = np.concatenate([pos, pos[last] + 1])
    dc = E["dcs"][rank % KC]
    keep = ~(dc >= r) if skip_ge else ~(dc > r)          # the probe skip: no entry of a probe with dc > r can pass (d >= dc)
    if drop_last_round:
        keep &= pos < lens[lst] // 64 * 64
    keep &= (d < r) if strict else (d <= r)
    if not (r >= 0):
        keep[:] = False
    d, rank, pos, lst, ids = d[keep], rank[keep], pos[keep], lst[keep], ids[keep]
    vpos = pos % chunk if restart_visit else pos          # position as the visit order names it
    if restart_visit:
        ids = ref.ids[ref.offsets[lst] + vpos]
    if per_query_fill:            # every item writes from the query's first slot: later items overwrite earlier ones, the rest stays 0
        item = rank * 4096 + pos // chunk
        buf = np.full(len(d), -1, np.int64)
        for it in np.unique(item):
            mine = np.nonzero(item == it)[0]
            buf[:len(mine)] = mine
        zero = buf < 0
        b = np.where(zero, 0, buf)
        d, rank, vpos, ids = np.where(zero, np.float32(0), d[b]), np.where(zero, 0, rank[b]), np.where(zero, 0, vpos[b]), \
            np.where(zero, np.uint32(0xFFFFFFFF), ids[b])
    o = np.lexsort((rank, vpos, d)) if no_rank else np.lexsort((vpos, rank, d))
    return ids[o].astype(np.uint32), d[o].astype(np.float32)


def model(stride, qis, radii, w, lims_shift=False, **mistake):
    rows = [model_one(stride, int(qi), r, w, **mistake) for qi, r in zip(qis, radii)]
    lims, ids, dd = pack(rows)
    if lims_shift:                # lims off by one item: row q starts where row q + 1 does
        lims = np.concatenate([lims[1:], lims[-1:]])
    return lims, ids, dd


MUTANTS = {
    "strict <": dict(strict=True),
    "probe skipped at dc >= r": dict(skip_ge=True),
    "ties in position order, probe rank ignored": dict(no_rank=True),
    "last partial round of 64 dropped": dict(drop_last_round=True),
    "rows behind list_len counted": dict(phantoms=True),
    "lims off by one item": dict(lims_shift=True),
    "fill offsets per query instead of per item": dict(per_query_fill=True),
    "visit order restarted per chunk": dict(restart_visit=True),
    "w not clamped": dict(no_clamp=True),
}
EQUIVALENT = {}     # every mutant above changes a result on the table (test_range_model.py)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def _run_index(E, take, D, want_cross):
    """a j with D[j - 1] == D[j] == D[j + 1] whose run of equal distances spans two lists (want_cross) or lies in any lists; None if there
    is none"""
    d, rank = E["d"][take], E["rank"][take]
    for j in range(1, len(D) - 1):
        if D[j - 1] == D[j] == D[j + 1]:
            spans = len(np.unique(rank[d == D[j]])) > 1
            if spans == want_cross:
                return j
    return None


@functools.lru_cache(maxsize=None)
def table(stride, w):
    """(qis, radii, kinds, flags) of one batch: NQ queries x KINDS radii.  flags: which preconditions each row meets."""
    ref, _ = case(stride)
    qis, radii, kinds = [], [], []
    for qi in range(NQ):
        E = entries(stride, qi)
        take = E["rank"] < min(w, KC)
        _, D = full_sorted(stride, qi, w)
        assert len(D) == int(take.sum())
        if len(D) == 0:                             # w = 1 and the nearest list is the empty one: the probe's dc stands in for D
            D = E["dcs"][:1]
        jin = _run_index(E, take, D, False)
        jx = _run_index(E, take, D, True)
        jin = jin if jin is not None else (jx if jx is not None else 0)   # (a probed list of one or two points has no run)
        jx = jx if jx is not None else jin          # (no cross-list run among these probes: the in-list one twice)
        dc2 = E["dcs"][2]
        dchit = E["dcs"][int(np.nonzero(E["cells"] == HIT)[0][0])]
        vals = {"neg": np.float32(-1), "zero": np.float32(0), "d0": D[0], "d0-": _prev(D[0]), "in_run": D[jin], "in_run-": _prev(D[jin]),
                "cross_run": D[jx], "cross_run-": _prev(D[jx]), "dc2": dc2, "dc2-": _prev(dc2), "dchit": dchit, "dchit-": _prev(dchit),
                "dlast": D[-1], "inf": np.float32(np.inf)}
        for k in KINDS:
            qis.append(qi)
            radii.append(vals[k])
            kinds.append(k)
    return np.array(qis), np.array(radii, np.float32), tuple(kinds)


@functools.lru_cache(maxsize=None)
def expected(stride, w):
    """(lims, ids, dists) of the batch table(stride, w) by range_reference's definition (the full sorted list is computed once per query)"""
    qis, radii, _ = table(stride, w)
    return pack([cut(*full_sorted(stride, int(qi), w), r) for qi, r in zip(qis, radii)])


def queries(stride, w):
    ref, qs = case(stride)
    qis, radii, _ = table(stride, w)
    return np.ascontiguousarray(qs[qis]), radii


def same(a, b):
    """lims, ids and distance BITS equal"""
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and np.array_equal(np.asarray(a[2], np.float32).view(np.uint32), np.asarray(b[2], np.float32).view(np.uint32)))
