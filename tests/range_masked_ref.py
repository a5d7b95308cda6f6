"""Support for the masked-range-search tests (tests/test_range_masked_model.py on the CPU, tests/test_gpu_range_masked.py on the GPU); not a
test.  Plain numpy.

A masked range search (ivfadc_range_search_masked) has no reference counterpart.  It is DEFINED as: query q with mask r >= 0 gets what
ivfadc_search_masked returns for it with K at least the number of probed points, cut after the last entry with d <= radii[q]; -1 gives the
plain range search.  Three things live here:

* reference: that sentence in numpy -- per query, masked._knn over subset.filtered_lists for its mask with K = every stored point, then
  range_ref.cut.  masked._knn serves both code widths (helpers.numpy_knn / u16_ref.knn_one).
* the case table: masked.case(stride) for u8_m8, u8_m3, u8_m10, u16_m8 and u16_m5 (kc = 12, lengths 0 .. 1025, 16 masks in one set,
  MASK_OF_QUERY's 20 queries) with range_ref.case's two edits of the quantizers -- the twin centroid (cells 7 and 8) and the exact hit in
  cell 11 -- on the UInt16 cases too (label -> codeword through U16Index.inv), and two more queries, both the hit query: one whose mask
  selects the hit point, one whose mask excludes it.  Radii per query: -1, 0, D[0], D[0]-, D[mid], D[mid]-, D[last], +inf, the dc of the
  third probe and its predecessor, dc_hit and its predecessor (x-: nextafter(x, -inf); D: the query's own MASKED sorted list at that w).
  w in {1, 3, kc, kc + 5}.
* MUTANTS: wrong implementations, as edits of a second statement of the same thing (every probed entry with its m terms, probe rank,
  position and id; the mask; the running sums; filter; sort).  test_range_masked_model.py shows that each differs from the reference.
"""
import functools

import numpy as np

import helpers
import masked as mk
import range_ref as rr
import subset as sb
import u16_ref
from oracle import oracle as ora

KC = mk.KC
N = mk.N
STRIDES = ("u8_m8", "u8_m3", "u8_m10", "u16_m8", "u16_m5")
U8_STRIDES = tuple(s for s in STRIDES if s in mk.U8_STRIDES)
U16_STRIDES = tuple(s for s in STRIDES if s in mk.U16_STRIDES)
WS = (1, 3, KC, KC + 5)
TWIN_A, TWIN_B, HIT = rr.TWIN_A, rr.TWIN_B, rr.HIT
NQ_TABLE = mk.NQ                 # the 20 queries of masked.case
NQ = NQ_TABLE + 2                # ... and the hit query twice
KINDS = ("neg", "zero", "d0", "d0-", "dmid", "dmid-", "dlast", "inf", "dc2", "dc2-", "dchit", "dchit-")
INF = np.float32(np.inf)
_prev = rr._prev
cut, pack, same = rr.cut, rr.pack, rr.same


@functools.lru_cache(maxsize=None)
def case(stride):
    """(c, moq, hit_id): subset.Case of masked.case(stride) with the twin centroid and the exact hit, 22 queries, and their mask numbers.
    c.ref is never changed."""
    base = mk.case(stride)
    r = base.ref
    cent, cbs = r.centroids.copy(), r.codebooks.copy()
    cent[TWIN_B] = cent[TWIN_A]
    grid = np.float32(1024.0)
    cent[HIT] = np.round(cent[HIT] * grid) / grid
    row = r.codes[int(r.offsets[HIT])]
    cw = []
    for ii in range(r.m):
        c = int(r.inv[ii, row[ii]]) if base.u16 else int(np.nonzero(r.labels[ii] == row[ii])[0][0])   # label -> codeword
        assert c >= 0
        cbs[ii, c] = np.round(cbs[ii, c] * grid) / grid
        cw.append(cbs[ii, c])
    if base.u16:
        ref = u16_ref.U16Index(cent, cbs, r.labels, r.offsets, r.codes, r.ids)
    else:
        ref = ora.OracleIndex(cent, cbs, r.labels, r.offsets, r.codes, r.ids)
    hitq = (cent[HIT] + np.concatenate(cw)).astype(np.float32)
    assert np.array_equal((hitq - cent[HIT]).astype(np.float32), np.concatenate(cw)), "the hit query's residual is the codeword row, exactly"
    hit_id = int(r.ids[int(r.offsets[HIT])])
    sel = [bool(sb.selected(m, np.array([hit_id]))[0]) for m in mk.masks(stride)]
    # a mask that selects the hit point and one that does not, neither of them "all" or "none" where another serves
    order = [i for i, (kind, _) in enumerate(mk.MASKS) if kind not in ("all", "none")] + [i for i, (kind, _) in enumerate(mk.MASKS) if kind in ("all", "none")]
    r_in = next(i for i in order if sel[i])
    r_out = next(i for i in order if not sel[i])
    qs = np.ascontiguousarray(np.concatenate([base.qs, hitq[None], hitq[None]]), np.float32)
    moq = np.concatenate([mk.MASK_OF_QUERY, [r_in, r_out]]).astype(np.int32)
    return sb.Case(stride, ref, qs), moq, hit_id


def masks(stride):
    return mk.masks(stride)       # (the masks are functions of the ids alone: the edits do not touch them)


@functools.lru_cache(maxsize=None)
def _filtered_ref(stride, r):
    c, _, _ = case(stride)
    return c.ref if r < 0 else c.with_lists(*sb.filtered_lists(*c.lists(), masks(stride)[r]))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def full_sorted(stride, qi, w, r=None):
    """(ids, D): the masked search of query qi (mask r; default: its own) with K = every stored point -- the reference's full sorted list"""
    c, moq, _ = case(stride)
    r = int(moq[qi]) if r is None else int(r)
    return mk._knn(c, _filtered_ref(stride, r), c.qs[qi], N, w)


def reference(stride, qis, radii, w, moq=None):
    """(lims, ids, dists): the definition, row by row"""
    _, own, _ = case(stride)
    moq = own[np.asarray(qis)] if moq is None else moq
    return pack([cut(*full_sorted(stride, int(qi), w, int(r)), rad) for qi, rad, r in zip(qis, radii, moq)])


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coarse_order(stride, qi):
    """(cells in visit order, their coarse distances) of query qi: the unfiltered index's"""
    c, _, _ = case(stride)
    acc = helpers.ref_coarse(c.ref, c.qs[qi])
    order = np.lexsort((np.arange(KC), acc))
    return order, acc[order].astype(np.float32)


@functools.lru_cache(maxsize=None)
def table(stride, w):
    """(qis, radii, kinds) of one batch: NQ queries x KINDS radii"""
    qis, radii, kinds = [], [], []
    for qi in range(NQ):
        cells, dcs = coarse_order(stride, qi)
        D = full_sorted(stride, qi, w)[1]
        if len(D) == 0:                              # nothing selected among the probes: the first probe's dc stands in for D
            D = dcs[:1]
        dchit = dcs[int(np.nonzero(cells == HIT)[0][0])]
        mid = len(D) // 2
        vals = {"neg": np.float32(-1), "zero": np.float32(0), "d0": D[0], "d0-": _prev(D[0]), "dmid": D[mid], "dmid-": _prev(D[mid]),
                "dlast": D[-1], "inf": INF, "dc2": dcs[2], "dc2-": _prev(dcs[2]), "dchit": dchit, "dchit-": _prev(dchit)}
        for k in KINDS:
            qis.append(qi)
            radii.append(vals[k])
            kinds.append(k)
    return np.array(qis), np.array(radii, np.float32), tuple(kinds)


@functools.lru_cache(maxsize=None)
def expected(stride, w):
    qis, radii, _ = table(stride, w)
    return reference(stride, qis, radii, w)


def queries(stride, w):
    """(queries, radii, mask numbers) of the batch table(stride, w)"""
    c, moq, _ = case(stride)
    qis, radii, _ = table(stride, w)
    return np.ascontiguousarray(c.qs[qis]), radii, np.ascontiguousarray(moq[qis])


# ---- a second statement of the same thing, which the mutants are edits of ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def entries(stride, qi):
    """Every stored entry as query qi sees it at w = kc, in visit order: its m terms T (the table entries of its code row), the
    terms folded (the running sum taken through every (ii, t) instead of through the sub-space sums) and the terms a kernel would take
    if it used the stored LABEL as a codeword index (UInt16), probe rank, position, list, id."""
    c, _, _ = case(stride)
    ref, q = c.ref, c.qs[qi]
    cells, dcs = coarse_order(stride, qi)
    T, Tlab, fold, rank, pos, lst, ids = [], [], [], [], [], [], []
    for j, cl in enumerate(cells):
        lo, hi = int(ref.offsets[cl]), int(ref.offsets[cl + 1])
        if hi == lo:
            continue
        res = (q - ref.centroids[cl]).astype(np.float32)
        tab = u16_ref.tables(ref, res) if c.u16 else np.stack([helpers.ref_table(ref, i, res) for i in range(ref.m)])   # [m][ksub] by codeword
        rows = ref.codes[lo:hi]
        if c.u16:
            cwi = np.stack([ref.inv[ii, rows[:, ii]] for ii in range(ref.m)], 1)
        else:
            inv = np.zeros((ref.m, 256), np.int64)
            for ii in range(ref.m):
                inv[ii, ref.labels[ii]] = np.arange(ref.ksub)
            cwi = np.stack([inv[ii, rows[:, ii]] for ii in range(ref.m)], 1)
        T.append(np.stack([tab[ii, cwi[:, ii]] for ii in range(ref.m)], 1))
        aslab = np.minimum(rows.astype(np.int64), ref.ksub - 1)              # the label itself, clamped, as a codeword index
        Tlab.append(np.stack([tab[ii, aslab[:, ii]] for ii in range(ref.m)], 1))
        f = np.full(hi - lo, dcs[j], np.float32)                              # folded: dist += df * df for every (ii, t)
        for ii in range(ref.m):
            for t in range(ref.dsub):
                df = ref.codebooks[ii, cwi[:, ii], t] - res[ii * ref.dsub + t]
                f = f + df * df
        fold.append(f)
        rank.append(np.full(hi - lo, j))
        pos.append(np.arange(hi - lo))
        lst.append(np.full(hi - lo, cl))
        ids.append(ref.ids[lo:hi])
    cat = lambda x, t: np.concatenate(x).astype(t)
    return dict(T=cat(T, np.float32), Tlab=cat(Tlab, np.float32), fold=cat(fold, np.float32), rank=cat(rank, np.int64), pos=cat(pos, np.int64),
                lst=cat(lst, np.int64), id=cat(ids, np.uint32), cells=cells, dcs=dcs)


def _running(dc, T):
    """the running sums after every sub-space: [n][m], Float32, dc first"""
    out = np.zeros(T.shape, np.float32)
    d = dc.astype(np.float32).copy()
    for ii in range(T.shape[1]):
        d = d + T[:, ii]
        out[:, ii] = d
    return out


def model_one(stride, qi, rad, w, mrow, mistake=None, chunk=1024, neighbour_row=None):
    """(ids, dists) of one query by the second statement.  mrow: its mask number.  mistake: one name of MUTANTS' values, or None."""
    c, _, _ = case(stride)
    E = entries(stride, qi)
    lens = np.diff(c.ref.offsets)
    rad = np.float32(rad)
    take = E["rank"] < min(w, KC)
    T = (E["Tlab"] if mistake == "label" else E["T"])[take]
    rank, pos, lst, ids = E["rank"][take], E["pos"][take], E["lst"][take], E["id"][take]
    dc = E["dcs"][rank]
    run = _running(dc, T)
    d = E["fold"][take] if mistake == "fold" else (run[:, -1] if T.shape[1] else dc)
    # the mask
    use = mrow if neighbour_row is None else neighbour_row
    sel = np.ones(len(ids), bool) if use < 0 else sb.selected(masks(stride)[use], ids)
    if mistake == "second_word":
        sel = sel & ((pos % 64 < 32) | (use < 0))
    # the radius test, as the kernels make it: the probe skip, then alive after every sub-space, hit = alive after the last
    if mistake == "early_ge":
        alive = (run < rad).all(axis=1)
    elif mistake == "early_term":
        alive = (T <= rad).all(axis=1)
    else:
        alive = (run <= rad).all(axis=1) if mistake != "fold" else (d <= rad)
    within = alive & ~(dc > rad) & bool(rad >= 0)
    if mistake == "ignored":
        keep = within
    elif mistake == "after_cut":
        # the unfiltered sorted list is cut to as many entries as the masked result holds, THEN filtered
        n = int((within & sel).sum())
        o = np.lexsort((pos, rank, d))
        first = np.zeros(len(d), bool)
        first[o[within[o]][:n]] = True
        keep = first & sel
    elif mistake in ("count_only", "fill_only"):
        # per work item: the count pass and the fill pass see different lanes.  count_only: the item's slots (masked count) are taken by
        # its first unmasked survivors in position order -- phantoms.  fill_only: the item has the unmasked count of slots, the masked
        # survivors fill the first of them, the rest keep what the key buffer held (modelled as key 0: distance +0, visit 0).
        item = rank * 4096 + pos // chunk
        keep = np.zeros(len(d), bool)
        lost = 0
        for it in np.unique(item):
            mine = np.nonzero((item == it) & within)[0]
            nm = int(sel[mine].sum())
            if mistake == "count_only":
                keep[mine[:nm]] = True
            else:
                keep[mine[sel[mine]]] = True
                lost += len(mine) - nm
        if mistake == "fill_only" and lost:
            k = np.nonzero(keep)[0]
            o = k[np.lexsort((pos[k], rank[k], d[k]))]
            first = c.ref.ids[int(c.ref.offsets[E["cells"][0]])] if lens[E["cells"][0]] else np.uint32(0)
            return (np.concatenate([np.full(lost, first, np.uint32), ids[o]]).astype(np.uint32),
                    np.concatenate([np.zeros(lost, np.float32), d[o]]).astype(np.float32))
    else:
        keep = within & sel
    d, rank, pos, lst, ids = d[keep], rank[keep], pos[keep], lst[keep], ids[keep]
    if mistake == "behind_len" and use >= 0:
        # bits behind list_len taken as set: one row behind the end of every probed list that does not end on a round, with the last
        # entry's distance and an id no entry has
        Ed = _running(E["dcs"][E["rank"]], E["T"])[:, -1]
        last = (E["rank"] < min(w, KC)) & (E["pos"] + 1 == lens[E["lst"]]) & (lens[E["lst"]] % 64 != 0) & (Ed <= rad) & bool(rad >= 0)
        last &= ~(E["dcs"][E["rank"]] > rad)
        d = np.concatenate([d, Ed[last]])
        rank = np.concatenate([rank, E["rank"][last]])
        pos = np.concatenate([pos, E["pos"][last] + 1])
        ids = np.concatenate([ids, (0xFFFFFF00 + E["lst"][last]).astype(np.uint32)])
    o = np.lexsort((pos, rank, d))
    return ids[o].astype(np.uint32), d[o].astype(np.float32)


def model(stride, qis, radii, w, moq=None, mistake=None):
    _, own, _ = case(stride)
    moq = own[np.asarray(qis)] if moq is None else np.asarray(moq)
    rows = []
    for row, (qi, rad) in enumerate(zip(qis, radii)):
        nb = None
        if mistake == "neighbour":
            # mask numbers not advanced with the sub-batch / sort-group offset: the second half of the batch reads the first half's
            half = (len(qis) + 1) // 2
            nb = int(moq[row - half]) if row >= half else None
        rows.append(model_one(stride, int(qi), rad, w, int(moq[row]), None if mistake == "neighbour" else mistake, neighbour_row=nb))
    return pack(rows)


MUTANTS = {
    "mask ignored": "ignored",
    "mask applied in the count pass only": "count_only",
    "mask applied in the fill pass only": "fill_only",
    "a neighbour query's mask row": "neighbour",
    "second word of a round dropped": "second_word",
    "bits behind list_len taken as set": "behind_len",
    "filter after the cut": "after_cut",
    "early-out at >= instead of >": "early_ge",
    "early-out on the term instead of the running sum": "early_term",
}
U16_MUTANTS = {
    "sub-space sum folded into the running sum": "fold",
    "code used as a label instead of a codeword index": "label",
}
