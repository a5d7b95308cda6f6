"""Support for the masked-search tests (tests/test_masked_model.py and tests/test_maskset_plan.py on the CPU, tests/test_gpu_masked.py on
the GPU); not a test.  Plain numpy.

A masked search (ivfadc_search_masked) gives every query a mask number.  Query q with mask r >= 0 sees the index's lists with every entry
whose stored id mask r does not select removed (deleteat! of utils.jl:98-99 without _shift_inverse_index!), probed in the w cells the
UNFILTERED coarse search picks; with -1 it sees the index as it is.  Three things live here:

* masked_reference: that sentence in numpy -- per query, the reference over subset.filtered_lists.  (A coarse search reads the centroids
  only, so the reference over the filtered lists probes the cells of the unfiltered index by itself.)
* the case table: kc = 12, one list per length on both sides of a mask word (32), a wave round (64), a workgroup step (256) and the
  1024-point chunk set_tuning(qg, 1024) forces; the 1025-point list makes two work items whose partial results go through merge_kernel.
  The whole index (1956 entries) comes back at K = 1963 <= 2048, through the LDS selectors of the masked kernel itself.  Code rows from a
  pool of 61 (order shows in the ids through ties), ids a permutation, the code strides of subset.STRIDES, and the mask kinds of
  subset.MASKS under both NBITS rules: 16 masks in ONE mask set.  20 queries: one per mask and four with -1, dealt so that -- in query
  order, which is the order w = kc fills the groups of a list in -- every group of four mixes four different masks and the first and the
  last mix masked and unmasked slots.
* MUTANTS: wrong implementations, each a function with masked_reference's signature.  test_masked_model.py shows that each of them that
  changes a result differs from the model on the case table at the K and w the GPU test uses; the one that only renumbers the keys is
  shown to be EQUIVALENT (ids and distances cannot tell it), and says so.
"""
import functools

import numpy as np

import helpers
import subset as sb
import u16_ref
from oracle import oracle as ora

KC = 12
LENS = (0, 1, 31, 32, 33, 63, 64, 65, 129, 256, 257, 1025)
N = sum(LENS)                   # 1956
K_ALL = N + 7                   # 1963: everything comes back, through the LDS selectors
K_REG = 64                      # register selectors: the masks that keep at most 57 entries come back whole
POOL = sb.POOL
STRIDES = sb.STRIDES
U8_STRIDES = tuple(s for s in STRIDES if STRIDES[s][3] == 8)
U16_STRIDES = tuple(s for s in STRIDES if STRIDES[s][3] == 16)
MASKS = tuple((kind, nb) for kind in sb.MASKS for nb in sb.NBITS)      # 16
MASK_OF_QUERY = np.array([0, 1, 2, -1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, -1, -1, -1], np.int32)
NQ = len(MASK_OF_QUERY)         # 20
assert N == 1956 and K_ALL <= 2048 and len(MASKS) == 16 and sorted(MASK_OF_QUERY[MASK_OF_QUERY >= 0].tolist()) == list(range(16))


@functools.lru_cache(maxsize=None)
def case(stride):
    """subset.Case of the table above at one code stride: `ref` (never changed) and the 20 queries."""
    d, m, ksub, bits = STRIDES[stride]
    seed = 9300 + sorted(STRIDES).index(stride)
    sizes = np.array(LENS, np.int64)
    if bits == 16:
        ref = u16_ref.make_index(seed, 0, d, KC, m, ksub, perm_labels=True, ndistinct=POOL, list_sizes=sizes)
        assert np.array_equal(np.diff(ref.offsets), sizes)
    else:
        rng = np.random.default_rng(seed)
        cent, cbs, labels = helpers.make_quantizers(seed, d, KC, m, ksub, label_perm=ksub < 256)
        pool = np.stack([labels[i][rng.integers(0, ksub, POOL)] for i in range(m)], 1)
        codes = np.ascontiguousarray(pool[rng.integers(0, POOL, N)], np.uint8)
        offsets = np.zeros(KC + 1, np.int64)
        np.cumsum(sizes, out=offsets[1:])
        ref = ora.OracleIndex(cent, cbs, labels, offsets, codes, rng.permutation(N).astype(np.uint32))
    qs = np.random.default_rng(seed + 1).random((NQ, d), dtype=np.float32)
    return sb.Case(stride, ref, qs)


@functools.lru_cache(maxsize=None)
def masks(stride):
    """The 16 boolean masks (indexed by id, each as long as its nbits rule says) of a case, in MASKS order."""
    c = case(stride)
    return tuple(c.mask(kind, nb)[0] for kind, nb in MASKS)


def kept(stride):
    """entries each of the 16 masks selects"""
    ids = case(stride).ref.ids
    return np.array([int(sb.selected(mk, ids).sum()) for mk in masks(stride)], np.int64)


def _knn(c, ref, q, K, w):
    if c.u16:
        return u16_ref.knn_one(ref, q, K, w)
    return helpers.numpy_knn(ref, q, K, w)


def _pack(rows, K):
    ids = np.zeros((len(rows), K), np.uint32)
    dists = np.full((len(rows), K), np.inf, np.float32)
    counts = np.zeros(len(rows), np.int32)
    for r, (i, dd) in enumerate(rows):
        counts[r] = len(i)
        ids[r, :len(i)] = i
        dists[r, :len(i)] = dd
    return ids, dists, counts


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def masked_reference(c, mks, mask_of_query, K, w):
    """(ids, dists, counts): per query the reference over subset.filtered_lists(lists, its mask) -- over the lists themselves for -1."""
    refs = {}
    rows = []
    for qi, r in enumerate(np.asarray(mask_of_query)):
        r = int(r)
        if r not in refs:
            refs[r] = c.ref if r < 0 else c.with_lists(*sb.filtered_lists(*c.lists(), mks[r]))
        rows.append(_knn(c, refs[r], c.qs[qi], K, w))
    return _pack(rows, K)


def plain_reference(c, K, w):
    return _pack([_knn(c, c.ref, c.qs[qi], K, w) for qi in range(c.qs.shape[0])], K)


# ---- a second statement of the same thing, which the mutants are edits of ------------------------------------------------------------
# Every probed entry of a query in (distance, visit order) order, ONCE per (case, query, w): a filter that removes entries keeps the
# order of the rest, so "the first K that are kept" is the masked result with the keys' ORIGINAL visit numbers.
def _entry_tables(c):
    off, _, ids = c.lists()
    lst = np.repeat(np.arange(len(off) - 1), np.diff(off))
    pos = np.arange(len(ids)) - off[lst]
    entry_of_id = np.zeros(int(ids.max()) + 1 if len(ids) else 0, np.int64)
    entry_of_id[ids] = np.arange(len(ids))          # (ids are a permutation)
    return lst, pos, entry_of_id


@functools.lru_cache(maxsize=None)
def _sorted_entries(stride, qi, w):
    c = case(stride)
    i, dd = _knn(c, c.ref, c.qs[qi], N, w)
    return _entry_tables(c)[2][i], dd


def _filtered(c, mks, mask_of_query, K, w, keep_of, post=False, full_count=False, phantoms=False):
    """keep_of(mask, qi) -> boolean per stored entry; post: the filter runs behind the top-K; full_count: the count is the unfiltered
    one; phantoms: behind the last entry of every list whose length is no multiple of 64 stands one more, selected by every mask,
    with the last entry's code row and an id no entry has (what a bit behind list_len would let in)."""
    off, _, ids = c.lists()
    rows = []
    for qi, r in enumerate(np.asarray(mask_of_query)):
        ent, dd = _sorted_entries(c.stride, qi, w)
        keep = np.ones(len(ids), bool) if r < 0 else keep_of(mks[int(r)], qi)
        out_ids, out_d = ids[ent], dd
        k = keep[ent]
        if phantoms:
            lst = _entry_tables(c)[0]
            last = (ent + 1 == off[lst[ent] + 1]) & ((off[lst[ent] + 1] - off[lst[ent]]) % 64 != 0)
            at = np.nonzero(last)[0] + 1
            out_ids = np.insert(out_ids, at, (0xFFFFFF00 + lst[ent[last]]).astype(np.uint32))
            out_d = np.insert(out_d, at, dd[last])
            k = np.insert(k, at, True)
        if post:
            out_ids, out_d, k = out_ids[:K], out_d[:K], k[:K]
        total = len(out_ids)
        out_ids, out_d = out_ids[k][:K], out_d[k][:K]
        if full_count:
            n = min(K, total)
            out_ids = np.concatenate([out_ids, np.zeros(n - len(out_ids), np.uint32)])
            out_d = np.concatenate([out_d, np.full(n - len(out_d), np.inf, np.float32)])
        rows.append((out_ids, out_d))
    return _pack(rows, K)


def _sel(c):
    ids = c.ref.ids
    return lambda mk, qi: sb.selected(mk, ids)


def original_keys(c, mks, moq, K, w):
    """the right answer by the second statement: keys keep their original visit numbers (what the kernels do)"""
    return _filtered(c, mks, moq, K, w, _sel(c))


# ---- wrong implementations -----------------------------------------------------------------------------------------------------------
def mutant_mask_ignored(c, mks, moq, K, w):
    """the mask is ignored: every query sees the whole index"""
    return _filtered(c, mks, moq, K, w, lambda mk, qi: np.ones(len(c.ref.ids), bool))


def mutant_neighbour_slot(c, mks, moq, K, w):
    """a slot tests the mask of the neighbouring slot of its group (query qi ^ 1)"""
    moq = np.asarray(moq)
    ids = c.ref.ids

    def keep(mk, qi):
        r = int(moq[qi ^ 1]) if (qi ^ 1) < len(moq) else int(moq[qi])
        return np.ones(len(ids), bool) if r < 0 else sb.selected(mks[r], ids)
    return _filtered(c, mks, moq, K, w, keep)


def mutant_filter_after_topk(c, mks, moq, K, w):
    """the filter runs behind the top-K: fewer than K come back where K kept entries exist"""
    return _filtered(c, mks, moq, K, w, _sel(c), post=True)


def mutant_count_not_reduced(c, mks, moq, K, w):
    """the count stays min(K, probed entries): the slots behind the kept ones hold no result"""
    return _filtered(c, mks, moq, K, w, _sel(c), full_count=True)


def mutant_bit_off_by_one(c, mks, moq, K, w):
    """id i is looked up at bit i + 1"""
    ids = c.ref.ids.astype(np.int64)
    return _filtered(c, mks, moq, K, w, lambda mk, qi: sb.selected(mk, ids + 1))


def mutant_position_as_id(c, mks, moq, K, w):
    """the position within the list is taken for the id"""
    pos = _entry_tables(c)[1]
    return _filtered(c, mks, moq, K, w, lambda mk, qi: sb.selected(mk, pos))


def mutant_second_word_dropped(c, mks, moq, K, w):
    """the second word of every wave round is dropped: positions 32 .. 63 of a round are never selected"""
    pos = _entry_tables(c)[1]
    ids = c.ref.ids
    return _filtered(c, mks, moq, K, w, lambda mk, qi: sb.selected(mk, ids) & (pos % 64 < 32))


def mutant_last_round_dropped(c, mks, moq, K, w):
    """the last, partial round of a list is dropped"""
    lst, pos, _ = _entry_tables(c)
    full = (np.diff(c.ref.offsets) // 64 * 64)[lst]
    ids = c.ref.ids
    return _filtered(c, mks, moq, K, w, lambda mk, qi: sb.selected(mk, ids) & (pos < full))


def mutant_bits_behind_len(c, mks, moq, K, w):
    """bits behind list_len are honoured: what lies in the spare capacity of a list's last round comes back"""
    return _filtered(c, mks, moq, K, w, _sel(c), phantoms=True)


def mutant_keys_renumbered(c, mks, moq, K, w):
    """keys renumbered to filtered positions: visit numbers change, their ORDER does not -- ids and distances are the model's"""
    return masked_reference(c, mks, moq, K, w)


MUTANTS = {
    "mask ignored": mutant_mask_ignored,
    "mask of the neighbouring slot": mutant_neighbour_slot,
    "filter behind the top-K": mutant_filter_after_topk,
    "count not reduced": mutant_count_not_reduced,
    "bit index off by one": mutant_bit_off_by_one,
    "position in list used as id": mutant_position_as_id,
    "second word of a round dropped": mutant_second_word_dropped,
    "last partial round dropped": mutant_last_round_dropped,
    "bits behind list_len honoured": mutant_bits_behind_len,
}
EQUIVALENT = {"keys renumbered to filtered positions": mutant_keys_renumbered}


# ---- the plan's width, restated: what last_qg a forced width must report (scan_layouts.h: scan_lds_bytes, sel_cap; plan.h: make_plan_masked)
def _sel_cap(k):
    if k <= 64:
        return 64
    p = 1
    while p < k + 64:
        p <<= 1
    return max(p, 128)


def scan_lds_bytes(m, d, qg, K):
    b = max(m, 2) * 256 * qg * 4 + (d * qg + 3) // 4 * 4 * 4
    if K > 64:
        b += 4 * qg * _sel_cap(K) * 8
    b += 4 * qg * 4 + 16
    b = (b + 7) // 8 * 8 + qg * 40 + 3 * 256
    if qg == 4 and m in (8, 16):
        b += 4 * 16 * 5 * 4
    return b


def forced_qg(stride, K, qg):
    """the width make_plan_masked runs when `qg` is forced: narrowed only while the layout exceeds a CU's 160 KB"""
    d, m, _, _ = STRIDES[stride]
    while qg > 1 and scan_lds_bytes(m, d, qg, K) > (160 << 10):
        qg >>= 1
    return qg


same_answer = sb.same_answer
