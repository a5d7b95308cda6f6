"""Support for the subset-view tests (tests/test_subset_model.py and tests/test_subset_plan.py on the CPU, tests/test_gpu_subset.py on
the GPU); not a test.  Plain numpy.

A subset view (ivfadc_clone_subset) behaves as an index whose lists hold only the entries whose stored id is selected by a bitmap, in
their stored order and with their stored ids (deleteat! of utils.jl:98-99 without _shift_inverse_index!).  Three things live here:

* filtered_lists: that sentence in numpy -- the model every device result is compared with.
* the case table: one list per length on both sides of every granularity the compaction works in (a wave's round of 64, a workgroup's
  256, the work item's SUBSET_CHUNK, read from the source), the masks and the two ways of choosing nbits, the code strides.
  The code rows of a case come from a small pool, so every list holds many exact distance ties and the ORDER of the kept entries
  shows in the ids of an exhaustive search (ties go by visit order); the ids are a permutation, so every entry is told from every other.
* MUTANTS: wrong compactions, each as a function with filtered_lists' signature.  test_subset_model.py shows that the exhaustive
  read-back tells each of them from the right one wherever its lists differ at all.
"""
import functools
import os
import re

import numpy as np

import helpers
import u16_ref
from oracle import oracle as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_H = os.path.join(ROOT, "ivfadc.jl_amd", "csrc", "subset_plan.h")
KC = 24
NQ = 2
POOL = 61                      # distinct code rows per case: ~n / 61 exact ties per row


@functools.lru_cache(maxsize=None)
def chunk():
    """SUBSET_CHUNK as csrc/subset_plan.h defines it."""
    m = re.search(r"constexpr\s+int\s+SUBSET_CHUNK\s*=\s*(\d+)\s*;", open(PLAN_H).read())
    assert m, "subset_plan.h must define SUBSET_CHUNK as a constexpr int"
    return int(m.group(1))


def lens():
    """One list per length, each length twice (kc = 24): ascending, then descending, so that every length has two different neighbours."""
    C = chunk()
    one = (0, 1, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 1)
    return one + one[::-1]


MASKS = ("all", "none", "every_other", "first_only", "last_only", "run_at_chunk", "random_half", "random_1pct")
NBITS = ("max_plus_1", "half_of_max")
# name -> (d, m, ksub, code bits): cs = 8, 12, 4, 48, 16, 12
STRIDES = {
    "u8_m8": (32, 8, 256, 8),
    "u8_m10": (40, 10, 64, 8),
    "u8_m3": (12, 3, 256, 8),
    "u8_m48": (768, 48, 256, 8),
    "u16_m8": (32, 8, 1024, 16),
    "u16_m5": (20, 5, 1024, 16),
}


def code_stride(name):
    d, m, ksub, bits = STRIDES[name]
    return (m * (bits // 8) + 3) // 4 * 4


def positions(kind, length, rng):
    """The positions of a list of `length` entries that mask `kind` selects (ascending)."""
    C = chunk()
    p = np.arange(length)
    if kind == "all":
        return p
    if kind == "none":
        return p[:0]
    if kind == "every_other":
        return p[::2]
    if kind == "first_only":
        return p[:1]
    if kind == "last_only":
        return p[-1:]
    if kind == "run_at_chunk":
        return p[(p >= C - 50) & (p < C + 50)]
    if kind == "random_half":
        return p[rng.random(length) < 0.5]
    if kind == "random_1pct":
        return p[rng.random(length) < 0.01]
    raise ValueError(kind)


class Case:
    """One index of the case table: `ref` (oracle.OracleIndex or u16_ref.U16Index, never changed) and its queries."""

    def __init__(self, stride, ref, qs):
        self.stride, self.ref, self.qs = stride, ref, qs
        self.u16 = isinstance(ref, u16_ref.U16Index)

    def lists(self):
        return self.ref.offsets, self.ref.codes, self.ref.ids

    def mask(self, kind, nbits_kind):
        """(mask, nbits): the boolean array indexed by id that `kind` selects per list, cut to nbits entries.  half_of_max: the ids at
        or above nbits that `kind` names are thereby NOT selected."""
        off, _, ids = self.lists()
        rng = np.random.default_rng(5000 + MASKS.index(kind))
        top = int(ids.max())
        full = np.zeros(top + 1, bool)
        for l in range(len(off) - 1):
            full[ids[off[l] + positions(kind, int(off[l + 1] - off[l]), rng)]] = True
        nbits = top + 1 if nbits_kind == "max_plus_1" else top // 2
        return full[:nbits].copy(), nbits

    def with_lists(self, offsets, codes, ids):
        r = self.ref
        if self.u16:
            return u16_ref.U16Index(r.centroids, r.codebooks, r.labels, offsets, codes, ids)
        return ora.OracleIndex(r.centroids, r.codebooks, r.labels, offsets, codes, ids)

    def exhaustive(self, lists, K=None):
        """(ids, dists, counts) of the w = kc, K = n (or K) search of the reference over `lists`, by the sort-based restatements."""
        ref = self.with_lists(*lists)
        K = max(1, int(lists[0][-1])) if K is None else K
        if self.u16:
            return u16_ref.knn(ref, self.qs, K, ref.kc)
        return helpers.numpy_knn_batch(ref, self.qs, K, ref.kc)


@functools.lru_cache(maxsize=None)
def case(stride):
    d, m, ksub, bits = STRIDES[stride]
    seed = 8100 + sorted(STRIDES).index(stride)
    sizes = np.array(lens(), np.int64)
    if bits == 16:
        ix = u16_ref.make_index(seed, 0, d, KC, m, ksub, perm_labels=True, ndistinct=POOL, list_sizes=sizes)
        # make_index deals the lists out at random; the table wants list l to be lens()[l] long, which list_sizes gives
        assert np.array_equal(np.diff(ix.offsets), sizes)
        ref = ix
    else:
        rng = np.random.default_rng(seed)
        cent, cbs, labels = helpers.make_quantizers(seed, d, KC, m, ksub, label_perm=ksub < 256)
        n = int(sizes.sum())
        pool = np.stack([labels[i][rng.integers(0, ksub, POOL)] for i in range(m)], 1)
        codes = np.ascontiguousarray(pool[rng.integers(0, POOL, n)], np.uint8)
        offsets = np.zeros(KC + 1, np.int64)
        np.cumsum(sizes, out=offsets[1:])
        ref = ora.OracleIndex(cent, cbs, labels, offsets, codes, rng.permutation(n).astype(np.uint32))
    qs = np.random.default_rng(seed + 1).random((NQ, d), dtype=np.float32)
    return Case(stride, ref, qs)


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def selected(mask, ids):
    """Which of `ids` the bitmap selects: id < len(mask) and mask[id]."""
    ids = np.asarray(ids, np.int64)
    ok = ids < len(mask)
    out = np.zeros(ids.shape[0], bool)
    out[ok] = np.asarray(mask, bool)[ids[ok]]
    return out


def _rebuild(offsets, keep_of_list):
    """offsets' and the concatenated source positions from a per-list array of source positions (absolute)"""
    new_off = np.zeros(len(offsets), np.int64)
    np.cumsum([len(k) for k in keep_of_list], out=new_off[1:])
    src = np.concatenate(keep_of_list).astype(np.int64) if len(keep_of_list) else np.zeros(0, np.int64)
    return new_off, src


def filtered_lists(offsets, codes, ids, mask):
    """(offsets', codes', ids'): the entries whose id `mask` (boolean, indexed by id; ids at or above its length are not selected)
    selects, in their stored order within each list, with their stored ids."""
    keep = selected(mask, ids)
    new_off = np.zeros(len(offsets), np.int64)
    np.cumsum([int(keep[offsets[l]:offsets[l + 1]].sum()) for l in range(len(offsets) - 1)], out=new_off[1:])
    return new_off, np.ascontiguousarray(codes[keep]), np.ascontiguousarray(ids[keep])


def pack(mask):
    """The bitmap words of a mask: id i at bit (i & 31) of word i >> 5."""
    by = np.packbits(np.asarray(mask, bool), bitorder="little")
    words = np.zeros((len(mask) + 31) // 32 * 4, np.uint8)
    words[:by.shape[0]] = by
    return words.view("<u4").astype(np.uint32)


# ---- wrong compactions -------------------------------------------------------------------------------------------------------------
def _per_list(offsets, codes, ids, keep, edit):
    """filtered_lists with `edit(positions within the list of the kept entries, list length) -> positions to emit` per list"""
    out = []
    for l in range(len(offsets) - 1):
        a, b = int(offsets[l]), int(offsets[l + 1])
        kept = np.nonzero(keep[a:b])[0]
        out.append(a + np.asarray(edit(kept, b - a), np.int64))
    new_off, src = _rebuild(offsets, out)
    return new_off, np.ascontiguousarray(codes[src]), np.ascontiguousarray(ids[src])


def mutant_unstable(offsets, codes, ids, mask):
    """the kept entries of every chunk come out in reverse (an atomic cursor instead of the prefix would give SOME other order)"""
    C = chunk()

    def edit(kept, length):
        return np.concatenate([kept[kept // C == c][::-1] for c in range(-(-length // C))]) if len(kept) else kept
    return _per_list(offsets, codes, ids, selected(mask, ids), edit)


def mutant_edge_dropped(offsets, codes, ids, mask):
    """the kept entry at a chunk's last position is lost"""
    C = chunk()
    return _per_list(offsets, codes, ids, selected(mask, ids), lambda kept, length: kept[kept % C != C - 1])


def mutant_edge_duplicated(offsets, codes, ids, mask):
    """the kept entry at a chunk's first position (chunks after the first) is written twice"""
    C = chunk()

    def edit(kept, length):
        return np.sort(np.concatenate([kept, kept[(kept % C == 0) & (kept > 0)]]), kind="stable")
    return _per_list(offsets, codes, ids, selected(mask, ids), edit)


def mutant_wrong_word(offsets, codes, ids, mask):
    """the bit is looked up in word id >> 6"""
    words = pack(mask)
    i = np.asarray(ids, np.int64)
    w = i >> 6
    ok = (i < len(mask)) & (w < len(words))
    keep = np.zeros(len(i), bool)
    keep[ok] = ((words[w[ok]] >> (i[ok] & 31).astype(np.uint32)) & 1) != 0
    return _per_list(offsets, codes, ids, keep, lambda kept, length: kept)


def mutant_beyond_nbits_kept(offsets, codes, ids, mask):
    """ids at or above nbits count as selected"""
    keep = selected(mask, ids) | (np.asarray(ids, np.int64) >= len(mask))
    return _per_list(offsets, codes, ids, keep, lambda kept, length: kept)


def mutant_codes_left(offsets, codes, ids, mask):
    """the ids are compacted, the code rows stay where they were: entry j of the new list has the code row of the old list's entry j"""
    new_off, _, new_ids = filtered_lists(offsets, codes, ids, mask)
    rows = [codes[offsets[l]:offsets[l] + (new_off[l + 1] - new_off[l])] for l in range(len(offsets) - 1)]
    return new_off, np.ascontiguousarray(np.concatenate(rows)), new_ids


def mutant_len_left(offsets, codes, ids, mask):
    """list_len stays the index's: behind the kept entries every list shows what the new buffers hold there -- zero rows, id 0"""
    new_off, new_codes, new_ids = filtered_lists(offsets, codes, ids, mask)
    out_codes, out_ids = np.zeros_like(codes), np.zeros_like(ids)
    for l in range(len(offsets) - 1):
        k = int(new_off[l + 1] - new_off[l])
        out_codes[offsets[l]:offsets[l] + k] = new_codes[new_off[l]:new_off[l + 1]]
        out_ids[offsets[l]:offsets[l] + k] = new_ids[new_off[l]:new_off[l + 1]]
    return np.asarray(offsets, np.int64).copy(), out_codes, out_ids


MUTANTS = {
    "unstable order within a chunk": mutant_unstable,
    "chunk edge dropped": mutant_edge_dropped,
    "chunk edge duplicated": mutant_edge_duplicated,
    "bit looked up in word id >> 6": mutant_wrong_word,
    "ids at or above nbits kept": mutant_beyond_nbits_kept,
    "code rows left at their old positions": mutant_codes_left,
    "list_len left at the index's value": mutant_len_left,
}


def same_lists(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def same_answer(a, b):
    """two (ids, dists, counts) results: identical counts, ids and distance bits over the first `count` slots"""
    if not np.array_equal(a[2], b[2]):
        return False
    for r in range(len(a[2])):
        c = int(a[2][r])
        if not np.array_equal(a[0][r, :c], b[0][r, :c]):
            return False
        if not np.array_equal(np.ascontiguousarray(a[1][r, :c]).view(np.uint32), np.ascontiguousarray(b[1][r, :c]).view(np.uint32)):
            return False
    return True
