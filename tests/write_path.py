"""Support for the write-path tests (tests/test_write_path_model.py on the CPU, tests/test_gpu_write_path.py on the GPU); not a test.

Three things live here:

* read_back / assert_device_equals: the whole live device copy of the lists, observed through ONE exhaustive search (w = kc,
  K = len(index)) and compared with a reference index built from a MODEL of the lists -- never from the library's host mirror.
  Every stored point comes back with its id and its distance bits, in key order, so a code byte or an id that a kernel moved
  wrongly changes the answer unless it hides behind an exact distance tie for every query.
* np_delete / np_shift / np_append: vectorised restatements of the reference's list maintenance (utils.jl:1-27, 90-105, 127-145) for
  the shapes the quadratic literal model (_RefModel in tests/test_gpu_parity.py) is too slow for.
* the `chunks` geometry, its code strides and its deletion patterns, shared by the CPU and the GPU file so that the CPU file can show
  on the very same lists and queries that the read-back tells a wrong compaction from a right one (DeviceModel and its mutants).
"""
import numpy as np

import helpers
import u16_ref
from oracle import oracle as ora


# ---- one face for the two references (oracle.OracleIndex for UInt8 codes, u16_ref.U16Index for UInt16 codes) --------------------
def is_u16(ref):
    return isinstance(ref, u16_ref.U16Index)


def ref_with_lists(ref, offsets, codes, ids):
    """A reference index with `ref`'s quantizers over the given lists."""
    if is_u16(ref):
        return u16_ref.U16Index(ref.centroids, ref.codebooks, ref.labels, offsets, codes, ids)
    return ora.OracleIndex(ref.centroids, ref.codebooks, ref.labels, offsets, codes, ids)


def ref_empty(ref):
    code_t = np.uint16 if is_u16(ref) else np.uint8
    return ref_with_lists(ref, np.zeros(ref.kc + 1, np.int64), np.zeros((0, ref.m), code_t), np.zeros(0, np.uint32))


def ref_knn(ref, qs, K, w):
    if is_u16(ref):
        return u16_ref.knn(ref, qs, K, w)
    return ref.knn_search(qs, K, w)


def ref_encode(ref, pts):
    if is_u16(ref):
        return u16_ref.encode(ref, pts)
    return ref.encode(pts)


def lists_of(ref):
    return ref.offsets, ref.codes, ref.ids


def gpu_handle(native, ref, with_lists=True):
    """A device index with `ref`'s quantizers (UInt16 labels make a UInt16-code handle) and, unless told otherwise, its lists."""
    if with_lists:
        return native.IVFADCIndex.from_arrays(ref.centroids, ref.codebooks, ref.labels, ref.offsets, ref.codes, ref.ids)
    return native.IVFADCIndex.from_arrays(ref.centroids, ref.codebooks, ref.labels)


# ---- the exhaustive read-back ----------------------------------------------------------------------------------------------------
def read_back(g, qs, plan=-2, restore=(0, 0)):
    """(ids, dists, counts) of a search over EVERY list for EVERY stored point: w = kc, K = max(1, len(g)).  plan -2 is the generic
    dump-and-sort path, which takes any K and w; the handle's tuning is set back to `restore` afterwards."""
    K = max(1, len(g))
    g.set_tuning(plan, 0)
    try:
        return g.search_raw(qs, K, g.kc)
    finally:
        g.set_tuning(*restore)


def assert_device_equals(g, ref, qs, what="", restore=(0, 0), plans=(-2, 0), knn=ref_knn):
    """The device copy of g's lists is `ref`'s lists: the exhaustive search of g equals the exhaustive search of the reference in
    counts, ids and distance bits, and every count is len(g) == the reference's size.  plans: the read-back is repeated through each
    (-2: generic path; 0: whatever the library plans for this K and w by itself), so that it does not rest on one implementation."""
    n = int(ref.offsets[-1])
    assert len(g) == n, "%s: the index holds %d points, the model %d" % (what, len(g), n)
    K = max(1, n)
    exp = knn(ref, qs, K, ref.kc)
    assert (np.asarray(exp[2]) == n).all(), "%s: the reference itself must return every point" % what
    for plan in plans:
        got = read_back(g, qs, plan, restore)
        assert (got[2] == len(g)).all(), "%s plan %d: counts %s, stored %d" % (what, plan, got[2], len(g))
        helpers.assert_same_results(got, exp, what="%s (read-back, plan %d)" % (what, plan))


def numpy_exhaustive(ref, qs, K, w):
    """helpers.numpy_knn_batch in ref_knn's form: the sort-based restatement, for K so large that the C oracle's bounded insertion
    (quadratic in K) would take minutes."""
    return helpers.numpy_knn_batch(ref, qs, K, w)


# ---- utils.jl restated on flat arrays --------------------------------------------------------------------------------------------
def _list_of_point(offsets):
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))


def np_delete(offsets, codes, ids, del_ids):
    """delete_from_index! on 0-based ids (utils.jl:90-105 with _shift_inverse_index!, :16-20): the stored ids among del_ids go,
    survivors keep their order, every surviving id drops by the number of removed ids below it.  Ids that are not stored and
    duplicates in the request are ignored.  Returns (offsets, codes, ids, number removed)."""
    offsets, ids = np.asarray(offsets, np.int64), np.asarray(ids, np.uint32)
    rem = np.intersect1d(np.unique(np.asarray(del_ids, np.uint32)), ids)          # sorted, distinct, stored
    keep = ~np.isin(ids, rem)
    kept = ids[keep]
    new_ids = (kept - np.searchsorted(rem, kept, side="left").astype(np.uint32)).astype(np.uint32)
    new_off = np.zeros_like(offsets)
    np.cumsum(np.bincount(_list_of_point(offsets)[keep], minlength=len(offsets) - 1), out=new_off[1:])
    return new_off, np.ascontiguousarray(codes[keep]), new_ids, int(ids.shape[0] - kept.shape[0])


def np_shift(offsets, codes, ids, delta):
    """_shift_up_inverse_index! (utils.jl:1-6): every stored id moves by delta (modulo 2^32, as UInt32 arithmetic does)."""
    return offsets, codes, ((np.asarray(ids, np.uint32).astype(np.int64) + int(delta)) % (1 << 32)).astype(np.uint32)


def np_append(offsets, codes, ids, lst, new_codes, new_ids):
    """push! for a batch (utils.jl:139-144): point i goes to the END of list lst[i], in call order."""
    offsets = np.asarray(offsets, np.int64)
    new_codes = np.asarray(new_codes, codes.dtype).reshape(-1, codes.shape[1])
    lop = np.concatenate([_list_of_point(offsets), np.asarray(lst, np.int64)])
    order = np.argsort(lop, kind="stable")
    new_off = np.zeros_like(offsets)
    np.cumsum(np.bincount(lop, minlength=len(offsets) - 1), out=new_off[1:])
    return (new_off, np.ascontiguousarray(np.concatenate([codes, new_codes])[order]),
            np.concatenate([np.asarray(ids, np.uint32), np.asarray(new_ids, np.uint32)])[order])


# ---- the `chunks` geometry -------------------------------------------------------------------------------------------------------
CHUNK = 256                                                # points per pass of the compaction kernel
CHUNK_LENS = (1000, 256, 257, 512, 255, 1, 0, 300)         # three full chunks and a ragged one, the chunk boundary from both sides, 1, 0
SHORT_LIST = 5                                             # the list of length 1
# name -> (code bits, d, m, ksub): cb = m * bits / 8 code bytes per point, stored at a stride of cs = cb rounded up to 4
STRIDES = {
    "u8_cs8": (8, 32, 8, 256),
    "u8_cb10_cs12": (8, 20, 10, 256),
    "u8_cb6_cs8": (8, 12, 6, 256),
    "u8_cs4": (8, 4, 2, 256),
    "u8_cs48": (8, 96, 48, 256),
    "u16_cb6_cs8": (16, 6, 3, 1000),
    "u16_cs4": (16, 4, 1, 1000),
}
PATTERNS = ("every_other", "chunk0_of_long_lists", "all_but_last_of_each_chunk", "boundary_pairs", "whole_list",
            "all_but_one_in_middle_chunk", "everything", "absent_and_duplicates")


def code_bytes(stride):
    bits, _, m, _ = STRIDES[stride]
    return m * bits // 8


def chunks_case(stride, nq=2):
    """(reference index over the `chunks` lists, queries): random valid codes, shuffled ids, seeded by the stride's name."""
    bits, d, m, ksub = STRIDES[stride]
    seed = 8800 + sorted(STRIDES).index(stride)
    n = sum(CHUNK_LENS)
    if bits == 16:
        ref = u16_ref.make_index(seed, n, d, len(CHUNK_LENS), m, ksub, list_sizes=CHUNK_LENS)
    else:
        rng = np.random.default_rng(seed)
        cent, cbs, labels = helpers.make_quantizers(seed, d, len(CHUNK_LENS), m, ksub, label_perm=True)
        codes = np.stack([labels[i][rng.integers(0, ksub, n)] for i in range(m)], 1).astype(np.uint8)
        offsets = np.zeros(len(CHUNK_LENS) + 1, np.int64)
        np.cumsum(CHUNK_LENS, out=offsets[1:])
        ref = ora.OracleIndex(cent, cbs, labels, offsets, codes, rng.permutation(n).astype(np.uint32))
    assert np.array_equal(np.diff(ref.offsets), CHUNK_LENS)
    return ref, chunk_queries(stride, nq)


def chunk_queries(stride, nq):
    d = STRIDES[stride][1]
    return np.random.default_rng(99 + sorted(STRIDES).index(stride)).random((nq, d), dtype=np.float32)


def pattern_positions(pattern, length):
    """Positions (within a list of `length` points) that a deletion pattern removes."""
    pos = np.arange(length)
    if pattern == "every_other":
        return pos[1::2]
    if pattern == "chunk0_of_long_lists":                  # survivors move down a whole chunk
        return pos[:CHUNK] if length > CHUNK else pos[:0]
    if pattern == "all_but_last_of_each_chunk":
        last = np.minimum((pos // CHUNK + 1) * CHUNK, length) - 1
        return pos[pos != last]
    if pattern == "boundary_pairs":
        want = np.array([0, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, length - 1])
        return np.unique(want[(want >= 0) & (want < length)])
    if pattern == "all_but_one_in_middle_chunk":
        if length == 0:
            return pos
        mid = ((length - 1) // CHUNK) // 2
        return pos[pos != min(mid * CHUNK + 100, length - 1)]
    if pattern == "everything":
        return pos
    raise ValueError(pattern)


def pattern_ids(pattern, offsets, ids):
    """The 0-based ids a deletion pattern asks to remove, for the current lists.  `whole_list`: the longest list;
    `absent_and_duplicates`: three stored ids, each named twice, among ids that are not stored."""
    offsets, ids = np.asarray(offsets, np.int64), np.asarray(ids, np.uint32)
    n = int(offsets[-1])
    if pattern == "whole_list":
        big = int(np.argmax(np.diff(offsets)))
        return ids[offsets[big]:offsets[big + 1]].copy()
    if pattern == "absent_and_duplicates":
        stored = ids[[0, n // 2, n - 1]]
        return np.concatenate([absent_ids(n), stored, stored[::-1], absent_ids(n)]).astype(np.uint32)
    out = [ids[offsets[l] + pattern_positions(pattern, int(offsets[l + 1] - offsets[l]))] for l in range(len(offsets) - 1)]
    return np.concatenate(out).astype(np.uint32)


def absent_ids(n):
    """Ids that an index of n points numbered 0 .. n-1 does not store."""
    return np.array([n, n + 5, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)


def capacity(lens):
    """Slots per list after a re-layout: len + max(32, len / 8) (the library's capacity rule; the tests compute from it which appends
    must stay in place and how many id slots the shift kernel walks)."""
    lens = np.asarray(lens, np.int64)
    return lens + np.maximum(32, lens // 8)


# ---- the device layout and its kernels, restated in numpy, with the ways they could be wrong -------------------------------------
MUTANTS = ("ids_lowered_in_first_chunk_only", "second_column_from_destination", "length_of_last_chunk", "append_at_len_times_cb")


class DeviceModel:
    """The device copy of the lists as the library lays it out -- per list `cap` id slots and `cap` code rows of cs = align4(cb) bytes,
    zero-filled spare room -- with delete_compact_kernel and append_scatter_kernel restated step by step (256-point chunks, a carried
    write cursor, one dword column at a time).  mutant=None is the kernels as they should be; each name in MUTANTS is one way of
    getting them subtly wrong.  arrays() reads the live part back as (offsets, codes, ids)."""

    def __init__(self, offsets, codes, ids):
        codes = np.ascontiguousarray(codes)
        self.code_dtype, self.m = codes.dtype, codes.shape[1]
        raw = codes.view(np.uint8).reshape(codes.shape[0], -1)
        self.cb = raw.shape[1]
        self.cs = (self.cb + 3) & ~3
        lens = np.diff(np.asarray(offsets, np.int64))
        self.len = [int(x) for x in lens]
        self.cap = [int(x) for x in capacity(lens)]
        self.ids, self.rows = [], []
        for l, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
            i = np.zeros(self.cap[l], np.uint32)
            r = np.zeros((self.cap[l], self.cs), np.uint8)
            i[:hi - lo] = ids[lo:hi]
            r[:hi - lo, :self.cb] = raw[lo:hi]
            self.ids.append(i)
            self.rows.append(r)

    def compact(self, del_ids, mutant=None):
        stored = np.concatenate([self.ids[l][:self.len[l]] for l in range(len(self.len))])
        rem = np.intersect1d(np.unique(np.asarray(del_ids, np.uint32)), stored)
        nw = self.cs // 4
        for l in range(len(self.len)):
            lid, lcode = self.ids[l], self.rows[l].view(np.uint32)      # (cap, nw) dwords
            wr = total = 0
            for c0 in range(0, self.len[l], CHUNK):
                p = np.arange(c0, min(c0 + CHUNK, self.len[l]))
                pid = lid[p].copy()
                lb = np.searchsorted(rem, pid, side="left")
                keep = ~((lb < len(rem)) & (rem[np.minimum(lb, max(len(rem) - 1, 0))] == pid)) if len(rem) else np.ones(len(p), bool)
                dst = wr + np.cumsum(keep) - 1
                low = lb.astype(np.uint32)
                if mutant == "ids_lowered_in_first_chunk_only" and c0 > 0:
                    low = np.zeros_like(low)
                lid[dst[keep]] = pid[keep] - low[keep]
                for wd in range(nw):
                    v = lcode[p, wd].copy()
                    if mutant == "second_column_from_destination" and wd == 1:
                        v = lcode[np.maximum(dst, 0), wd].copy()
                    lcode[dst[keep], wd] = v[keep]
                total = int(keep.sum())
                wr += total
            self.len[l] = total if mutant == "length_of_last_chunk" else wr

    def append(self, lst, new_codes, new_ids, mutant=None):
        raw = np.ascontiguousarray(new_codes).view(np.uint8).reshape(len(lst), -1)
        step = self.cb if mutant == "append_at_len_times_cb" else self.cs
        for i, l in enumerate(np.asarray(lst, np.int64)):
            assert self.len[l] < self.cap[l], "the model appends in place only"
            flat = self.rows[l].reshape(-1)
            flat[self.len[l] * step: self.len[l] * step + self.cb] = raw[i]
            self.ids[l][self.len[l]] = new_ids[i]
            self.len[l] += 1

    def arrays(self):
        offsets = np.zeros(len(self.len) + 1, np.int64)
        np.cumsum(self.len, out=offsets[1:])
        ids = np.concatenate([self.ids[l][:self.len[l]] for l in range(len(self.len))]).astype(np.uint32)
        raw = np.concatenate([self.rows[l][:self.len[l], :self.cb] for l in range(len(self.len))])
        codes = np.ascontiguousarray(raw).view(self.code_dtype).reshape(-1, self.m)
        return offsets, codes, ids


def mutant_applies(mutant, stride):
    """A mutant is a different program only where the stride lets it be: the second dword column needs cs >= 8, the cb / cs
    mix-up needs cb != cs -- and, to give the reference valid codes to read, UInt8 labels that cover every byte value."""
    cb = code_bytes(stride)
    if mutant == "second_column_from_destination":
        return cb > 4
    if mutant == "append_at_len_times_cb":
        return cb % 4 != 0 and STRIDES[stride][0] == 8
    return True


def append_batch(ref, seed, n):
    """n seeded points spread over the cells of `ref`, with the reference's own encoding of them: (pts, lists, codes)."""
    rng = np.random.default_rng(seed)
    pts = (ref.centroids[rng.integers(0, ref.kc, n)] + np.float32(0.05) * rng.standard_normal((n, ref.d))).astype(np.float32)
    lst, codes = ref_encode(ref, pts)
    return pts, lst, codes


def run_mutant(stride, mutant):
    """(reference, lists the kernels should leave, lists the mutant leaves) on the `chunks` geometry: see run_mutant_on."""
    return run_mutant_on(chunks_case(stride)[0], mutant)


def run_mutant_on(ref, mutant, dele=None):
    """"every other point" deleted, then a batch appended into the freed room -- the first mutations of the GPU file's chained test --
    by the kernels as they should be and by the mutant."""
    good, bad = DeviceModel(*lists_of(ref)), DeviceModel(*lists_of(ref))
    if dele is None:
        dele = pattern_ids("every_other", ref.offsets, ref.ids)
    good.compact(dele)
    bad.compact(dele, mutant)
    _, lst, codes = append_batch(ref, 4242, 40)
    new_ids = np.arange(40, dtype=np.uint32) + np.uint32(sum(good.len))
    good.append(lst, codes, new_ids)
    bad.append(lst, codes, new_ids, mutant)
    return ref, good.arrays(), bad.arrays()


def same_answer(a, b):
    """Two (ids, dists, counts) results identical over their first `count` slots, bit for bit."""
    try:
        helpers.assert_same_results(a, b)
    except AssertionError:
        return False
    return True


def pre_existing_check_sees(ref, good, bad):
    """Would the checks the suite had before the read-back have told `bad` lists from `good` ones?  Those checks: 48 queries at
    K = 10 / w = 5 and K = 4 / w = kc (verify() of test_delete_pop_pushfirst_in_place_on_device)."""
    qs = np.random.default_rng(610).random((48, ref.d), dtype=np.float32)
    rg, rb = ref_with_lists(ref, *good), ref_with_lists(ref, *bad)
    return any(not same_answer(ref_knn(rb, qs, K, w), ref_knn(rg, qs, K, w)) for K, w in ((10, 5), (4, ref.kc)))
