"""Support for the locate / reconstruct tests (tests/test_reconstruct_model.py on the CPU, tests/test_gpu_reconstruct.py on the GPU); not a
test.

The contract of ivfadc_locate / ivfadc_reconstruct (include/ivfadc_hip.h) as a numpy model:

* a stored entry counts only below its list's length;
* locate(v) is what the loop of _pop! finds (utils.jl:49-55): the LAST list that holds v (no break: later lists overwrite) and the FIRST
  position of v within that list (findfirst); no list holds v: absent, (-1, -1);
* reconstruct(v) = centroid of that list + the concatenated codewords its stored codes name, one Float32 addition per component; the
  rotation of an :opq file is not applied; an absent id gives d floats +0.0 and found = 0;
* requests are answered slot by slot, in request order; ids are unsigned 32-bit numbers.

`Stored` holds the lists the way the device does -- per list `cap` id slots and code rows of which the first `len` count -- so that the
model and the wrong implementations (MUTANTS) can be told apart on what lies behind a list's end.  `case_table()` builds the cases both
files walk, each once."""
import functools

import numpy as np

f32 = np.float32
# one list per value, on both sides of a wave (64) and of a workgroup (256), plus five ordinary ones: kc = 13
EDGE_LENS = (0, 1, 63, 64, 65, 255, 256, 257)
CASE_LENS = EDGE_LENS + (3, 17, 40, 100, 71)
REQUEST_SIZES = (1, 2, 64, 65, 1000)
SPECIAL_IDS = (0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 0x80000001, 0x7FFFFFFF, 0)
MUTANTS = ("first_list", "last_position", "to_capacity", "label_as_index", "other_lists_centre", "sorted_request_order",
           "duplicates_once", "signed_ids")


class Stored:
    """Lists as the device holds them: ids[l] (cap,) uint32, rows[l] (cap, m) stored codes (LABELS), len[l] <= cap."""

    def __init__(self, ids, rows, lens):
        self.ids, self.rows, self.len = list(ids), list(rows), [int(x) for x in lens]

    @classmethod
    def from_lists(cls, offsets, codes, ids):
        offsets = np.asarray(offsets, np.int64)
        kc = len(offsets) - 1
        return cls([np.asarray(ids[offsets[l]:offsets[l + 1]], np.uint32) for l in range(kc)],
                   [np.asarray(codes[offsets[l]:offsets[l + 1]]) for l in range(kc)], np.diff(offsets))

    @classmethod
    def from_device_model(cls, model):
        """write_path.DeviceModel: every slot up to the capacity, stale rows included."""
        rows = [np.ascontiguousarray(model.rows[l][:, :model.cb]).view(model.code_dtype).reshape(-1, model.m) for l in range(len(model.len))]
        return cls([model.ids[l].copy() for l in range(len(model.len))], rows, model.len)

    def arrays(self):
        """(offsets, codes, ids) of the live part, the layout ivfadc_set_lists takes."""
        offsets = np.zeros(len(self.len) + 1, np.int64)
        np.cumsum(self.len, out=offsets[1:])
        ids = np.concatenate([self.ids[l][:self.len[l]] for l in range(len(self.len))]).astype(np.uint32)
        codes = np.concatenate([self.rows[l][:self.len[l]] for l in range(len(self.len))])
        return offsets, np.ascontiguousarray(codes), ids


class Quantizers:
    def __init__(self, centroids, codebooks, labels):
        self.centroids, self.codebooks, self.labels = np.asarray(centroids, f32), np.asarray(codebooks, f32), np.asarray(labels)
        self.kc, self.d = self.centroids.shape
        self.m, self.ksub, self.dsub = self.codebooks.shape
        self.inv = np.full((self.m, 1 << (8 * self.labels.dtype.itemsize)), -1, np.int64)        # label -> codeword index
        for i in range(self.m):
            self.inv[i, self.labels[i]] = np.arange(self.ksub)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _locate_one(st, v, mutant=None):
    """(list, position, list whose centre is used) of one id."""
    found = (-1, -1, -1)
    first = None
    for l in range(len(st.len)):
        reach = len(st.ids[l]) if mutant == "to_capacity" else st.len[l]
        hits = np.nonzero(st.ids[l][:reach] == np.uint32(v))[0]
        if hits.size:
            p = int(hits[-1] if mutant == "last_position" else hits[0])
            if first is None:
                first = (l, p, l)
            found = (l, p, first[0] if mutant == "other_lists_centre" else l)
    return first if mutant == "first_list" and first is not None else found


def _answer_slots(req, mutant):
    """For every request slot: which id it is answered for (None: left absent) -- the identity for the model."""
    req = [int(v) for v in np.asarray(req, np.uint32)]
    if mutant == "sorted_request_order":
        return sorted(req)
    if mutant == "duplicates_once":
        seen, out = set(), []
        for v in req:
            out.append(None if v in seen else v)
            seen.add(v)
        return out
    if mutant == "signed_ids":
        # wanted ids sorted as SIGNED numbers, then searched with unsigned comparisons: an id the search does not reach is absent
        want = np.array(sorted(set(req), key=lambda v: v - (1 << 32) if v >= (1 << 31) else v), np.uint32)
        out = []
        for v in req:
            a, b = 0, len(want)
            while a < b:
                mid = (a + b) // 2
                if int(want[mid]) < v:
                    a = mid + 1
                else:
                    b = mid
            out.append(v if a < len(want) and int(want[a]) == v else None)
        return out
    return req


def locate(st, req, mutant=None):
    """(lists (n,) int32, positions (n,) int64) in request order; -1 / -1 for an absent id."""
    ans = _answer_slots(req, mutant)
    lists, pos = np.full(len(ans), -1, np.int32), np.full(len(ans), -1, np.int64)
    memo = {}
    for j, v in enumerate(ans):
        if v is None:
            continue
        if v not in memo:
            memo[v] = _locate_one(st, v, mutant)
        lists[j], pos[j] = memo[v][0], memo[v][1]
    return lists, pos


def reconstruct(st, qz, req, mutant=None):
    """(vectors (n, d) float32, found (n,) bool) in request order."""
    ans = _answer_slots(req, mutant)
    vec, found = np.zeros((len(ans), qz.d), f32), np.zeros(len(ans), bool)
    for j, v in enumerate(ans):
        if v is None:
            continue
        l, p, lc = _locate_one(st, v, mutant)
        if l < 0:
            continue
        row = st.rows[l][p]
        if mutant == "label_as_index":
            c = np.minimum(row.astype(np.int64), qz.ksub - 1)
        else:
            c = qz.inv[np.arange(qz.m), row]
            assert (c >= 0).all(), "a live row holds a code that is no label"
        vec[j] = qz.centroids[lc] + qz.codebooks[np.arange(qz.m), c].reshape(qz.d)        # one Float32 addition per component
        found[j] = True
    return vec, found


def literal(st, qz, v):
    """utils.jl:41-81 word for word for one id that is stored (the reference asserts nothing about an absent one: it fails)."""
    cluster, idx, point_codes = 0, 0, None
    for i in range(len(st.len)):                                                       # for i = eachindex(ivfadc.inverse_index)
        idxs = [int(x) for x in st.ids[i][:st.len[i]]]
        if v in idxs:                                                                  # if vecid in idxs
            cluster = i
            idx = idxs.index(v)                                                        # findfirst(isequal(vecid), idxs)
            point_codes = st.rows[i][idx]
    residual = np.empty(qz.d, f32)                                                     # _decode_point
    for i in range(qz.m):
        residual[i * qz.dsub:(i + 1) * qz.dsub] = qz.codebooks[i][int(np.nonzero(qz.labels[i] == point_codes[i])[0][0])]
    return cluster, idx, qz.centroids[cluster] + residual


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, f32).view(np.uint32), np.ascontiguousarray(b, f32).view(np.uint32))


# ---- the case table -------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, qz, st, notes=()):
        self.name, self.qz, self.st, self.notes = name, qz, st, tuple(notes)
        self.u16 = qz.labels.dtype == np.uint16

    def stored_ids(self):
        return np.concatenate([self.st.ids[l][:self.st.len[l]] for l in range(len(self.st.len))]).astype(np.uint32)

    def requests(self, size, seed=0):
        """`size` ids: stored ones (with repeats once there is room), absent ones and the special values, shuffled -- never sorted."""
        rng = np.random.default_rng(4200 + 17 * size + seed)
        stored = self.stored_ids()
        absent = np.setdiff1d(np.array(SPECIAL_IDS + (len(stored) + 7, 123456789, 0x90000000), np.int64), stored.astype(np.int64))
        if size == 1:
            return stored[rng.integers(0, len(stored), 1)].astype(np.uint32)
        if size == 2:                                     # one stored, one absent, the larger first
            return np.array(sorted([int(stored[rng.integers(0, len(stored))]), int(absent[0])], reverse=True), np.uint32)
        n_abs = min(len(absent), max(1, size // 8))
        pick = stored[rng.integers(0, len(stored), size - n_abs - min(len(SPECIAL_IDS), size // 8))]          # with replacement: repeats
        pick[-3:] = pick[:3]                                                                                  # repeats for certain
        req = np.concatenate([pick.astype(np.int64), absent[:n_abs], np.array(SPECIAL_IDS[:min(len(SPECIAL_IDS), size // 8)], np.int64)])
        req = rng.permutation(req)
        if np.array_equal(req, np.sort(req)):
            req = req[::-1]
        return req.astype(np.uint32)


def make_quantizers(seed, d, kc, m, ksub, bits=8, label_perm=False, bit_patterns=False):
    rng = np.random.default_rng(seed)
    dsub = d // m
    cent = rng.random((kc, d), dtype=f32)
    cbs = ((rng.random((m, ksub, dsub), dtype=f32) - f32(0.5)) * f32(0.5)).astype(f32)
    if bits == 16:
        labels = np.stack([(rng.permutation(65536)[:ksub] if label_perm else np.arange(ksub)) for _ in range(m)]).astype(np.uint16)
    else:
        labels = np.stack([(rng.permutation(256)[:ksub] if label_perm else np.arange(ksub)) for _ in range(m)]).astype(np.uint8)
    if bit_patterns:
        # subnormal, signed-zero and large-magnitude components on both sides of the addition, in every combination that matters:
        # -0 + -0 = -0, -0 + +0 = +0, subnormal + subnormal, subnormal + -subnormal = +0, large + large, large + small
        pat = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-40, 5.9e-39, 1e38, -1.6e38, 1.5e38, 1.0], f32)          # (no sum overflows)
        cent[:, :] = pat[rng.integers(0, len(pat), cent.shape)]
        cbs[:, :, :] = pat[rng.integers(0, len(pat), cbs.shape)]
        cent[0, :4] = (-0.0, 1e-45, 1e-40, 1.5e38)
        cbs[0, 0, :min(dsub, 3)] = (-0.0, -1e-45, 1e-40)[:min(dsub, 3)]
    return Quantizers(cent, cbs, labels)


def make_case(name, seed, d, m, ksub, lens, bits=8, label_perm=False, special_ids=False, duplicates=False, bit_patterns=False):
    qz = make_quantizers(seed, d, len(lens), m, ksub, bits, label_perm, bit_patterns)
    rng = np.random.default_rng(seed + 500)
    offsets = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    n = int(offsets[-1])
    idx = rng.integers(0, ksub, (n, m))
    if bit_patterns:
        idx[0] = 0
    codes = np.stack([qz.labels[i][idx[:, i]] for i in range(m)], 1)
    ids = rng.permutation(n).astype(np.int64)
    if special_ids:
        ids += 1                                                      # (the only 0 is the special one)
        ids[rng.choice(n, len(SPECIAL_IDS), replace=False)] = SPECIAL_IDS
        up =rng.choice(np.nonzero(~np.isin(ids, SPECIAL_IDS))[0], n // 3, replace=False)
        ids[up] += 0x80000002                                         # a third of the ids in the upper half
    notes = []
    if duplicates:
        big = [l for l in range(len(lens)) if lens[l] >= 40]
        a, b, c = big[0], big[1], big[-1]
        # within one list: positions 5 and 30 of list a share an id; across lists: position 7 of list a, 3 of b and 9 and 20 of c share one
        ids[offsets[a] + 30] = ids[offsets[a] + 5]
        for l, p in ((b, 3), (c, 9), (c, 20)):
            ids[offsets[l] + p] = ids[offsets[a] + 7]
        notes = [("within", int(ids[offsets[a] + 5]), a, 5), ("across", int(ids[offsets[a] + 7]), c, 9)]
    return Case(name, qz, Stored.from_lists(offsets, codes, ids.astype(np.uint32)), notes)


def random_lens(seed, n, kc):
    """n points spread over kc lists at random (the base shape: an ordinary index)."""
    return np.bincount(np.random.default_rng(seed).integers(0, kc, n), minlength=kc).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case_table():
    """name -> Case.  Built once and left unchanged by everyone."""
    base = random_lens(1, 900, 13)
    cases = [
        make_case("m8", 11, 24, 8, 256, base),                                                  # code stride 8
        make_case("m3", 12, 24, 3, 256, base),                                                  # code stride 4, three bytes used
        make_case("dsub5", 13, 50, 10, 256, base),                                              # dsub no multiple of 4, d no multiple of 64
        make_case("u16", 14, 24, 8, 300, base, bits=16),
        make_case("perm8", 15, 24, 8, 200, base, label_perm=True),
        make_case("perm16", 16, 24, 3, 300, base, bits=16, label_perm=True),
        make_case("edge_lens", 17, 24, 8, 256, CASE_LENS, label_perm=True),
        make_case("upper_ids", 18, 24, 8, 256, CASE_LENS, special_ids=True),
        make_case("duplicates", 19, 24, 8, 256, CASE_LENS, duplicates=True),
        make_case("bit_patterns", 20, 24, 8, 256, base, bit_patterns=True),
    ]
    return {c.name: c for c in cases}
