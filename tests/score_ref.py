"""Support for the score tests (tests/test_score_model.py on the CPU, tests/test_gpu_score.py on the GPU); not a test.

The contract of ivfadc_score_ids (include/ivfadc_hip.h) as a numpy model, written from the four lines of the contract and not from the
oracle's search loop: for query q and candidate id v with (l, p) = locate(v) (reconstruct_ref: the last list that holds v, the first
position within it, nothing at or behind list_len), in Float32 with one rounding per operation,

    dc = 0;   t ascending:                 u = C_l[t] - q[t];          dc = dc + u * u
    r[t] = q[t] - C_l[t]
    s_ii = 0; t of sub-space ii ascending: u = CB_ii[c_ii][t] - r[t];  s_ii = s_ii + u * u
    dist = dc; ii ascending:               dist = dist + s_ii

c_ii the codeword the stored code (a LABEL) names.  An absent id: +Inf, found = 0.  A slot at or behind counts[q]: the same, and its id is
not looked at.  ids (C,) is ONE shared row scored against every query; ids (nq, C) is a row per query.

numpy's elementwise Float32 operations round once each, so the chains are vectorised ACROSS pairs and sequential along t and ii.

MUTANTS are the twelve wrong implementations the case table must tell from the model (tests/test_score_model.py).  `case_table()` builds
the cases both test files walk, each once: the shapes of the kernel's paths (16-byte and scalar row loads, both code widths, code strides
8 and 4, ksub = 2 and 256 with permuted labels, ksub = 300 in 16 bits) on rounding-hostile quantizers and queries in the manner of
helpers.build_stress_index (graded sub-space magnitudes in both directions, sums dominated by dc, exact hits)."""
import functools

import numpy as np

import reconstruct_ref as rr

f32, f64 = np.float32, np.float64
INF_BITS = 0x7F800000
MUTANTS = ("fma", "dc_last", "reversed", "pairwise", "reconstruct", "f64", "first_list", "to_capacity", "absent_zero", "counts_ignored",
           "label_as_index", "shared_stride_c")
KINDS = ("uniform", "graded", "graded_reversed", "dc_dominant", "exact_hits")
EDGE_C = (1, 63, 64, 65, 257)


def _fma(a, b, c):
    """fl32(a * b + c): the product of two Float32 is exact in float64"""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def _sq_chain(acc, u, mutant):
    return _fma(u, u, acc) if mutant == "fma" else acc + u * u


def pair_distances(qz, q, lists, cw, mutant=None):
    """The distances of query q (d,) to n entries: lists (n,) their lists, cw (n, m) the codeword index of every sub-space."""
    q = np.asarray(q, f32)
    n = len(lists)
    cent = qz.centroids[lists]                                                     # (n, d)
    words = qz.codebooks[np.arange(qz.m)[None, :], cw].reshape(n, qz.d)            # (n, d): the concatenated codewords
    if mutant == "reconstruct":                                                    # || q - (centre + codewords) ||^2
        x = cent + words
        acc = np.zeros(n, f32)
        for t in range(qz.d):
            u = q[t] - x[:, t]
            acc = acc + u * u
        return acc
    dc = np.zeros(n, f32)
    for t in range(qz.d):
        u = cent[:, t] - q[t]
        dc = _sq_chain(dc, u, mutant)
    r = q[None, :] - cent
    sums = []
    for ii in range(qz.m):
        ts = range(ii * qz.dsub, (ii + 1) * qz.dsub)
        if mutant == "f64":                                                        # the table entry in float64, rounded at the end
            s = np.zeros(n, f64)
            for t in ts:
                u = words[:, t].astype(f64) - r[:, t].astype(f64)
                s = s + u * u
            s = s.astype(f32)
        elif mutant == "pairwise":
            terms = []
            for t in ts:
                u = words[:, t] - r[:, t]
                terms.append(u * u)
            while len(terms) > 1:
                terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
            s = terms[0]
        else:
            s = np.zeros(n, f32)
            for t in ts:
                u = words[:, t] - r[:, t]
                s = _sq_chain(s, u, mutant)
        sums.append(s)
    if mutant == "dc_last":
        dist = np.zeros(n, f32)
        for s in sums:
            dist = dist + s
        return dist + dc
    dist = dc.copy()
    for s in (sums[::-1] if mutant == "reversed" else sums):
        dist = dist + s
    return dist


def _locate_all(st, uniq, mutant):
    loc_mut = mutant if mutant in ("first_list", "to_capacity") else None
    return {int(v): rr._locate_one(st, int(v), loc_mut)[:2] for v in uniq}


def score(st, qz, queries, ids, counts=None, mutant=None):
    """(dists (nq, C) float32, found (nq, C) bool) of the model, or of one of MUTANTS."""
    queries = np.asarray(queries, f32).reshape(-1, qz.d)
    nq = queries.shape[0]
    ids = np.asarray(ids, np.uint32)
    shared = ids.ndim == 1
    C = ids.shape[-1]
    if shared and mutant == "shared_stride_c":
        # row q read at q * C: behind the one row there is nothing of the caller's; whatever is read there is no stored id here
        rows = np.full((nq, C), 0xFFFFFFFE, np.uint32)
        rows[0] = ids
    else:
        rows = np.broadcast_to(ids, (nq, C)) if shared else ids
    live = np.full(nq, C, np.int64) if counts is None or mutant == "counts_ignored" else np.clip(np.asarray(counts, np.int64), 0, C)
    dists = np.full((nq, C), np.inf, f32)
    found = np.zeros((nq, C), bool)
    wanted = np.unique(np.concatenate([rows[q, :live[q]] for q in range(nq)])) if nq else np.zeros(0, np.uint32)
    loc = _locate_all(st, wanted, mutant)
    for q in range(nq):
        slots, lists, cw = [], [], []
        for j in range(int(live[q])):
            l, p = loc[int(rows[q, j])]
            if l < 0:
                continue
            row = st.rows[l][p]
            if mutant == "label_as_index":
                c = np.minimum(row.astype(np.int64), qz.ksub - 1)
            else:
                c = qz.inv[np.arange(qz.m), row]
                assert (c >= 0).all(), "a live row holds a code that is no label"
            slots.append(j)
            lists.append(l)
            cw.append(c)
        if slots:
            dists[q, slots] = pair_distances(qz, queries[q], np.array(lists), np.array(cw), mutant)
            found[q, slots] = True
    if mutant == "absent_zero":
        dists[~found] = f32(0.0)
    return dists, found


def same_answer(a, b):
    return np.array_equal(a[1], b[1]) and rr.same_bits(a[0], b[0])


def first_difference(got, exp, ids):
    """None, or a sentence naming the first pair on which (dists, found) differ."""
    gd, gf = got
    ed, ef = exp
    bad = np.argwhere((np.ascontiguousarray(gd, f32).view(np.uint32) != np.ascontiguousarray(ed, f32).view(np.uint32)) | (gf != ef))
    if not len(bad):
        return None
    q, j = (int(x) for x in bad[0])
    v = int(ids[j] if np.ndim(ids) == 1 else ids[q, j])
    return "query %d, slot %d (id %d): %s / found %d, expected %s / found %d; %d of %d pairs differ" % (
        q, j, v, float(gd[q, j]).hex(), gf[q, j], float(ed[q, j]).hex(), ef[q, j], len(bad), gd.size)


# ---- the case table -------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, kind, qz, st, queries, notes=()):
        self.name, self.kind, self.qz, self.st, self.queries, self.notes = name, kind, qz, st, queries, tuple(notes)
        self.u16 = qz.labels.dtype == np.uint16

    def stored_ids(self):
        return np.concatenate([self.st.ids[l][:self.st.len[l]] for l in range(len(self.st.len))]).astype(np.uint32)

    def absent_ids(self, n):
        stored = self.stored_ids().astype(np.int64)
        pool = np.concatenate([np.array(rr.SPECIAL_IDS, np.int64), len(stored) + 7 + 3 * np.arange(n + 8)])      # 0xFFFFFFFF first
        return pool[~np.isin(pool, stored)][:n].astype(np.uint32)

    def rows(self, C, seed=0, nq=None):
        """(nq, C) candidate rows: stored ids with repeats, a few absent ones and 0xFFFFFFFF, shuffled."""
        nq = len(self.queries) if nq is None else nq
        rng = np.random.default_rng(9100 + 31 * C + seed)
        stored = self.stored_ids()
        out = stored[rng.integers(0, len(stored), (nq, C))]
        if C >= 4:
            absent = self.absent_ids(max(2, C // 8))
            for q in range(nq):
                out[q, rng.choice(C, len(absent), replace=False)] = absent
                a, b = rng.choice(C, 2, replace=False)
                out[q, a] = out[q, b]                                            # a repeat for certain
        return np.ascontiguousarray(out, np.uint32)

    def ragged_counts(self, C, nq=None):
        """one count per query: a zero, C itself and values in between"""
        nq = len(self.queries) if nq is None else nq
        return np.array([(0, C, C // 2, max(C - 1, 0), 1)[q % 5] for q in range(nq)], np.int32)


def _grade(m, reverse):
    e = np.round(12.0 * np.arange(m) / max(m - 1, 1)).astype(np.int64)
    return e[::-1].copy() if reverse else e


def make_case(name, kind, seed, d, m, ksub, kc, n, bits=8, label_perm=False, nq=6):
    """A reconstruct_ref case (random lists, codes and unique shuffled ids) whose quantizers and queries are made rounding-hostile."""
    base = rr.make_case(name, seed, d, m, ksub, rr.random_lens(seed, n, kc), bits=bits, label_perm=label_perm)
    qz, st = base.qz, base.st
    rng = np.random.default_rng(seed + 77)
    qs = rng.random((nq, d), dtype=f32)
    dsub = d // m
    if kind.startswith("graded"):
        sc = np.ldexp(f32(1.0), -_grade(m, kind.endswith("reversed"))).astype(f32)
        qz.codebooks *= sc[:, None, None]
        qz.centroids *= np.repeat(sc, dsub)[None, :]
        qs *= np.repeat(sc, dsub)[None, :]
    elif kind == "dc_dominant":
        off = f32(300.0 if seed % 2 == 0 else 5000.0)
        qz.centroids += off
        qs[: nq // 2] += off
    elif kind == "exact_hits":
        qz.codebooks *= f32(2.0 ** -10)
        off, codes, _ = st.arrays()
        lists = np.repeat(np.arange(kc), np.diff(off))
        for i in range(nq):                                                      # every query AT a stored point's quantization
            e = int(rng.integers(0, len(lists)))
            c = qz.inv[np.arange(m), codes[e]]
            qs[i] = qz.centroids[lists[e]] + qz.codebooks[np.arange(m), c].reshape(d)
    else:
        assert kind == "uniform", kind
    return Case(name, kind, qz, st, np.ascontiguousarray(qs, f32), base.notes)


# name -> (kind, seed, d, m, ksub, kc, n, bits, label_perm): the shapes of the issue's table and the hostile kinds spread over them
SHAPES = {
    "d32_m8": ("graded", 7101, 32, 8, 256, 7, 300, 8, True),                     # dsub = 4: 16-byte loads throughout; code stride 8
    "d10_m2": ("dc_dominant", 7102, 10, 2, 256, 7, 300, 8, False),               # 40-byte rows: no 16-byte alignment; code stride 4
    "d6_m1": ("uniform", 7103, 6, 1, 256, 7, 300, 8, False),                     # one sub-space
    "d96_m16": ("graded_reversed", 7104, 96, 16, 256, 7, 300, 8, False),         # 16-byte centre rows, scalar codewords (dsub = 6)
    "d128_m8": ("exact_hits", 7105, 128, 8, 256, 7, 300, 8, False),              # dsub = 16
    "d768_m48": ("dc_dominant", 7107, 768, 48, 256, 4, 200, 8, False),           # kc = 4
    "ksub2": ("graded", 7108, 32, 8, 2, 7, 300, 8, True),
    "m3": ("exact_hits", 7109, 24, 3, 256, 7, 300, 8, True),                     # code stride 4, three bytes used
    "u16": ("graded", 7110, 32, 8, 300, 7, 300, 16, True),
    "u16_m2": ("uniform", 7111, 10, 2, 300, 7, 300, 16, False),                  # 16-bit codes, stride 4, scalar loads
}


@functools.lru_cache(maxsize=None)
def case_table():
    """name -> Case.  Built once and left unchanged by everyone."""
    cases = {name: make_case(name, *row[:7], bits=row[7], label_perm=row[8]) for name, row in SHAPES.items()}
    # stored ids repeated within a list and across lists (reconstruct_ref's case), under uniform queries
    dup = rr.make_case("duplicates", 7120, 24, 8, 256, rr.CASE_LENS, duplicates=True)
    cases["duplicates"] = Case("duplicates", "uniform", dup.qz, dup.st, np.random.default_rng(7121).random((6, 24), dtype=f32), dup.notes)
    return cases
