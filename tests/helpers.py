"""Shared test helpers: seeded index builders and an independent numpy restatement used to
cross-check the C oracle (tests only)."""
import numpy as np

from oracle import oracle as ora


def make_quantizers(seed, d, kc, m, ksub, label_perm=False, scale=0.25):
    rng = np.random.default_rng(seed)
    dsub = d // m
    cent = rng.random((kc, d), dtype=np.float32)
    cbs = ((rng.random((m, ksub, dsub), dtype=np.float32) - 0.5) * 2 * scale).astype(np.float32)
    if label_perm:
        labels = np.stack([rng.permutation(256)[:ksub].astype(np.uint8) for _ in range(m)])
    else:
        labels = np.tile(np.arange(ksub, dtype=np.uint8), (m, 1))
    return cent, cbs, labels


def build_index(seed, n, d, kc, m, ksub=256, label_perm=False, mode="encode", ndistinct=None, shuffle_ids=True):
    """Returns (OracleIndex, data).  mode: 'encode' = lists/codes from the oracle's _encode_point;
    'random' = random list assignment and random codes (optionally only `ndistinct` different
    codes -> many exact distance ties)."""
    rng = np.random.default_rng(seed + 1000)
    cent, cbs, labels = make_quantizers(seed, d, kc, m, ksub, label_perm)
    data = rng.random((n, d), dtype=np.float32)
    tmp = ora.OracleIndex(cent, cbs, labels, np.zeros(kc + 1, np.int64), np.zeros((0, m), np.uint8), np.zeros(0, np.uint32))
    if mode == "encode":
        lst, codes = tmp.encode(data) if n else (np.zeros(0, np.int32), np.zeros((0, m), np.uint8))
    else:
        lst = rng.integers(0, kc, n).astype(np.int32)
        if ndistinct:
            pool = np.stack([labels[i][rng.integers(0, ksub, ndistinct)] for i in range(m)], 1)   # (ndistinct, m)
            codes = pool[rng.integers(0, ndistinct, n)]
        else:
            codes = np.stack([labels[i][rng.integers(0, ksub, n)] for i in range(m)], 1).astype(np.uint8)
    order = np.argsort(lst, kind="stable")
    ids = order.astype(np.uint32)            # id = original position, ascending within a list
    if shuffle_ids and mode != "encode":
        ids = rng.permutation(n).astype(np.uint32)
    offsets = np.zeros(kc + 1, np.int64)
    np.cumsum(np.bincount(lst, minlength=kc), out=offsets[1:])
    oidx = ora.OracleIndex(cent, cbs, labels, offsets, np.ascontiguousarray(codes[order]), ids)
    return oidx, data


def ref_coarse(oidx, q):
    """Coarse distances of one query in the reference's order: ascending dimension, sub / mul / add, one rounding each."""
    acc = np.zeros(oidx.kc, np.float32)
    for i in range(oidx.d):
        t = oidx.centroids[:, i] - q[i]
        acc = acc + t * t
    return acc


def ref_table(oidx, i, r):
    """Table row of sub-space i for residual r (all ksub codewords) in the reference's order: ascending t."""
    s = np.zeros(oidx.ksub, np.float32)
    for t_ in range(oidx.dsub):
        df = oidx.codebooks[i, :, t_] - r[i * oidx.dsub + t_]
        s = s + df * df
    return s


def ref_adc(dc, terms):
    """ADC sums of one list in the reference's order: dc, then t0 .. t(m-1).  terms: m arrays, one entry per point."""
    dd = np.full(terms[0].shape[0], dc, np.float32)
    for t in terms:
        dd = dd + t
    return dd


def numpy_knn(oidx, q, K, w, coarse=ref_coarse, table=ref_table, adc=ref_adc):
    """Independent restatement: exhaustive (dist, visit order) list, then a lexicographic sort.
    float32 throughout, sums sequential in ascending index (elementwise numpy ops round once).
    coarse / table / adc: the three sums, replaceable so that tests/test_parity_power.py can restate the ways a kernel goes
    subtly wrong; the defaults are the reference's."""
    f32 = np.float32
    q = np.asarray(q, f32)
    w = min(w, oidx.kc)
    acc = coarse(oidx, q)
    order = np.lexsort((np.arange(oidx.kc), acc))[:w]
    cand_d, cand_id = [], []
    for j, cl in enumerate(order):
        dc = acc[cl]
        r = q - oidx.centroids[cl]
        lo, hi = int(oidx.offsets[cl]), int(oidx.offsets[cl + 1])
        if hi > lo:
            tab = np.zeros((oidx.m, 256), f32)
            for i in range(oidx.m):
                tab[i, oidx.labels[i]] = table(oidx, i, r)
            cand_d.append(adc(dc, [tab[ii, oidx.codes[lo:hi, ii]] for ii in range(oidx.m)]))
            cand_id.append(oidx.ids[lo:hi])
    cd = np.concatenate(cand_d) if cand_d else np.zeros(0, f32)
    ci = np.concatenate(cand_id) if cand_id else np.zeros(0, np.uint32)
    sel = np.lexsort((np.arange(cd.shape[0]), cd))[:K]
    return ci[sel], cd[sel]


def numpy_knn_batch(oidx, qs, K, w, **sums):
    """numpy_knn over a batch, in the (ids, dists, counts) form the search entries and the oracle return."""
    qs = np.asarray(qs, np.float32).reshape(-1, oidx.d)
    ids = np.zeros((qs.shape[0], K), np.uint32)
    dists = np.full((qs.shape[0], K), np.inf, np.float32)
    counts = np.zeros(qs.shape[0], np.int32)
    for r in range(qs.shape[0]):
        i, dd = numpy_knn(oidx, qs[r], K, w, **sums)
        counts[r] = len(i)
        ids[r, :len(i)] = i
        dists[r, :len(i)] = dd
    return ids, dists, counts


# ---- rounding-hostile inputs (tests/test_gpu_bitwise.py; tests/test_parity_power.py shows on the CPU that each of them tells the
# reference's order from every restated mistake) ---------------------------------------------------------------------------------
STRESS_KINDS = ("uniform", "graded", "graded_reversed", "dc_dominant", "exact_hits")


def _grade(m, reverse):
    """Exponents e_i: sub-space i is scaled by 2^-e_i, falling across 2^12 over the m sub-spaces (rising when reversed)."""
    e = np.round(12.0 * np.arange(m) / max(m - 1, 1)).astype(np.int64)
    return e[::-1].copy() if reverse else e


def build_stress_index(kind, seed, n, d, kc, m, ksub=256, nq=64, label_perm=False):
    """(OracleIndex, queries) on top of build_index (random lists and codes), seeded.
    uniform:          build_index's data as it is, uniform queries.
    graded[_reversed]: sub-quantizer i's codebook -- and the matching dimensions of centroids and queries, so that the residuals
                      keep the codebook's scale -- times 2^-e_i, e_i from 0 to 12 over the m sub-spaces (reversed: 12 to 0).  Powers
                      of two: every entry is the uniform one's times 4^-e_i exactly, and which entries a sum absorbs depends on the
                      order of the additions.
    dc_dominant:      centroids carry a common offset of 300 (seed even) or 5000 (seed odd); half of the queries carry it too
                      (residuals are differences of large numbers), half do not (dc and every entry are huge, dc largest).
    exact_hits:       codebooks times 2^-10 and every query at centroid + codewords: dc is tiny, the hit's entries are 0 up to the
                      rounding of the residual, every sum of the nearest list is tiny."""
    assert kind in STRESS_KINDS, kind
    oidx, _ = build_index(seed, n, d, kc, m, ksub, label_perm=label_perm, mode="random")
    rng = np.random.default_rng(seed + 77)
    qs = rng.random((nq, d), dtype=np.float32)
    dsub = d // m
    if kind.startswith("graded"):
        sc = np.ldexp(np.float32(1.0), -_grade(m, kind.endswith("reversed"))).astype(np.float32)
        oidx.codebooks *= sc[:, None, None]
        oidx.centroids *= np.repeat(sc, dsub)[None, :]
        qs *= np.repeat(sc, dsub)[None, :]
    elif kind == "dc_dominant":
        off = np.float32(300.0 if seed % 2 == 0 else 5000.0)
        oidx.centroids += off
        qs[: nq // 2] += off
    elif kind == "exact_hits":
        oidx.codebooks *= np.float32(2.0 ** -10)
        for i in range(nq):
            code = rng.integers(0, ksub, m)
            qs[i] = oidx.centroids[rng.integers(0, kc)] + np.concatenate([oidx.codebooks[ii, code[ii]] for ii in range(m)])
    return oidx, np.ascontiguousarray(qs, np.float32)


# the shapes tests/test_gpu_bitwise.py runs the kernel forms on: name -> (seed, n, d, kc, m, ksub, K, w)
BITWISE_SHAPES = {
    "m8": (9101, 40000, 128, 24, 8, 256, 10, 6),        # m = 8, dsub = 16: list-major 1/2/4, 16-bit integer filter, eight-wave, narrow-field
    "m16": (9102, 40000, 96, 24, 16, 256, 10, 6),       # m = 16, dsub = 6: striped filter, matrix-core lower-bound tables (padded k-step)
    "m48": (9103, 9000, 768, 24, 48, 256, 10, 8),       # m = 48, dsub = 16: matrix-core lower-bound tables
    "m10": (9104, 8000, 40, 40, 10, 64, 10, 5),         # generic-m kernel (dsub = 4), ksub < 256, permuted labels
    "kc2048": (9105, 30000, 64, 2048, 8, 256, 10, 16),  # a coarse problem large enough for every coarse mode
}


def _ulps(a, b):
    """Distance in units in the last place between two float32 values (monotone integer mapping of the bit patterns)."""
    def key(x):
        u = int(np.float32(x).view(np.uint32))
        return u if u < 0x80000000 else 0x80000000 - u
    return abs(key(a) - key(b))


def assert_same_results(got, exp, what=""):
    """(ids, dists, counts) of a search against the oracle's (or another search's): counts identical, ids identical over the first
    `count` slots, Float32 distances identical BIT FOR BIT over the same slots (README: every result's sum is the reference's:
    dc, then t0 .. t(m-1), one rounding per operation).  A failure names the query, the first differing slot, both values as
    float.hex and how many ulp they are apart."""
    gi, gd, gc = got
    ei, ed, ec = exp
    gd, ed = np.asarray(gd), np.asarray(ed)
    assert gd.dtype == np.float32 and ed.dtype == np.float32, "%s distances must be float32 arrays, got %s vs %s" % (what, gd.dtype, ed.dtype)
    assert np.array_equal(gc, ec), "%s counts differ: %s vs %s" % (what, np.asarray(gc)[:16], np.asarray(ec)[:16])
    for r in range(np.asarray(gc).shape[0]):
        c = int(gc[r])
        assert np.array_equal(gi[r, :c], ei[r, :c]), "%s ids differ at query %d: %s vs %s (d %s vs %s)" % (
            what, r, gi[r, :c], ei[r, :c], gd[r, :c], ed[r, :c])
        gb, eb = np.ascontiguousarray(gd[r, :c]).view(np.uint32), np.ascontiguousarray(ed[r, :c]).view(np.uint32)
        if not np.array_equal(gb, eb):
            bad = np.nonzero(gb != eb)[0]
            s = int(bad[0])
            raise AssertionError("%s distance bits differ at query %d, slot %d (id %d; %d of %d slots differ): got %s, expected %s, %d ulp apart" % (
                what, r, s, int(gi[r, s]), bad.shape[0], c, float(gd[r, s]).hex(), float(ed[r, s]).hex(), _ulps(gd[r, s], ed[r, s])))


def numpy_partial_keys(oidx, qs, K, w, nparts, part):
    """List-partitioned restatement: for every query the K smallest (distance, visit order) keys over the probed lists l with
    l % nparts == part -- visit orders counted over ALL w probes, as one rank of ivfadc_search_device_partial leaves them --
    plus the stored ids of those keys.  float32 throughout, sums sequential in ascending index."""
    f32 = np.float32
    qs = np.asarray(qs, f32)
    w = min(w, oidx.kc)
    nq = qs.shape[0]
    keys = np.full((nq, K), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    ids = np.zeros((nq, K), np.uint32)
    counts = np.zeros(nq, np.int32)
    for qi in range(nq):
        q = qs[qi]
        acc = np.zeros(oidx.kc, f32)
        for i in range(oidx.d):
            t = oidx.centroids[:, i] - q[i]
            acc = acc + t * t
        order = np.lexsort((np.arange(oidx.kc), acc))[:w]
        base = 0
        ck, ci = [], []
        for cl in order:
            lo, hi = int(oidx.offsets[cl]), int(oidx.offsets[cl + 1])
            if cl % nparts == part and hi > lo:
                r = q - oidx.centroids[cl]
                tab = np.zeros((oidx.m, 256), f32)
                for i in range(oidx.m):
                    s = np.zeros(oidx.ksub, f32)
                    for t_ in range(oidx.dsub):
                        df = oidx.codebooks[i, :, t_] - r[i * oidx.dsub + t_]
                        s = s + df * df
                    tab[i, oidx.labels[i]] = s
                dd = np.full(hi - lo, acc[cl], f32)
                for ii in range(oidx.m):
                    dd = dd + tab[ii, oidx.codes[lo:hi, ii]]
                ck.append((dd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (base + np.arange(hi - lo)).astype(np.uint64))
                ci.append(oidx.ids[lo:hi])
            base += hi - lo
        if ck:
            allk, alli = np.concatenate(ck), np.concatenate(ci)
            sel = np.argsort(allk, kind="stable")[:K]
            keys[qi, :len(sel)] = allk[sel]
            ids[qi, :len(sel)] = alli[sel]
            counts[qi] = len(sel)
    return keys, counts, ids
