"""Numpy restatement of knn_search / _encode_point for UInt16 codes (tests only).

Float32 throughout, the reference's order: coarse distances summed in ascending dimension, top-w by (distance, cluster id)
(coarsequantizers.jl:33-37), tables sum_t (cb - r)^2 in ascending t (index.jl:232-236), sums dc + tab[0] + tab[1] + ... in
ascending sub-space (index.jl:240-246), the K smallest (distance, visit order) keys (index.jl:247-257).  Codes are LABELS, as the
reference stores them; tables are indexed through each block's label -> codeword map."""
import numpy as np

f32 = np.float32


class U16Index:
    def __init__(self, centroids, codebooks, labels, offsets, codes, ids):
        self.centroids = np.ascontiguousarray(centroids, f32)
        self.codebooks = np.ascontiguousarray(codebooks, f32)
        self.labels = np.ascontiguousarray(labels, np.uint16)
        self.offsets = np.ascontiguousarray(offsets, np.int64)
        self.codes = np.ascontiguousarray(codes, np.uint16).reshape(-1, self.codebooks.shape[0])
        self.ids = np.ascontiguousarray(ids, np.uint32)
        self.kc, self.d = self.centroids.shape
        self.m, self.ksub, self.dsub = self.codebooks.shape
        self.inv = np.full((self.m, 65536), -1, np.int64)
        for i in range(self.m):
            self.inv[i, self.labels[i]] = np.arange(self.ksub)


def coarse(ix, q, w):
    acc = np.zeros(ix.kc, f32)
    for i in range(ix.d):
        t = ix.centroids[:, i] - q[i]
        acc = acc + t * t
    order = np.lexsort((np.arange(ix.kc), acc))[:min(w, ix.kc)]
    return order, acc


def tables(ix, r):
    tab = np.zeros((ix.m, ix.ksub), f32)
    for i in range(ix.m):
        s = np.zeros(ix.ksub, f32)
        for t in range(ix.dsub):
            df = ix.codebooks[i, :, t] - r[i * ix.dsub + t]
            s = s + df * df
        tab[i] = s
    return tab


def knn_one(ix, q, K, w):
    q = np.asarray(q, f32)
    order, acc = coarse(ix, q, w)
    cand_d, cand_id = [], []
    for cl in order:
        lo, hi = int(ix.offsets[cl]), int(ix.offsets[cl + 1])
        dd = np.full(hi - lo, acc[cl], f32)
        if hi > lo:
            tab = tables(ix, q - ix.centroids[cl])
            for ii in range(ix.m):
                dd = dd + tab[ii, ix.inv[ii, ix.codes[lo:hi, ii]]]
        cand_d.append(dd)
        cand_id.append(ix.ids[lo:hi])
    cd = np.concatenate(cand_d)
    ci = np.concatenate(cand_id)
    sel = np.lexsort((np.arange(cd.shape[0]), cd))[:K]
    return ci[sel], cd[sel]


def knn(ix, Q, K, w):
    """(ids (nq, K) uint32, dists (nq, K) float32, counts (nq,) int32) as the search entries return them."""
    Q = np.asarray(Q, f32).reshape(-1, ix.d)
    ids = np.zeros((Q.shape[0], K), np.uint32)
    dists = np.zeros((Q.shape[0], K), f32)
    cnt = np.zeros(Q.shape[0], np.int32)
    for r in range(Q.shape[0]):
        i, dd = knn_one(ix, Q[r], K, w)
        cnt[r] = len(i)
        ids[r, :len(i)] = i
        dists[r, :len(i)] = dd
    return ids, dists, cnt


def encode(ix, pts):
    """_encode_point: nearest centroid (first minimum), then per sub-space the first codeword of smallest distance; codes are labels."""
    pts = np.asarray(pts, f32).reshape(-1, ix.d)
    lst = np.zeros(pts.shape[0], np.int32)
    codes = np.zeros((pts.shape[0], ix.m), np.uint16)
    for p in range(pts.shape[0]):
        order, _ = coarse(ix, pts[p], 1)
        lst[p] = order[0]
        r = pts[p] - ix.centroids[order[0]]
        tab = tables(ix, r)
        codes[p] = ix.labels[np.arange(ix.m), np.argmin(tab, axis=1)]
    return lst, codes


def make_index(seed, n, d, kc, m, ksub, perm_labels=True, empty_every=0, ndistinct=0, scale=0.25, centroids=None, list_sizes=None):
    """Random quantizers, random list assignment and codes (labels; `ndistinct` > 0: only that many code rows -> exact ties; 1: every
    point has the same code row), ids a permutation.  empty_every > 0: every such list is left empty.  `centroids` (kc, d): used
    instead of random ones; `list_sizes` (kc,): exact list lengths instead of a random assignment (n is then their sum)."""
    rng = np.random.default_rng(seed)
    dsub = d // m
    cent = rng.random((kc, d), dtype=f32)
    if centroids is not None:
        cent = np.ascontiguousarray(centroids, f32).reshape(kc, d)
    cbs = ((rng.random((m, ksub, dsub), dtype=f32) - 0.5) * 2 * scale).astype(f32)
    if perm_labels:
        labels = np.stack([rng.permutation(65536)[:ksub] for _ in range(m)]).astype(np.uint16)
    else:
        labels = np.tile(np.arange(ksub, dtype=np.uint16), (m, 1))
    lists = np.arange(kc) if not empty_every else np.array([l for l in range(kc) if l % empty_every])
    lst = lists[rng.integers(0, len(lists), n)]
    if list_sizes is not None:
        lst = rng.permutation(np.repeat(np.arange(kc), np.asarray(list_sizes, np.int64)))
        n = lst.shape[0]
    if ndistinct:
        pool = np.stack([labels[i][rng.integers(0, ksub, ndistinct)] for i in range(m)], 1)
        codes = pool[rng.integers(0, ndistinct, n)]
    else:
        codes = np.stack([labels[i][rng.integers(0, ksub, n)] for i in range(m)], 1)
    order = np.argsort(lst, kind="stable")
    offsets = np.zeros(kc + 1, np.int64)
    np.cumsum(np.bincount(lst, minlength=kc), out=offsets[1:])
    ids = rng.permutation(n).astype(np.uint32)
    return U16Index(cent, cbs, labels, offsets, codes[order].astype(np.uint16), ids)


def assert_exact(got, exp, what=""):
    """(ids, dists, counts) of a search entry against the reference (or another entry): counts, ids and distance bits identical."""
    gi, gd, gc = got
    ei, ed, ec = exp
    assert np.array_equal(gc, ec), "%s counts %s vs %s" % (what, gc[:8], ec[:8])
    for r in range(gc.shape[0]):
        c = int(gc[r])
        assert np.array_equal(gi[r, :c], ei[r, :c]), "%s ids differ at query %d: %s vs %s" % (what, r, gi[r, :c], ei[r, :c])
        assert np.array_equal(gd[r, :c].view(np.uint32), ed[r, :c].view(np.uint32)), "%s dists differ at query %d" % (what, r)
