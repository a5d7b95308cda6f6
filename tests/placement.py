"""Support for the placement tests (tests/test_placement_model.py on the CPU, tests/test_gpu_placement.py on the GPU); not a test.

Every scan kernel prunes with a bound whose proof counts over the kernel's own work decomposition (the largest of the P parts'
ceil(K/P)-th keys).  With codes drawn at random the K best points of a list are spread evenly over positions, waves,
steps, chunks and lanes, and every such bound is loose by a wide margin: a wrong rank, a minimum for a maximum or a bound kept through
the merge changes nothing.  Here the RANK of every row of a list is prescribed by position.  Three things live here:

* the placements: permutations pi of 0 .. L-1, rank r (by the designer query's (sum, pool index)) is stored at position pi[r].  Nothing
  about the values is special -- random codebooks, random code rows --, only where the rows stand.
* placed_case: one list per (placement, length) for the kinds of list_end.KINDS, eight queries per list (the designer query three
  times, three jittered copies, two unrelated queries that reach the list as a later probe), w = 3.
* model: "P parts scan disjoint positions, each with its own selector, under a shared bound, then merge" in numpy, with the geometry
  (granule, parts) as parameters, and MUTANTS, the ways this class of bound goes wrong.
"""
import bisect
import functools

import numpy as np

import list_end as le
import u16_ref
from oracle import oracle as ora

f32 = np.float32
W = le.W
QPL = le.QPL                 # queries per list: query r belongs to list r // QPL
KINDS = le.KINDS
LEN_LONG, LEN_SHORT = 6203, 299      # multiples of no granule: six 1024-point steps plus 59 points; below one 1024-point step
NTIED = 130
K_REG = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 57, 63, 64)       # register selectors, the eight-wave pool
K_WIDE = (65, 72, 73, 121, 127, 128)                               # the wide pool
K_LDS = (65, 100, 129, 192, 193)                                   # LDS selectors (four-wave K > 64, UInt16 wide)
K_ALL = tuple(sorted(set(K_REG + K_WIDE + K_LDS)))
KMAX = max(K_ALL)
# (granule, parts): a position p belongs to part (p // granule) % parts; parts None: one part per granule (the chunks of a list)
GEOMETRIES = ((64, 4), (256, 4), (256, 8), (1024, None), (2048, None))


# ---- the placements --------------------------------------------------------------------------------------------------------------
def _rest_shuffled(L, head, rng):
    """pi with ranks 0 .. len(head)-1 at the positions `head` and every further rank at a random one of the positions left."""
    head = np.asarray(head, np.int64)
    assert len(np.unique(head)) == len(head) and (head >= 0).all() and (head < L).all()
    free = np.setdiff1d(np.arange(L), head)
    return np.concatenate([head, rng.permutation(free)])


def ascending(L, rng=None):
    return np.arange(L)


def descending(L, rng=None):
    return L - 1 - np.arange(L)


def whole_granules(L, g):
    return L // g


def block(L, g, b, rng):
    """ranks 0 .. g-1 fill granule b (positions b g ..), the rest is shuffled: all winners in one wave / step / chunk"""
    assert 0 <= b < whole_granules(L, g)
    return _rest_shuffled(L, b * g + np.arange(g), rng)


def stride(L, g, c, rng, nranks=256):
    """rank r at position r g + c: one winner per granule.  Where r g + c >= L the ranks wrap: with G granules that hold position c,
    rank r stands in granule r % G at offset c + r // G."""
    G = len(range(c, L, g))
    r = np.arange(min(nranks, L))
    head = (r % G) * g + c + r // G
    head = head[head < L]
    _, first = np.unique(head, return_index=True)
    return _rest_shuffled(L, head[np.sort(first)], rng)


def lane(L, c, rng):
    """rank r at position 64 r + c: every winner in the same lane of its wave"""
    return stride(L, 64, c, rng)


def split(L, rng=None):
    """the even ranks from the front, the odd ranks from the back"""
    pi = np.zeros(L, np.int64)
    r = np.arange(L)
    pi[r % 2 == 0] = r[r % 2 == 0] // 2
    pi[r % 2 == 1] = L - 1 - r[r % 2 == 1] // 2
    return pi


def near_misses_first(L, rng):
    """ranks 128 .. 255 at positions 0 .. 127 in descending order, ranks 0 .. 127 in the last 128 positions, the rest between: the
    selectors fill with the closest losers, the bound sits one rank above the winners while they arrive, in the tail"""
    assert L >= 384
    head = np.concatenate([L - 128 + np.arange(128), 127 - np.arange(128)])
    return _rest_shuffled(L, head, rng)


def shuffled(L, rng):
    return rng.permutation(L)


def _mid(n):
    """a middle granule that is not the first of a group of four"""
    b = n // 2
    return b + 1 if b % 4 == 0 and b + 1 < n - 1 else b


def placements(L):
    """[(name, tied?, function(rng) -> pi)] of a list length"""
    out = [("ascending", False, lambda rng: ascending(L)), ("descending", False, lambda rng: descending(L)),
           ("split", False, lambda rng: split(L)), ("shuffled", False, lambda rng: shuffled(L, rng))]
    if L >= 384:
        out.append(("near_misses_first", False, lambda rng: near_misses_first(L, rng)))
    for g in (64, 256, 1024, 2048, 4096):
        n = whole_granules(L, g)
        for b in sorted({0, _mid(n), n - 1}) if n else ():
            out.append(("block(%d,%d)" % (g, b), False, lambda rng, g=g, b=b: block(L, g, b, rng)))
    for g, c in ((64, 0), (64, 37), (64, 58), (256, 5), (1024, 37), (2048, 41)):
        if g + c < L:
            out.append((("lane(%d)" % c) if g == 64 else "stride(%d,%d)" % (g, c), False, lambda rng, g=g, c=c: stride(L, g, c, rng)))
    # exact ties across the K boundary that only the visit order breaks
    n64, n256 = whole_granules(L, 64), whole_granules(L, 256)
    out.append(("tied(descending)", True, lambda rng: descending(L)))
    out.append(("tied(block(64,%d))" % (n64 - 1), True, lambda rng: block(L, 64, n64 - 1, rng)))
    if n256 > 1:
        out.append(("tied(block(256,%d))" % _mid(n256), True, lambda rng: block(L, 256, _mid(n256), rng)))
        out.append(("tied(block(1024,%d))" % (L // 1024 - 1), True, lambda rng: block(L, 1024, L // 1024 - 1, rng)))
        out.append(("tied(lane(37))", True, lambda rng: lane(L, 37, rng)))
    return out


# ---- the index -------------------------------------------------------------------------------------------------------------------
class Placed:
    """placed_case's result.  lists: [(placement name, length, pi)] in list order; ref, qs as in list_end.Case."""

    def __init__(self, kind, ref, qs, lists):
        self.kind, self.ref, self.qs, self.lists = kind, ref, qs, lists
        self.u16 = isinstance(ref, u16_ref.U16Index)
        self._sorted = None

    def designer(self, l):
        return l * QPL

    def what(self, r):
        name, L, _ = self.lists[r // QPL]
        return "query %d of list %d: %s, length %d" % (r, r // QPL, name, L)

    def with_lists(self, offsets, codes, ids):
        r = self.ref
        cls = u16_ref.U16Index if self.u16 else ora.OracleIndex
        return cls(r.centroids, r.codebooks, r.labels, offsets, codes, ids)


def _quantizers(kind, kc, rng):
    d, m, ksub, bits = KINDS[kind]
    cent = rng.random((kc, d), dtype=f32)
    cbs = ((rng.random((m, ksub, d // m), dtype=f32) - f32(0.5)) * f32(0.5)).astype(f32)
    if bits == 8:
        labels = np.stack([rng.permutation(256)[:ksub] for _ in range(m)]).astype(np.uint8)
    else:
        labels = np.stack([rng.permutation(65536)[:ksub] for _ in range(m)]).astype(np.uint16)
    return cent, cbs, labels


@functools.lru_cache(maxsize=None)
def placed_case(kind):
    """See the module's docstring.  Built once per kind and left unchanged by everyone."""
    d, m, ksub, bits = KINDS[kind]
    specs = [(name, tied, fn, L) for L in (LEN_LONG, LEN_SHORT) for name, tied, fn in placements(L)]
    kc = len(specs)
    rng = np.random.default_rng(8800 + sorted(KINDS).index(kind))
    cent, cbs, labels = _quantizers(kind, kc, rng)
    code_t = np.uint8 if bits == 8 else np.uint16
    cls = ora.OracleIndex if bits == 8 else u16_ref.U16Index
    empty = cls(cent, cbs, labels, np.zeros(kc + 1, np.int64), np.zeros((0, m), code_t), np.zeros(0, np.uint32))
    # queries: per list the designer query three times, three jittered copies (1e-4 of the residual norm), two unrelated ones
    qs = np.zeros((kc * QPL, d), f32)
    near = np.argsort(((cent[:, None, :].astype(np.float64) - cent[None, :, :]) ** 2).sum(-1), axis=1)
    for l in range(kc):
        res = (f32(0.05) * rng.standard_normal(d)).astype(f32)
        q = (cent[l] + res).astype(f32)
        qs[l * QPL:l * QPL + 3] = q
        for i in range(3, 6):
            u = rng.standard_normal(d)
            qs[l * QPL + i] = (q + (1e-4 * np.linalg.norm(res) / np.linalg.norm(u)) * u).astype(f32)
        found = 0
        for other in near[l, 1:]:
            for a in (0.45, 0.4, 0.35, 0.3):
                if found == 2:
                    break
                cand = (f32(a) * cent[l] + f32(1 - a) * cent[other] + f32(0.02) * rng.standard_normal(d).astype(f32)).astype(f32)
                pr = le.probes_of(cent, cand[None])[0][0]
                if pr[0] != l and l in pr[1:]:
                    qs[l * QPL + 6 + found] = cand
                    found += 1
        assert found == 2, "list %d has no unrelated query that reaches it as a later probe" % l
    probes, dcs = le.probes_of(cent, qs)
    own = np.repeat(np.arange(kc), QPL).reshape(kc, QPL)
    assert (probes[:, 0].reshape(kc, QPL)[:, :6] == own[:, :6]).all(), "every list must be the first probe of its own designer queries"
    assert all(l != probes[l * QPL + i, 0] and l in probes[l * QPL + i, 1:] for l in range(kc) for i in (6, 7))
    # lists: a pool of L random rows, sorted by (the designer query's sum, pool index), rank r stored at position pi[r]
    codes, lists = [], []
    for l, (name, tied, fn, L) in enumerate(specs):
        pool = np.stack([labels[i][rng.integers(0, ksub, L)] for i in range(m)], 1).astype(code_t)
        sums = le.row_sums(empty, qs[l * QPL], l, dcs[l * QPL, 0], pool)
        by_rank = pool[np.lexsort((np.arange(L), sums))]
        if tied:
            by_rank[:NTIED] = by_rank[0]
        pi = np.asarray(fn(rng), np.int64)
        assert np.array_equal(np.sort(pi), np.arange(L)), name
        rows = np.zeros_like(by_rank)
        rows[pi] = by_rank
        codes.append(rows)
        lists.append((name, L, pi))
    offsets = np.zeros(kc + 1, np.int64)
    np.cumsum([L for _, L, _ in lists], out=offsets[1:])
    n = int(offsets[-1])
    assert n < 1_000_000
    ids = rng.permutation(n).astype(np.uint32)
    ref = cls(cent, cbs, labels, offsets, np.ascontiguousarray(np.concatenate(codes)), ids)
    return Placed(kind, ref, qs, lists)


def probe_sums(case, r, ref=None):
    """[(list, f32 sums in position order)] of query r's W probes in visit order, in the reference's order of operations; ref: an index
    with the case's quantizers over other lists (a filtered copy)"""
    ref = case.ref if ref is None else ref
    probes, dcs = le.probes_of(ref.centroids, case.qs[r:r + 1])
    out = []
    for j, cl in enumerate(probes[0]):
        cl = int(cl)
        rows = ref.codes[ref.offsets[cl]:ref.offsets[cl + 1]]
        out.append((cl, le.row_sums(ref, case.qs[r], cl, dcs[0, j], rows)))
    return out


class Sorted:
    """The KMAX smallest (sum, visit order) keys of every query of a case over `ref`'s lists, by one stable sort per query.  The K best
    for any K <= KMAX are the first K of them (a sort's prefix); test_placement_model.py holds this against helpers.numpy_knn_batch /
    u16_ref.knn and the C oracle."""

    def __init__(self, case, ref=None):
        ref = case.ref if ref is None else ref
        nq = case.qs.shape[0]
        self.ids, self.dists = np.zeros((nq, KMAX), np.uint32), np.full((nq, KMAX), np.inf, f32)
        self.counts = np.zeros(nq, np.int64)
        for r in range(nq):
            ps = probe_sums(case, r, ref)
            dd = np.concatenate([s for _, s in ps])
            ii = np.concatenate([ref.ids[ref.offsets[cl]:ref.offsets[cl + 1]] for cl, _ in ps])
            top = np.argsort(dd, kind="stable")[:KMAX]
            self.counts[r] = len(top)
            self.ids[r, :len(top)], self.dists[r, :len(top)] = ii[top], dd[top]

    def top(self, K, queries=None):
        """(ids, dists, counts) as the search entries return them"""
        assert K <= KMAX
        sl = slice(None) if queries is None else queries
        return (np.ascontiguousarray(self.ids[sl, :K]), np.ascontiguousarray(self.dists[sl, :K]),
                np.minimum(self.counts[sl], K).astype(np.int32))


def reference(case, K, queries=None):
    """(ids, dists, counts) of the reference at K <= KMAX"""
    if case._sorted is None:
        case._sorted = Sorted(case)
    return case._sorted.top(K, queries)


def winners_mask(case, nranks=256):
    """boolean by id: the rows of rank < nranks of every list (the winners and their near misses)"""
    ref = case.ref
    mask = np.zeros(int(ref.ids.max()) + 1, bool)
    for l, (_, L, pi) in enumerate(case.lists):
        mask[ref.ids[ref.offsets[l] + pi[:nranks]]] = True
    return mask


def every_second_id(case):
    ids = case.ref.ids
    return np.arange(int(ids.max()) + 1) % 2 == 0


# ---- the model -------------------------------------------------------------------------------------------------------------------
KEY_MAX = (1 << 64) - 1
MUTANTS = {
    "a": "the floor(K/P)-th key where the ceil(K/P)-th is needed",
    "b": "the smallest, not the largest, of the parts' rank keys",
    "c": "parts that have not yet seen ceil(K/P) keys are ignored instead of holding the bound at KEY_MAX",
    "d": "the shared bound is kept through the merge: an entry equal to it is refused",
    "e": "held entries re-tested inclusively against the bound's sum: a part's own key, and every tie with it, is cut",
    "f": "a candidate that passed the block's stale mask replaces the selector's worst entry without being re-tested",
}


def keys_of(sums, base):
    """(sum bits << 32) | visit order, as Python-int-valued uint64: sums are positive floats, whose bit patterns order as they do"""
    s = np.ascontiguousarray(sums, f32)
    assert (s >= 0).all()
    return (s.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (base + np.arange(len(s))).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def _positions(L, granule, parts):
    gran = np.arange(L) // granule
    part_of = gran if parts is None else gran % parts
    P = int(part_of.max()) + 1 if parts is None else parts
    return [np.nonzero(part_of == j)[0] for j in range(P)]


# what the plan of this suite also lists as mutants, and what they are instead: both differ from the right form only at an exact tie of
# sums ACROSS probes -- a later probe's key of the same sum loses by its visit order either way --, so no result can tell them
EQUIVALENT = {
    "g": "the bound of probe j applied to probe j + 1's keys before their visit-order base is added",
    "h": "probe pruning with >= for > against the next probe's coarse distance",
}


def model(probes, K, granule, parts, mutant=None, block=64, dcs=None, info=None):
    """probes: the f32 sums of a query's probed lists in position order, in visit order.  Returns (visit orders, sums) of the K best.

    A position p of a list belongs to part (p // granule) % parts (parts None: p // granule, one part per chunk).  Every part has a
    selector of K entries and reads its positions in blocks of `block`; the parts take turns, block by block, and after every block the
    shared bound is refreshed: B = min(B, the largest of the P parts' ceil(K/P)-th smallest held keys), KEY_MAX while any part holds
    fewer.  (P ceil(K/P) >= K held keys lie at or below it: it never falls below the K-th best key.)  A block's candidates are masked
    once against B as it stood when the block began (key <= B), then inserted one by one, each re-tested against the selector's worst
    entry once the selector is full.  Held entries above a refreshed bound are dropped.  The bound carries over from probe to probe;
    the merge takes the K smallest of everything held.  dcs: the probes' coarse distances; given them, a probe whose coarse distance
    exceeds the bound's sum is skipped (every sum of a list is at least its coarse distance); info["skipped"] counts those."""
    assert mutant is None or mutant in MUTANTS or mutant in EQUIVALENT
    B = KEY_MAX
    held = {}                 # part -> sorted list of keys
    base = 0
    for j_probe, sums in enumerate(probes):
        keys = keys_of(sums, base)
        L = len(keys)
        mine = base
        base += L
        if L == 0:
            continue
        if dcs is not None and B != KEY_MAX:
            dc_bits, b_bits = int(np.asarray(dcs[j_probe], f32).view(np.uint32)), B >> 32
            if dc_bits >= b_bits if mutant == "h" else dc_bits > b_bits:
                if info is not None:
                    info["skipped"] = info.get("skipped", 0) + 1
                continue
        pos = _positions(L, granule, parts)
        P = len(pos)
        rk = max(1, K // P) if mutant == "a" else -(-K // P)
        for j in range(P):
            held.setdefault(j, [])
        for t in range(max(-(-len(p) // block) for p in pos)):
            for j in range(P):
                blk = keys[pos[j][t * block:(t + 1) * block]]
                if len(blk) == 0:
                    continue
                S = held[j]
                took = False
                seen_as = blk - np.uint64(mine) if mutant == "g" else blk
                for c in blk[seen_as <= np.uint64(B)].tolist():   # the mask is the block's: B as it stood when the block began
                    if len(S) < K:
                        bisect.insort(S, c)
                        took = True
                    elif mutant == "f" or c < S[-1]:
                        S.pop()
                        bisect.insort(S, c)
                        took = True
                if not took:                                      # nothing held has changed: neither has the bound
                    continue
                # refresh
                rank_keys = [held[i][rk - 1] if len(held[i]) >= rk else None for i in range(P)]
                if mutant == "c":
                    rank_keys = [x for x in rank_keys if x is not None]
                if rank_keys and all(x is not None for x in rank_keys):
                    B = min(B, min(rank_keys) if mutant == "b" else max(rank_keys))
                if B != KEY_MAX:
                    for i in held:
                        if mutant == "e":
                            held[i] = [x for x in held[i] if (x >> 32) < (B >> 32)]
                        elif held[i] and held[i][-1] > B:
                            held[i] = held[i][:bisect.bisect_right(held[i], B)]
    merged = sorted(x for S in held.values() for x in S if not (mutant == "d" and x >= B))[:K]
    out = np.array(merged, np.uint64)
    return (out & np.uint64(0xFFFFFFFF)).astype(np.int64), (out >> np.uint64(32)).astype(np.uint32).view(f32)


def exhaustive(probes, K):
    """the K smallest (sum, visit order) keys of the probes, by a sort: what model() must return when it is not mutated"""
    keys = np.sort(np.concatenate([keys_of(s, b) for s, b in zip(probes, np.cumsum([0] + [len(s) for s in probes[:-1]]))]))[:K]
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), (keys >> np.uint64(32)).astype(np.uint32).view(f32)


# ---- the probe placement ---------------------------------------------------------------------------------------------------------
PROBE_WS = (1, 2, 3, 16, 17, 24, 25, 32, 33, 48, 49, 63, 64, 65)
PROBE_KS = (1, 10, 17, 64)
PROBE_MODES = ("first", "last", "each")      # the probe rank(s) whose list holds the winners: 0, w - 1, every one
PROBE_KC, PROBE_D, PROBE_M = 256, 32, 8
PROBE_ORDINARY = 40                          # ordinary points per list
PROBE_WINNERS = 12                           # all-zero codes in the holding list (`each`: one per list): K = 1 / 10 are winners only --
#                                              the K-th best key lies BELOW the next probe's coarse distance --, K = 17 / 64 reach into
#                                              the ordinary points, whose sums lie ABOVE every coarse distance
PROBE_NQ = 16                                # the designer query four times, four jittered copies, eight unrelated queries


class ProbeCase:
    def __init__(self, mode, w, ref, qs, holding):
        self.mode, self.w, self.ref, self.qs, self.holding = mode, w, ref, qs, holding


@functools.lru_cache(maxsize=None)
def _probe_base():
    """quantizers and queries shared by every probe case: codebooks as in list_end.hostile_case -- one zero codeword per sub-space, every
    other codeword 4 .. 5 times the longest residual slice long -- so that a point with the all-zero code beats every ordinary point of
    every probed list"""
    kc, d, m = PROBE_KC, PROBE_D, PROBE_M
    dsub = d // m
    rng = np.random.default_rng(8900)
    cent = rng.random((kc, d), dtype=f32)
    res = (f32(0.02) * rng.standard_normal(d)).astype(f32)
    q = (cent[17] + res).astype(f32)
    qs = np.zeros((PROBE_NQ, d), f32)
    qs[:4] = q
    for i in range(4, 8):
        u = rng.standard_normal(d)
        qs[i] = (q + (1e-4 * np.linalg.norm(res) / np.linalg.norm(u)) * u).astype(f32)
    qs[8:] = rng.random((8, d), dtype=f32)
    wmax = max(PROBE_WS)
    probes, dcs = le.probes_of(cent, qs, wmax)
    assert all(np.array_equal(probes[i], probes[0]) for i in range(8)), "the jitter must not move the designer query's probe order"
    r = (qs[:, None, :] - cent[probes]).reshape(PROBE_NQ, wmax, m, dsub).astype(np.float64)
    rmax = float(np.sqrt((r ** 2).sum(-1)).max())
    labels = np.stack([rng.permutation(256) for _ in range(m)]).astype(np.uint8)
    zero = np.array([int(np.nonzero(labels[i] == 0)[0][0]) for i in range(m)])
    dirs = rng.standard_normal((m, 256, dsub))
    dirs /= np.sqrt((dirs ** 2).sum(-1, keepdims=True))
    cbs = (dirs * (rmax * rng.uniform(4.01, 4.99, (m, 256, 1)))).astype(f32)
    cbs[np.arange(m), zero] = 0
    return cent, cbs, labels, zero, qs, probes[0], dcs[0]


@functools.lru_cache(maxsize=None)
def probe_case(mode, w):
    """An index whose all-zero-code points sit only in the designer query's probe of rank 0 (`first`), of rank w - 1 (`last`: the list
    probe pruning would drop first), or one in every probe (`each`).  `first` and `each` are one index for every w."""
    assert mode in PROBE_MODES and w in PROBE_WS
    if mode != "last" and w != PROBE_WS[0]:
        c = probe_case(mode, PROBE_WS[0])
        return ProbeCase(mode, w, c.ref, c.qs, c.holding)
    cent, cbs, labels, zero, qs, order, _ = _probe_base()
    kc, m = PROBE_KC, PROBE_M
    rng = np.random.default_rng(8901 + 100 * PROBE_MODES.index(mode) + w)
    holding = {"first": order[:1], "last": order[w - 1:w], "each": order}[mode]
    nwin = np.zeros(kc, np.int64)
    nwin[holding] = 1 if mode == "each" else PROBE_WINNERS
    sizes = PROBE_ORDINARY + nwin
    offsets = np.zeros(kc + 1, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    n = int(offsets[-1])
    pick = rng.integers(0, 255, (n, m))
    pick += pick >= zero[None, :]
    codes = np.stack([labels[i][pick[:, i]] for i in range(m)], 1).astype(np.uint8)
    for l in np.nonzero(nwin)[0]:
        at = offsets[l] + rng.choice(sizes[l], nwin[l], replace=False)
        codes[at] = 0
    ids = rng.permutation(n).astype(np.uint32)
    ref = ora.OracleIndex(cent, cbs, labels, offsets, np.ascontiguousarray(codes), ids)
    return ProbeCase(mode, w, ref, qs, np.sort(holding))
