"""The coarse stage's case table and a CPU model of its certificates (tests/test_coarse_edges_model.py, tests/test_gpu_coarse_edges.py).

The coarse search has three "certified exact" readers -- refine_probes over a pool of approx_pool(w) matrix-core scores, select_listed
over per-tile records of four keys, and the two-level visit of twolevel.hip.h -- and each is exact by an argument with an edge of its
own: the pool's last member against T, a record's fourth key against T, LISTED_MAX tiles, a group's bound against the w-th distance.
With uniform-random centroids the w-th cell lies nowhere near any of them.  Here every quantizer is a few hostile cells placed among
filler cells so that the premise of each edge is exact and can be asserted on the CPU:

  * coordinates live on a power-of-two lattice, so every distance the table reasons about is exact in Float32 in the reference's order;
  * a cluster "one ulp apart" is (a, b_j, 0, ...) around its query with a^2 = rho and b_j^2 = j ulp(rho): the reference's sum is
    rho + j ulp exactly, while the Float64 distance kept beside it tells the members apart even where the Float32 sums tie.

The reference is the oracle's coarse_search: the Float32 sequential sum without FMA, sorted by (distance bits, cell).

The model restates the three readers over scores A_c = D_c + e_c that an adversary chooses with |e_c| <= eps_form(q) (ADVERSARIES), and
MUTANTS lists the ways this class of certificate goes wrong; a mutant that no row catches is a hole in the table."""
import numpy as np

f32 = np.float32
TILE = 64                 # centroids per record / per tile minimum (128-wide kernels: two 64-cell tiles per workgroup column)
LISTED_MAX = 128
RHO = 4.0                 # squared distance of a hostile cluster from its query (a = 2); every other cell lies at >= 4 RHO
ULP_RHO = 2.0 ** -21
FORMS = ("f32", "bf16", "f16")
POOL_WS = (1, 8, 16, 24, 32, 48)
D = 32


def approx_pool(w):
    return min(64, w + max(16, w))


def eps_coef(form, d, listed=False):
    """refine_args: the score's error over (||c|| + ||q||)^2"""
    u = f32(5.9604645e-8)
    if form == "f16":
        c = f32(2.0) * (f32(8194.0) + f32(2.0) + f32(0.51) * f32(d + 40) + f32(d + 8)) * u
    elif form == "bf16":
        c = f32(2.0) * (f32(97.0) + f32(0.51) * f32(3 * d + 40) + f32(d + 8)) * u
    else:
        c = f32(2.0) * f32(d + 3) * u
    if listed:
        c = c + f32(128.0) * u
    return float(c)


def gam(d):
    return float(f32(4.0) * f32(d + 2) * f32(5.9604645e-8))


def tl_eps(d):
    return float(f32(d + 16) * f32(1.1920929e-7))


_CMAXN = {}


def cmaxn_of(cent):
    """centroid_norms: >= the largest centroid norm (memoised per array, which the memo keeps alive)"""
    key = (cent.ctypes.data, cent.shape)
    if key not in _CMAXN or _CMAXN[key][0] is not cent:
        _CMAXN[key] = (cent, float(f32(np.sqrt((cent.astype(np.float64) ** 2).sum(1).max()) * (1.0 + 1e-6))))
    return _CMAXN[key][1]


def f16_scale(cent):
    return float(2.0 ** np.floor(np.log2(4096.0 / float(np.abs(cent).max()))))


def flagged(cent, q):
    """split_f16_kernel: a scaled component outside the f16 range flags the query"""
    return bool((np.abs(q.astype(f32) * f32(f16_scale(cent))) > f32(65000.0)).any())


def eps_of(form, cent, q, listed=False):
    qn = float((q.astype(np.float64) ** 2).sum())
    sumn = cmaxn_of(cent) + np.sqrt(qn) * 1.00001
    return eps_coef(form, cent.shape[1], listed) * sumn * sumn


def threshold(tau, eps, g, mutant=None):
    """T of refine_probes / select_listed.  The relative inflation is gam and the 1e-6 safety factor together: mutant `no_gam` drops both."""
    if mutant == "no_eps":
        return tau * (1.0 + g) * (1.0 + 1e-6)
    if mutant == "no_gam":
        return tau + 2.0 * eps
    t = (tau + eps) * (1.0 + g) + eps
    return t + abs(t) * 1e-6


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def oracle_dists(cent, qs):
    """(nq, kc) Float32 distances in the reference's order: ascending dimension, sub / mul / add, one rounding each"""
    qs = np.atleast_2d(qs).astype(f32)
    acc = np.zeros((qs.shape[0], cent.shape[0]), f32)
    for i in range(cent.shape[1]):
        t = cent[None, :, i] - qs[:, i, None]
        acc = acc + t * t
    return acc


def exact_dists(cent, q):
    return ((cent.astype(np.float64) - q.astype(np.float64)[None, :]) ** 2).sum(1)


def top_of(dist, w, cells=None):
    """the w smallest (distance bits, cell) of one row: cells, distances"""
    cells = np.arange(dist.shape[0]) if cells is None else np.asarray(cells)
    o = np.lexsort((cells, dist))[:w]
    return cells[o].astype(np.int32), dist[o].astype(f32)


def oracle_rows(cent, qs, w):
    """(lists, dists) of a batch, in chunks"""
    qs = np.atleast_2d(qs)
    lists, dists = np.zeros((qs.shape[0], w), np.int32), np.zeros((qs.shape[0], w), f32)
    for r0 in range(0, qs.shape[0], 512):
        acc = oracle_dists(cent, qs[r0:r0 + 512])
        key = (acc.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(cent.shape[0], dtype=np.uint64)[None, :]
        part = np.sort(np.partition(key, w - 1, axis=1)[:, :w], axis=1) if w < cent.shape[0] else np.sort(key, axis=1)
        lists[r0:r0 + 512] = (part & np.uint64(0xFFFFFFFF)).astype(np.int32)
        dists[r0:r0 + 512] = (part >> np.uint64(32)).astype(np.uint32).view(f32)
    return lists, dists


# ---- tables -----------------------------------------------------------------------------------------------------------------------------
class Row:
    def __init__(self, name, q, ws, **meta):
        self.name, self.q, self.ws, self.meta = name, np.ascontiguousarray(q, f32), tuple(ws), meta

    def __repr__(self):
        return self.name


class Table:
    """cent (kc, d); rows; groups: the clumps of a two-level table (lists of cells), None elsewhere"""

    def __init__(self, name, cent, rows, groups=None):
        self.name, self.cent, self.rows, self.groups = name, np.ascontiguousarray(cent, f32), rows, groups
        self.kc, self.d = self.cent.shape

    def row(self, name):
        return next(r for r in self.rows if r.name == name)


def _signs(rng, n, d=D):
    return (rng.integers(0, 2, (n, d)) * 2 - 1).astype(f32)


def cluster(centre, t, equal=False):
    """t cells at squared distance RHO + j ulp from `centre` (whose coordinates 0 and 1 are 0), j = t - 1 down to 0: the order by cell is
    the reverse of the order by distance.  equal: all at RHO exactly."""
    out = np.tile(centre.astype(f32), (t, 1))
    out[:, 0] += f32(2.0)
    if not equal:
        j = np.arange(t - 1, -1, -1)
        out[:, 1] += (np.sqrt(2.0 * j).astype(f32) * f32(2.0 ** -11)).astype(f32)
    return out


class _Builder:
    """A quantizer of kc cells: hostile blocks at chosen or random cell numbers, lattice filler {-2, 2}^d everywhere else"""

    def __init__(self, seed, kc, d=D):
        self.rng = np.random.default_rng(seed)
        self.kc, self.d = kc, d
        self.cent = f32(2.0) * _signs(self.rng, kc, d)
        self.free = np.ones(kc, bool)
        self.rows = []

    def site(self):
        """a query location: lattice {-2, 2} with coordinates 0 and 1 at 0"""
        s = f32(2.0) * _signs(self.rng, 1, self.d)[0]
        s[:2] = 0
        return s

    def put(self, cells, at=None):
        """cells (n, d) at the consecutive cell numbers at ..., or at a random free run; returns the first cell number"""
        n = cells.shape[0]
        if at is None:
            for _ in range(10000):
                at = int(self.rng.integers(0, self.kc - n + 1))
                if self.free[at:at + n].all():
                    break
            else:
                raise AssertionError("no room for %d cells" % n)
        assert self.free[at:at + n].all(), (at, n)
        self.cent[at:at + n] = cells
        self.free[at:at + n] = False
        return at

    def put_at(self, cells, numbers):
        for c, n in zip(cells, numbers):
            self.put(c[None, :], int(n))


def pool_table(kc=2088, ws=POOL_WS, seed=7001, d=D):
    """Pool edge, norms and signs"""
    b = _Builder(seed, kc, d)
    # pool edge: t cells around the query on either side of P = approx_pool(w); a sibling with all distances equal at t = P - 1 and P
    for w in ws:
        P = approx_pool(w)
        for t in (P - 2, P - 1, P, P + 1):
            for equal in ((False, True) if t in (P - 1, P) else (False,)):
                s = b.site()
                at = b.put(cluster(s, t, equal))
                b.rows.append(Row("pool w=%d t=%s%d%s" % (w, "P" if t == P else "P%+d" % (t - P), t, " equal" if equal else ""), s, (w,),
                                  family="pool", t=t, P=P, cells=(at, at + t), equal=equal))
    # norms and signs
    tw = b.put(np.tile(f32(2.0) * _signs(b.rng, 1, d), (2, 1)))                    # twins side by side ...
    far_twin = b.put(b.cent[tw][None, :].copy())                                     # ... and a third one elsewhere
    b.rows.append(Row("on a cell: twins", b.cent[tw], (1, 2, 8), family="norms", twins=(tw, tw + 1, far_twin)))
    lone = int(np.nonzero(b.free)[0][3])
    b.rows.append(Row("on a cell: filler", b.cent[lone], (1, 8, 48), family="norms", cell=lone))
    v = _signs(b.rng, 3, d)
    b.rows.append(Row("far outside, 8 ||c||", f32(15.5) * v[0], (1, 8, 32), family="norms"))
    b.rows.append(Row("far outside, flagged", f32(64.0) * v[1], (1, 8, 32), family="norms", flagged=True))
    u = (b.rng.random((2, d)) * 4 - 2).astype(f32)
    inside, outside = u[0].copy(), u[0].copy()
    inside[5], outside[5] = f32(31.5), f32(32.0)
    b.rows.append(Row("f16: component 31.5, inside the range", inside, (1, 8, 32), family="norms", flagged=False))
    b.rows.append(Row("f16: component 32, flagged", outside, (1, 8, 32), family="norms", flagged=True))
    b.cent[int(np.nonzero(b.free)[0][0])] = f32(2.0)                                  # max |component| = 2 exactly: f16 scale 2048
    return Table("pool kc=%d d=%d" % (kc, d), b.cent, b.rows)


GAP_W = 8


def gap_table(kc=2088, seed=7008, d=D):
    """Gap sweep, w = 8: w - 1 cells at squared distance 1 + j ulp, the w-th at RHO in the site's HIGHEST cell, and in its lowest cells the
    (w + 1)-th to (P + 1)-th, all eps_form 2^k beyond the w-th, k = -6 ... 3 for each form's eps: the pool's last member stands the gap
    away from tau, on either side of T - tau ~ 2 eps.  Where exactly a form's certificate turns depends on the kernel's real error.
    Rounding tie: the w-th and (w + 1)-th cells have the SAME Float32 distance and different real ones; the lower cell -- which wins the
    tie -- is the farther one, so its score may exceed the other's by 2 eps and more: only the relative inflation of T keeps it."""
    b = _Builder(seed, kc, d)
    w, P = GAP_W, approx_pool(GAP_W)
    near = (np.sqrt(2.0 * np.arange(w - 1, 0, -1)).astype(f32) * f32(2.0 ** -12)).astype(f32)
    for form in FORMS:
        for k in range(-6, 4):
            s = b.site()
            n = P - w + 1
            cells = np.tile(s, (n + w, 1))
            cells[:n, 0] += f32(2.0)                       # (their second coordinate needs eps, which needs the finished quantizer: below)
            cells[n:n + w - 1, 0] += f32(1.0)
            cells[n:n + w - 1, 1] += near
            cells[n + w - 1, 0] += f32(2.0)
            at = b.put(cells)
            b.rows.append(Row("gap %s k=%d" % (form, k), s, (w,), family="gap", form=form, k=k, cells=(at, at + n + w), beyond=n))
    s = b.site()
    cells = np.tile(s, (w + 1, 1))
    cells[:, 0] += f32(2.0)
    cells[1:w, 0] -= f32(1.0)
    cells[1:w, 1] += near
    b5 = f32(np.sqrt(10.0)) * f32(2.0 ** -11)
    cells[0, 1] += f32(b5 * f32(1.0 + 2.0 ** -10))
    cells[w, 1] += b5
    at = b.put(cells)
    b.rows.append(Row("rounding tie", s, (w,), family="gap", cells=(at, at + w + 1), beyond=1))
    # the same tie at w = 1 with the two cells in different 64-cell tiles: each is its record's first key, so the records' reader takes
    # tau from the nearer one's score and must still reach the farther, lower cell
    s = b.site()
    pair = np.tile(s, (2, 1))
    pair[:, 0] += f32(2.0)
    pair[0, 1] += f32(b5 * f32(1.0 + 2.0 ** -10))
    pair[1, 1] += b5
    free_tiles = [t for t in range(kc // TILE) if b.free[TILE * t:TILE * (t + 1)].any()]
    tlo, thi = free_tiles[1], free_tiles[-2]
    numbers = [TILE * t + int(np.nonzero(b.free[TILE * t:TILE * (t + 1)])[0][0]) for t in (tlo, thi)]
    b.put_at(pair, numbers)
    b.rows.append(Row("rounding tie across two tiles", s, (1,), family="gap", pair=tuple(numbers)))
    b.cent[int(np.nonzero(b.free)[0][0])] = f32(2.0)
    tab = Table("gap kc=%d" % kc, b.cent, b.rows)
    for r in tab.rows:
        if "k" in r.meta:
            gap = eps_of(r.meta["form"], tab.cent, r.q) * 2.0 ** r.meta["k"]
            lo = r.meta["cells"][0]
            tab.cent[lo:lo + r.meta["beyond"], 1] += f32(np.sqrt(gap))
    return tab


def records_table(kc=2088, seed=7002, d=D):
    """select_listed's records: near-ties inside one 64-cell tile, winners sharing two tiles, the ragged last tile"""
    assert kc % 64 and kc % 128
    b = _Builder(seed, kc, d)
    tiles = list(b.rng.permutation(kc // TILE - 1)[:20])
    for n in (3, 4, 5, 64):
        s = b.site()
        t = int(tiles.pop())
        at = b.put(cluster(s, n), TILE * t + (0 if n == 64 else int(b.rng.integers(0, TILE - n + 1))))
        b.rows.append(Row("record: %d near-ties in tile %d" % (n, t), s, (1, 2, 8), family="records", cells=(at, at + n), n=n))
    for na, nb in ((4, 4), (5, 3), (7, 1)):
        s = b.site()
        ta, tb = int(tiles.pop()), int(tiles.pop())
        cl = cluster(s, na + nb)
        lo, hi = min(ta, tb), max(ta, tb)
        a0 = b.put(cl[:nb], TILE * lo + int(b.rng.integers(0, TILE - 8)))             # the farther ones in the lower tile
        a1 = b.put(cl[nb:], TILE * hi + int(b.rng.integers(0, TILE - 8)))
        b.rows.append(Row("records: 8 winners as %d + %d in tiles %d and %d" % (nb, na, lo, hi), s, (8,), family="records", cells=(a0, a1)))
    # one per tile with a gap in front of the w-th: seven winners at squared distance 1, the eighth at RHO, each alone in its tile -- the
    # tile AT the bound holds a winner, and the seven keys below it say nothing about where the eighth lies
    s = b.site()
    cl = np.tile(s, (8, 1))
    cl[:, 0] += f32(1.0)
    cl[:, 1] += (np.sqrt(2.0 * np.arange(8)).astype(f32) * f32(2.0 ** -12)).astype(f32)
    cl[7, :2] = (2.0, 0.0)
    numbers = [TILE * int(tiles.pop()) + int(b.rng.integers(0, TILE)) for _ in range(8)]
    b.put_at(cl, numbers)
    b.rows.append(Row("records: one winner per tile, the 8th beyond a gap", s, (8,), family="records", numbers=numbers))
    # the ragged last tile: a query at the origin (a phantom cell of that tile, an all-zero row, would lie at distance ||q||^2 = 0) whose
    # winners are the tile's last real cells
    s = np.zeros(d, f32)
    at = b.put(cluster(s, 3), kc - 3)
    b.rows.append(Row("ragged tile: winner at the last real cell, query at the origin", s, (1, 2, 8), family="records", cells=(at, kc), origin=True))
    s = b.site()
    at = b.put(cluster(s, 1), kc - 4)
    b.rows.append(Row("ragged tile: lone winner", s, (1, 8), family="records", cells=(at, at + 1)))
    for i, u in enumerate((b.rng.random((4, d)) * 4 - 2).astype(f32)):              # what a filler query looks like
        b.rows.append(Row("records: uniform query %d" % i, u, (1, 8), family="filler"))
    b.cent[int(np.nonzero(b.free)[0][0])] = f32(2.0)
    return Table("records kc=%d" % kc, b.cent, b.rows)


def tiles_table(kc=8320, seed=7003, d=D):
    """Near-ties one per tile across 127, 128 and 129 tiles: either side of LISTED_MAX"""
    assert kc // TILE >= 130
    b = _Builder(seed, kc, d)
    for n in (127, 128, 129):
        s = b.site()
        tl = np.sort(b.rng.permutation(kc // TILE)[:n])
        cl = cluster(s, n)                                                           # the nearest in the highest tile
        numbers = []
        for t in tl:
            free = np.nonzero(b.free[TILE * t:TILE * (t + 1)])[0]
            numbers.append(TILE * int(t) + int(free[b.rng.integers(0, free.size)]))
            b.free[numbers[-1]] = False
        b.cent[numbers] = cl
        b.rows.append(Row("tiles: one near-tie in each of %d tiles" % n, s, (1, 8), family="tiles", n=n, numbers=np.array(numbers)))
    b.cent[int(np.nonzero(b.free)[0][0])] = f32(2.0)
    return Table("tiles kc=%d" % kc, b.cent, b.rows)


def norm_table(kc=2088, seed=7004, d=D):
    """One cell with 2^10 times the others' norm: cmaxn, and with it eps, is set by a cell far from every query"""
    b = _Builder(seed, kc, d)
    big = int(b.rng.integers(0, kc))
    b.cent[big] *= f32(1024.0)
    for i, c in enumerate(np.nonzero(np.arange(kc) != big)[0][[5, 700, kc - 3]]):
        b.rows.append(Row("big norm: on cell %d" % c, b.cent[c], (1, 8, 48), family="norms", cell=int(c)))
    u = (b.rng.random(d) * 4 - 2).astype(f32)
    b.rows.append(Row("big norm: uniform query", u, (1, 8, 48), family="norms"))
    return Table("big norm kc=%d" % kc, b.cent, b.rows)


CLUMPS = (1, 2, 63, 64, 65, 128, 129) + (32,) * 9


def clump_table(seed=7005, d=D):
    """Two-level: 16 well-separated clumps (centres 4 v, v in {-1, 1}^d) of the sizes around the kernel's 64-lane round.  Every clump of
    two or more ends -- at its HIGHEST cell number, the slot whose lanes past the group's end repeat -- with a champion at 3.5 v: from the
    origin all champions tie at 392 exactly, and a query near the origin has its w winners in w different clumps.  Clumps are numbered
    so that the one with the largest bound from the origin holds the lowest cells."""
    rng = np.random.default_rng(seed)
    v = _signs(rng, len(CLUMPS), d)
    assert len({tuple(x) for x in v}) == len(CLUMPS)
    blocks = []
    for k, n in enumerate(CLUMPS):
        offs = set()
        while len(offs) < max(n - 1, 1):
            o = np.zeros(d, f32)
            o[rng.permutation(d)[:4]] = rng.choice(np.array([-0.5, -0.25, 0.25, 0.5], f32), 4)
            offs.add(tuple(o))
        mem = f32(4.0) * v[k][None, :] + np.array(sorted(offs), f32)
        if n == 1:
            mem = f32(4.0) * v[k][None, :]
        else:
            mem = np.concatenate([mem[:n - 1], f32(3.5) * v[k][None, :]])
        blocks.append(mem)
    # order the clumps by descending bound from the origin
    zero = np.zeros(d, f32)
    bounds = [group_bound(blk, zero, tl_eps(d)) for blk in blocks]
    order = sorted(range(len(CLUMPS)), key=lambda k: -bounds[k])
    cent = np.concatenate([blocks[k] for k in order])
    sizes = [CLUMPS[k] for k in order]
    start = np.concatenate([[0], np.cumsum(sizes)])
    groups = [np.arange(start[i], start[i + 1]) for i in range(len(sizes))]
    by_size = {n: groups[i] for i, n in enumerate(sizes)}
    rows = []
    ws = (1, 8, 64, 65)
    g128 = by_size[128]
    inside = cent[g128[:-1]].astype(np.float64).mean(0).astype(f32)
    inside = (np.round(inside * 64) / 64).astype(f32)
    inside[0] += f32(0.125)
    rows.append(Row("two-level: inside the clump of 128", inside, ws, family="twolevel", group=128))
    delta = (rng.integers(-8, 9, d) / 64.0).astype(f32)
    rows.append(Row("two-level: winners spread over w clumps", delta, ws, family="twolevel"))
    rows.append(Row("two-level: champions tie across clumps", zero, ws, family="twolevel"))
    for n in (1, 2, 63, 64, 65, 129):
        g = by_size[n]
        q = cent[g[-1]].copy()
        q[3] += f32(0.125)
        rows.append(Row("two-level: next to the last member of the clump of %d" % n, q, ws, family="twolevel", group=n))
    return Table("clumps kc=%d" % cent.shape[0], cent, rows, groups)


def twins_table(d=D):
    """clump_table with the clump of 128 handed to the model as two groups, both of which contain a query that sits on a cell of the lower
    half; a cell of the upper half is made that cell's twin, and the upper half is visited first (same bound, 0; lower group number).  The
    lower cell wins the tie only if a bound EQUAL to the w-th distance does not end the visit.  (The library's own grouping may differ:
    on the GPU this is an exactness row like any other.)"""
    tab = clump_table(d=d)
    g128 = next(g for g in tab.groups if len(g) == 128)
    cent = tab.cent.copy()
    lo, hi = int(g128[10]), int(g128[70])
    cent[hi] = cent[lo]
    groups = [g128[64:]] + [g for g in tab.groups if g is not g128] + [g128[:64]]
    return Table("clumps + twins", cent, [Row("two-level: twins in two groups that both contain the query", cent[lo], (1, 2), family="twolevel",
                                              twins=(lo, hi))], groups)


def stray_table(seed=7006, d=D):
    """clump_table plus a lone cell at squared distance 2.25 from a member of the clump of 129, as a group of its own: without the
    `s > 0` clamp the big clump's bound (r - ||q - g||)^2 exceeds 2.25 and the member at distance +0 is never looked at"""
    tab = clump_table(d=d)
    g = max(tab.groups, key=len)
    q = tab.cent[g[7]].copy()
    stray = q.copy()
    stray[2] += f32(1.5)
    cent = np.concatenate([tab.cent, stray[None, :]])
    groups = [np.asarray(x) for x in tab.groups] + [np.array([cent.shape[0] - 1])]
    return Table("clumps + stray", cent, [Row("two-level: stray cell beside a member", q, (1, 2), family="twolevel")], groups)


def normal_table(kc=4160, seed=7007, d=D):
    """Unstructured N(0, 1) centroids: no bound closes, G > 64, the branch after 64 groups runs.  The model's grouping: 64 cells each,
    in cell order (65 groups); rows: queries on cells of the last group."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((kc, d)).astype(f32)
    groups = [np.arange(g0, min(g0 + 64, kc)) for g0 in range(0, kc, 64)]
    rows = [Row("normal: on cell %d" % c, cent[c], (1, 8, 64), family="twolevel") for c in (kc - 1, kc - 40, 17)]
    return Table("normal kc=%d" % kc, cent, rows, groups)


_TABLES = {}


def table(name):
    if name not in _TABLES:
        _TABLES[name] = {"pool": pool_table, "small": lambda: pool_table(384, (1, 8), 7011),
                         "small64": lambda: pool_table(384, (1, 8), 7012, 64), "gap": gap_table, "records": records_table, "tiles": tiles_table,
                         "norm": norm_table, "clumps": clump_table, "twins": twins_table, "stray": stray_table, "normal": normal_table}[name]()
    return _TABLES[name]


# ---- placement in the batch -------------------------------------------------------------------------------------------------------------
def filler_queries(nq, d, seed):
    return (np.random.default_rng(seed).random((nq, d)) * 4 - 2).astype(f32)


def safe_filler(tab, ws, n, seed, candidates=16384):
    """n uniform queries, drawn from `candidates`, whose certificate PASSES at every w of ws in every form whatever the kernel's rounding
    does: with the f16 form's eps (the largest), the P-th smallest real distance minus eps lies above T(w-th smallest + eps).  A uniform
    query whose nearest point is one of the table's clusters fails the certificate legitimately; beside the pool-edge rows, whose
    fallbacks are counted, the filler must not."""
    qs = filler_queries(candidates, tab.d, seed)
    ok = filler_passes(tab, qs, ws)
    assert ok.sum() >= n, (tab.name, int(ok.sum()), n)
    return qs[ok][:n]


def filler_of(tab, n=1024):
    """The n distinct filler queries the GPU file repeats through its batches of this table: uniform over the box of the centroids
    (two-level tables), uniform and provably passing where fallbacks are counted (tables with pool or gap rows), uniform elsewhere."""
    if tab.groups is not None:
        lo, hi = tab.cent.min(0), tab.cent.max(0)
        return (lo + np.random.default_rng(13).random((n, tab.d), dtype=f32) * (hi - lo)).astype(f32)
    counted = sorted({w for r in tab.rows if r.meta["family"] in ("pool", "gap") for w in r.ws})
    if counted:
        return safe_filler(tab, counted, n, 12)
    return filler_queries(n, tab.d, 12)


def filler_passes(tab, qs, ws):
    c64 = tab.cent.astype(np.float64)
    ok = np.ones(qs.shape[0], bool)
    for r0 in range(0, qs.shape[0], 1024):
        q = qs[r0:r0 + 1024].astype(np.float64)
        qn = (q ** 2).sum(1)
        dd = np.sort(qn[:, None] - 2.0 * q @ c64.T + (c64 ** 2).sum(1)[None, :], axis=1)
        sumn = cmaxn_of(tab.cent) + np.sqrt(qn) * 1.00001
        eps = eps_coef("f16", tab.d) * sumn * sumn
        for w in ws:
            P = min(approx_pool(w), tab.kc)
            T = (dd[:, w - 1] + 2.0 * eps) * (1.0 + gam(tab.d)) + eps
            ok[r0:r0 + 1024] &= dd[:, P - 1] - eps > T * (1.0 + 1e-6) + 1e-9
    return ok


def place(filler, hostile, turn=0):
    """The batch: `filler` with the hostile queries written over it in four blocks -- from row 0, up to row 127, from the first row of the
    last 128-row tile, up to the last row -- each block rotated by `turn`, so that the query ON the anchor row changes from call to call.
    Returns (batch, rows): rows[i] = the four positions of hostile query i."""
    nq, h = filler.shape[0], len(hostile)
    last = (nq - 1) // 128 * 128
    assert h >= 1 and (nq <= 128 or (2 * h <= 128 and 2 * h <= nq - last)), (nq, h)
    out = filler.copy()
    pos = [[] for _ in range(h)]
    starts = [0, 128 - h, last, nq - h] if nq > 128 else [0, nq - h]
    for bi, s0 in enumerate(starts):
        for j in range(h):
            i = (j + turn + bi) % h
            out[s0 + j] = hostile[i]
            pos[i].append(s0 + j)
    return out, pos


# ---- the model --------------------------------------------------------------------------------------------------------------------------
ADVERSARIES = ("zero", "worst", "opposite", "random")


def adversary(pattern, kc, winners, eps, seed=0):
    """e_c with |e_c| <= eps: none; + on the oracle's winners and - on everyone else; the opposite; seeded random signs"""
    if pattern == "zero":
        return np.zeros(kc)
    if pattern == "random":
        return eps * (np.random.default_rng(seed).integers(0, 2, kc) * 2.0 - 1.0)
    e = np.full(kc, -eps)
    e[winners] = eps
    return e if pattern == "worst" else -e


def _pick(cand, O, w, mutant):
    cand = np.asarray(cand, np.int64)
    o = np.lexsort((-cand if mutant == "ties_high" else cand, O[cand]))[:w]
    return cand[o].astype(np.int32), O[cand[o]].astype(f32)


def model_refine(A, O, w, eps, g, flag=False, mutant=None):
    """refine_probes over the scores A (A_c ~ D_c within eps): (cells, distances, fell_back)"""
    kc = A.shape[0]
    P = min(approx_pool(w), kc)
    pool = np.lexsort((np.arange(kc), A))[:P]
    if mutant == "no_refine":
        return pool[:w].astype(np.int32), O[pool[:w]], False
    tau = A[pool[w - 1]]
    T = threshold(tau, eps, g, mutant)
    complete = (not flag or mutant == "trust_flagged") and (P >= kc or A[pool[-1]] > T or mutant == "no_last_check")
    if not complete:
        return _pick(np.arange(kc), O, w, mutant) + (True,)
    cand = pool[:w] if mutant == "first_w" else pool[A[pool] <= T]
    return _pick(cand, O, w, mutant) + (False,)


def model_listed(A, O, w, eps, g, qn, flag=False, mutant=None):
    """select_listed over records and tile minima built from the scores A: (cells, distances, fell_back).  A phantom cell (mutant
    `phantom`: the ragged tile's rows past kc taken for centroids at the origin) has score and distance ||q||^2."""
    kc = A.shape[0]
    nt = (kc + TILE - 1) // TILE
    if mutant == "phantom" and kc % TILE:
        pad = nt * TILE - kc
        A, O = np.concatenate([A, np.full(pad, qn)]), np.concatenate([O, np.full(pad, qn, f32)])
    n = A.shape[0]
    recs = []
    for t in range(nt):
        cells = np.arange(TILE * t, min(TILE * (t + 1), n))
        recs.append(cells[np.lexsort((cells, A[cells]))[:4]])
    tmin = np.array([A[r[0]] for r in recs])
    exact = lambda: _pick(np.arange(n), O, w, mutant) + (True,)
    if (flag and mutant != "trust_flagged") or nt < w:
        return exact()
    bound = np.sort(tmin)[w - 1]
    t1 = np.nonzero(tmin < bound if mutant == "strict_gate" else tmin <= bound)[0]
    if t1.size > LISTED_MAX:
        if mutant != "truncate":
            return exact()
        t1 = t1[:LISTED_MAX]
    keys = np.sort(np.concatenate([A[recs[t]] for t in t1] + [np.zeros(0)]))
    keys = keys[keys <= bound]
    if keys.size < w:
        if mutant != "strict_gate" or keys.size == 0:
            return exact()
        tau = keys[-1]                              # (the mutant's gate left fewer than w keys and it goes on with what it has)
    else:
        tau = keys[w - 1]
    T = threshold(tau, eps, g, mutant)
    t2 = np.nonzero(tmin <= T)[0]
    if t2.size > LISTED_MAX:
        if mutant != "truncate":
            return exact()
        t2 = t2[:LISTED_MAX]
    cand = []
    for t in t2:
        r = recs[t]
        under = r[A[r] <= T]
        if r.size == 4 and A[r[3]] <= T and mutant != "no_expand":
            cand.extend(range(TILE * t, min(TILE * (t + 1), n)))
        else:
            cand.extend(under.tolist())
    return _pick(cand, O, w, mutant) + (False,)


def _seq_dist(a, b):
    acc = f32(0.0)
    for x, y in zip(a.astype(f32), b.astype(f32)):
        t = f32(x - y)
        acc = f32(acc + f32(t * t))
    return acc


def group_centre_radius(mem, mutant=None):
    """build_twolevel: the members' mean in double, rounded; the radius in double against that centre, rounded up"""
    g = mem.astype(np.float64).mean(0).astype(f32)
    r = np.sqrt(((mem.astype(np.float64) - g.astype(np.float64)[None, :]) ** 2).sum(1))
    r = r.mean() if mutant == "mean_radius" else r.max()
    return g, np.nextafter(f32(r * (1.0 + 1e-6)), f32(np.inf))


def lower_bound(gd, r, eps, mutant=None):
    """tl_lower_bound, in Float32"""
    one = f32(1.0) - f32(eps)
    s = f32(f32(np.sqrt(f32(gd))) * one) - f32(r)
    if s > 0 or mutant == "no_clamp":
        return f32(f32(s * s) * one)
    return f32(0.0)


def group_bound(mem, q, eps, mutant=None):
    g, r = group_centre_radius(mem, mutant)
    return lower_bound(_seq_dist(g, q), r, eps, mutant)


def model_twolevel(cent, groups, q, w, O, mutant=None):
    """twolevel_topw_kernel over the given grouping: (cells, distances, visited)"""
    eps = tl_eps(cent.shape[1])
    G = len(groups)
    lb = np.array([group_bound(cent[g], q, eps, mutant) for g in groups], f32)
    order = np.lexsort((np.arange(G), lb))
    first = order[:64]
    sel = []                                     # (distance bits, cell) keys offered so far
    visited = 0

    def thr():
        return sorted(sel)[w - 1][0] if len(sel) >= w else None

    def closed(b):
        t = thr()
        return t is not None and (b >= t if mutant == "break_ge" else b > t)

    def scan(gi):
        nonlocal visited
        mem = list(groups[gi])
        visited += len(mem)
        if mutant == "push_past_end" and len(mem) % 64:
            mem = mem + [mem[-1]] * (64 - len(mem) % 64)
        sel.extend((int(O[c].view(np.uint32)), int(c)) for c in mem)

    j = 0
    while j < len(first) and not closed(int(lb[first[j]].view(np.uint32))):
        scan(first[j])
        j += 1
    if j == len(first) and len(first) == 64 and G > 64 and mutant != "no_branch":
        for gi in order[64:][np.argsort(order[64:])]:           # every other group, in index order
            if not closed(int(lb[gi].view(np.uint32))):
                scan(gi)
    top = sorted(sel)[:w]
    return (np.array([c for _, c in top], np.int32), np.array([b for b, _ in top], np.uint32).view(f32), visited)


MUTANTS = {
    "no_refine": ("refine", "top-w by score, no refine"),
    "first_w": ("refine", "only the first w pool members are refined"),
    "no_eps": ("refine", "T without eps"),
    "no_gam": ("refine", "T without its relative inflation"),
    "no_last_check": ("refine", "the pool's last member is not checked against T"),
    "ties_high": ("refine", "ties go to the higher cell"),
    "trust_flagged": ("refine", "a flagged query's scores are trusted"),
    "no_expand": ("listed", "an overflow tile is not expanded"),
    "truncate": ("listed", "more than LISTED_MAX tiles are silently truncated"),
    "phantom": ("listed", "a phantom cell of the ragged tile is accepted"),
    "strict_gate": ("listed", "the tile-minimum gate is strict, and the selection goes on with the fewer keys that leaves"),
    "break_ge": ("twolevel", "the two-level visit breaks on bound >= threshold"),
    "no_clamp": ("twolevel", "the two-level bound without the s > 0 clamp"),
    "push_past_end": ("twolevel", "lanes past a group's end are pushed: a member enters twice"),
    "no_branch": ("twolevel", "no branch after 64 groups"),
    "mean_radius": ("twolevel", "radius = mean, not max, member distance"),
}


# ---- running the model on a row ---------------------------------------------------------------------------------------------------------
class Ctx:
    def __init__(self, tab, row):
        self.O = oracle_dists(tab.cent, row.q)[0]
        self.D = exact_dists(tab.cent, row.q)
        self.qn = float((row.q.astype(np.float64) ** 2).sum())
        self.flag = flagged(tab.cent, row.q)


_CTX = {}


def context(tab, row):
    key = (tab.name, row.name)
    if key not in _CTX:
        _CTX[key] = Ctx(tab, row)
    return _CTX[key]


def readers_of(tab, w):
    """(reader, form) pairs that can serve w on this table: the score-matrix reader in each form; the records where run_coarse writes
    them (bf16 or f16, at least 4 w tiles); the two-level visit on the tables that come with a grouping"""
    out = []
    if w <= 48:
        out += [("refine", f) for f in FORMS]
        if (tab.kc + TILE - 1) // TILE >= 4 * w:
            out += [("listed", f) for f in FORMS[1:]]
    if tab.groups is not None and w <= 64:
        out.append(("twolevel", "exact"))
    return out


def run(tab, row, w, reader, form, pattern="zero", mutant=None, seed=0):
    """(cells, distances, info) of the model on one row; info: fell_back (score readers) or visited (two-level)"""
    c = context(tab, row)
    if reader == "twolevel":
        return model_twolevel(tab.cent, tab.groups, row.q, w, c.O, mutant)
    listed = reader == "listed"
    eps = eps_of(form, tab.cent, row.q, listed)
    flag = c.flag and form == "f16"
    win = top_of(c.O, w)[0]
    e = adversary(pattern, tab.kc, win, eps * (1e6 if flag else 1.0), seed)       # a flagged query's scores carry no bound at all
    if listed:
        return model_listed(c.D + e, c.O, w, eps, gam(tab.d), c.qn, flag, mutant)
    return model_refine(c.D + e, c.O, w, eps, gam(tab.d), flag, mutant)
