"""The offer-order rule of the query-major scan and the stand-alone top-w, as a numpy model; no GPU.

A register selector (kernels.hip.h: WSel<true>) is offered 64 keys at a time, one per lane.  Empty, it adopts the K smallest of an
offer of 16 or more candidates in one wave sort (the seed); afterwards every key below its K-th key is one serial insertion, in lane
order, each against the bound the insertion before it left.  What it holds in the end is the K smallest keys of everything it was
offered -- whatever the order -- but the NUMBER of insertions depends on the order:

* register order: the first offer is an arbitrary 64 of the n keys; the rest cost about K ln(n / 64) insertions;
* minima first: every lane sorts its own keys (the scan) or takes its minimum out (the top-w) and the first offer is the 64 lane
  minima; the K-th smallest of them has about K (1 + 1 / 64) of the n keys below it, K of them in the seed.

The model counts insertions for both orders on seeded random keys, asserts that both end with the same K keys (the K smallest) and
that minima first needs fewer insertions on average at the two shapes of the flagship step: 256 points per wave step at K = 10 and a
1024-entry row at w = 8.  The averages are printed; none is asserted beyond the comparison."""
import numpy as np
import pytest

KEY_MAX = (1 << 64) - 1
SEED_MIN = 16          # WSel<true>::push seeds an empty selector from an offer of at least this many candidates


class Selector:
    """WSel<true> at wave level: `top` = the sorted keys held (at most 64; the first K are the result), thr = min(K-th key, bound)."""

    def __init__(self, K, bound=KEY_MAX):
        self.K, self.top, self.ext, self.thr = K, [], bound, bound
        self.insertions = self.seeds = 0

    def _kth(self):
        return self.top[self.K - 1] if len(self.top) >= self.K else KEY_MAX

    def push(self, keys):
        """one offer: keys[lane] or None"""
        cand = [k for k in keys if k is not None and k < self.thr]
        if not cand:
            return
        if len(cand) >= SEED_MIN and not self.top:
            self.seeds += 1
            self.top = sorted(cand)[:self.K]
            self.thr = min(self._kth(), self.ext)
            return
        for k in keys:             # lane order; every lane is re-tested against the bound the insertion before it left
            if k is None or not k < self.thr:
                continue
            self.insertions += 1
            self.top = sorted(self.top + [k])[:64]
            self.thr = min(self._kth(), self.ext)

    def result(self):
        return self.top[:self.K]


def keys_of(rng, n, ndistinct=None):
    """n unique keys: random f32 bit patterns of non-negative values (few distinct ones on request: ties) over the position"""
    vals = rng.random(n, dtype=np.float32)
    if ndistinct:
        vals = vals[rng.integers(0, ndistinct, n)]
    return [(int(b) << 32) | p for p, b in enumerate(vals.view(np.uint32))]


def scan_offers(keys, ppl, minima_first):
    """a wave step of 64 * ppl points: lane l holds the keys at positions point(r, l); offers r = 0 .. ppl - 1.  The position map is the
    m = 8 kernel's (CodeRegs<8, 4>::point): (r >> 1) * 128 + 2 l + (r & 1); a short list leaves None."""
    lanes = []
    for l in range(64):
        mine = []
        for r in range(ppl):
            p = (r >> 1) * 128 + 2 * l + (r & 1)
            mine.append(keys[p] if p < len(keys) else KEY_MAX)
        lanes.append(sorted(mine) if minima_first else mine)
    return [[lanes[l][r] if lanes[l][r] != KEY_MAX else None for l in range(64)] for r in range(ppl)]


def row_offers(keys, minima_first):
    """a row of up to 1024 entries on one wave: lane l holds entries u * 256 + 4 l + e (u, e in 0 .. 3); offers in (u, e) order,
    behind the lane minima where they go first (the minimum is then left out of its own offer)"""
    def at(l, u, e):
        c = u * 256 + 4 * l + e
        return keys[c] if c < len(keys) else None
    offers, taken = [], {}
    if minima_first:
        first = []
        for l in range(64):
            mine = [(at(l, u, e), (u, e)) for u in range(4) for e in range(4) if at(l, u, e) is not None]
            k, where = min(mine) if mine else (None, None)
            first.append(k)
            taken[l] = where
        offers.append(first)
    for u in range(4):
        for e in range(4):
            offers.append([None if taken.get(l) == (u, e) else at(l, u, e) for l in range(64)])
    return offers


def run(offers, K, bound=KEY_MAX):
    s = Selector(K, bound)
    for o in offers:
        s.push(o)
    return s


@pytest.mark.parametrize("n,K,ppl", [(256, 10, 4), (256, 1, 4), (256, 64, 4), (255, 10, 4), (65, 10, 4), (5, 10, 4), (128, 10, 2)])
def test_scan_step_same_set_either_order(n, K, ppl):
    for seed in range(40):
        rng = np.random.default_rng(1000 * n + seed)
        keys = keys_of(rng, n, ndistinct=(3 if seed % 4 == 3 else None))
        bound = KEY_MAX if seed % 5 else sorted(keys)[len(keys) // 2]          # a bound from outside: only keys below it count
        want = [k for k in sorted(keys) if k < bound][:K]
        a, b = run(scan_offers(keys, ppl, False), K, bound), run(scan_offers(keys, ppl, True), K, bound)
        assert a.result() == want and b.result() == want, (n, K, seed)
        assert a.thr == b.thr


@pytest.mark.parametrize("kc,w", [(1024, 8), (1024, 1), (1024, 64), (1000, 9), (256, 32), (64, 8), (64, 64), (8, 9)])
def test_row_same_set_either_order(kc, w):
    for seed in range(40):
        rng = np.random.default_rng(7000 * kc + seed)
        keys = keys_of(rng, kc, ndistinct=(2 if seed % 4 == 3 else None))
        want = sorted(keys)[:w]
        a, b = run(row_offers(keys, False), w), run(row_offers(keys, True), w)
        assert a.result() == want and b.result() == want, (kc, w, seed)


def test_minima_first_inserts_less_at_the_flagship_shapes():
    trials = 300
    scan = np.zeros((trials, 2))
    row = np.zeros((trials, 2))
    for t in range(trials):
        rng = np.random.default_rng(424200 + t)
        keys = keys_of(rng, 256)
        scan[t] = [run(scan_offers(keys, 4, mf), 10).insertions for mf in (False, True)]
        keys = keys_of(rng, 1024)
        row[t] = [run(row_offers(keys, mf), 8).insertions for mf in (False, True)]
    print("insertions per wave step (256 points, K = 10): register order %.2f, lane minima first %.2f   [K ln(256 / 64) = %.1f]" % (
        scan[:, 0].mean(), scan[:, 1].mean(), 10 * np.log(4)))
    print("insertions per row (1024 entries, w = 8): block order %.2f, lane minima first %.2f   [w ln(1024 / 64) = %.1f]" % (
        row[:, 0].mean(), row[:, 1].mean(), 8 * np.log(16)))
    assert scan[:, 1].mean() < scan[:, 0].mean()
    assert row[:, 1].mean() < row[:, 0].mean()
