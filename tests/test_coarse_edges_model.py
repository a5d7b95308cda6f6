"""CPU side of the coarse-edge suite (tests/coarse_edges.py; the GPU side is tests/test_gpu_coarse_edges.py): the table has teeth.

1. Every family's premise holds, exactly: the clusters' Float32 distances are rho + j ulp in reverse cell order, everything else lies at
   >= 4 rho, T_max(form) < 2 rho and 4 rho > 2 T_max for the f32, bf16 and f16 forms -- so a score-matrix reader's certificate passes
   for t <= P - 1 near-ties and fails for t >= P whatever the kernel's rounding does.
2. The model -- refine_probes, select_listed, the two-level visit, restated over adversarial scores -- returns the oracle's rows on
   every row under every adversary.
3. Every one of coarse_edges.MUTANTS returns a wrong row somewhere in the table; the rows that catch it are printed.
4. What uniform-random quantizers of the same sizes catch is printed beside it (nothing is asserted about it).  Measured: 7 of the 16
   mutants -- no_refine, first_w, no_eps, no_last_check, strict_gate, and push_past_end / no_branch through group lengths that are
   no multiple of 64 -- and none of no_gam, ties_high, trust_flagged, no_expand, truncate, phantom, break_ge, no_clamp, mean_radius;
   the table catches 16 of 16."""
import numpy as np
import pytest

import coarse_edges as ce
from oracle import oracle as ora

f32 = np.float32
TABLES = ("pool", "small", "small64", "gap", "records", "tiles", "norm", "clumps", "twins", "stray", "normal")


def _same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(np.asarray(got[1], f32).view(np.uint32), np.asarray(exp[1], f32).view(np.uint32))


def _expected(tab, row, w):
    return ce.top_of(ce.context(tab, row).O, w)


# ---- 1. premises ------------------------------------------------------------------------------------------------------------------------
def test_the_numpy_reference_is_the_c_oracle():
    for name in ("pool", "records", "clumps", "norm"):
        tab = ce.table(name)
        z = np.zeros((1, 1, tab.d), f32)
        oidx = ora.OracleIndex(tab.cent, z, np.zeros((1, 1), np.uint8), np.zeros(tab.kc + 1, np.int64), np.zeros((0, 1), np.uint8), np.zeros(0, np.uint32))
        for row in tab.rows:
            w = min(64, tab.kc)
            cl, dd = oidx.coarse_search(row.q, w)
            assert _same((cl, dd), _expected(tab, row, w)), (name, row)
        qs = np.stack([r.q for r in tab.rows])
        got = ce.oracle_rows(tab.cent, qs, 9)
        for i, row in enumerate(tab.rows):
            assert _same((got[0][i], got[1][i]), _expected(tab, row, 9)), (name, row)


@pytest.mark.parametrize("name", ["pool", "small64", "gap", "records", "tiles", "norm", "clumps", "normal"])
def test_the_filler_reference_is_the_c_oracle(name):
    """The GPU file checks its filler rows against coarse_edges.oracle_rows: on that very filler (coarse_edges.filler_of), every query of
    it, oracle_rows is the C oracle's coarse_search -- at the largest w the GPU file asks for; a smaller w is a prefix."""
    tab = ce.table(name)
    fq = ce.filler_of(tab)
    w = 65 if tab.groups is not None else 48
    lists, dists = ce.oracle_rows(tab.cent, fq, w)
    z = np.zeros((1, 1, tab.d), f32)
    oidx = ora.OracleIndex(tab.cent, z, np.zeros((1, 1), np.uint8), np.zeros(tab.kc + 1, np.int64), np.zeros((0, 1), np.uint8), np.zeros(0, np.uint32))
    for r in range(fq.shape[0]):
        assert _same(oidx.coarse_search(fq[r], w), (lists[r], dists[r])), (name, r)


def _t_max(form, tab, q, tau_max, listed=False):
    eps = ce.eps_of(form, tab.cent, q, listed)
    return ce.threshold(tau_max + eps, eps, ce.gam(tab.d)), eps


@pytest.mark.parametrize("name", ["pool", "small", "small64"])
def test_pool_edge_premise(name):
    tab = ce.table(name)
    assert float(np.abs(tab.cent).max()) == 2.0 and ce.f16_scale(tab.cent) == 2048.0
    seen = set()
    for row in tab.rows:
        m = row.meta
        if m["family"] != "pool":
            continue
        (w,) = row.ws
        t, P = m["t"], m["P"]
        assert P == ce.approx_pool(w) == {1: 17, 8: 24, 16: 32, 24: 48, 32: 64, 48: 64}[w]
        seen.add((w, t - P, m["equal"]))
        c = ce.context(tab, row)
        lo, hi = m["cells"]
        inside = np.zeros(tab.kc, bool)
        inside[lo:hi] = True
        # the cluster: rho + j ulp, j = t - 1 ... 0 in cell order (equal: rho), the real distances ordered likewise
        want = np.full(t, ce.RHO) if m["equal"] else ce.RHO + np.arange(t - 1, -1, -1) * ce.ULP_RHO
        assert np.array_equal(c.O[lo:hi].astype(np.float64), want), row
        if not m["equal"]:
            assert (np.diff(c.D[lo:hi]) < 0).all() and np.abs(c.D[lo:hi] - want).max() < 1e-3 * ce.ULP_RHO
        # everyone else
        assert c.O[~inside].min() >= 4 * ce.RHO and c.D[~inside].min() >= 4 * ce.RHO, row
        # the oracle's w-th cell is the cluster's highest cell that is among the winners: winners = the last w cells, nearest = highest
        cl, _ = _expected(tab, row, w)
        if t >= w:
            assert np.array_equal(cl, np.arange(lo, lo + w) if m["equal"] else np.arange(hi - 1, hi - 1 - w, -1)), row
        for form in ce.FORMS:
            Tmax, eps = _t_max(form, tab, row.q, ce.RHO + t * ce.ULP_RHO)
            assert Tmax < 2 * ce.RHO and 4 * ce.RHO > 2 * Tmax, (row, form, Tmax)
            # t <= P - 1: the pool's last member is not of the cluster, its score >= 4 rho - eps > T.  t >= P: the pool is all cluster,
            # last score <= rho + (t - 1) ulp + eps, and T >= (rho - eps + eps)(1 + gam) + eps: fails when (t - 1) ulp <= rho gam
            assert 4 * ce.RHO - eps > Tmax
            assert (t - 1) * ce.ULP_RHO <= ce.RHO * ce.gam(tab.d)
            assert not ce.flagged(tab.cent, row.q)
    ws = ce.POOL_WS if name == "pool" else (1, 8)
    assert seen == {(w, dt, False) for w in ws for dt in (-2, -1, 0, 1)} | {(w, dt, True) for w in ws for dt in (-1, 0)}


@pytest.mark.parametrize("name", ["pool", "small", "small64", "gap"])
def test_the_filler_beside_the_pool_edge_rows_passes_every_certificate(name):
    """The GPU file counts fallbacks on batches of pool-edge rows and filler: its filler (coarse_edges.safe_filler) passes in every form
    at every w under every adversary -- shown by the model on a sample, by the inequality on all of it."""
    tab = ce.table(name)
    ws = sorted({w for r in tab.rows if r.meta["family"] in ("pool", "gap") for w in r.ws})
    fq = ce.filler_of(tab)
    assert fq.shape == (1024, tab.d) and ce.filler_passes(tab, fq, ws).all() and np.abs(fq).max() <= 2.0
    plain = ce.filler_passes(tab, ce.filler_queries(2048, tab.d, 12), ws)
    print("%s: %d of 2048 uniform queries pass every certificate provably" % (name, plain.sum()))
    for i in range(0, 1024, 128):
        row = ce.Row("filler %d" % i, fq[i], ws, family="filler")
        for w in ws:
            for form in ce.FORMS:
                for pattern in ce.ADVERSARIES:
                    got = ce.run(tab, row, w, "refine", form, pattern, seed=i)
                    assert not got[2] and _same(got[:2], _expected(tab, row, w)), (name, i, w, form, pattern)
        ce._CTX.pop((tab.name, row.name))


def test_gap_sweep_premise():
    tab = ce.table("gap")
    assert float(np.abs(tab.cent).max()) == 2.0
    w, P = ce.GAP_W, ce.approx_pool(ce.GAP_W)
    ks = {f: [] for f in ce.FORMS}
    for row in tab.rows:
        m = row.meta
        c = ce.context(tab, row)
        if "pair" in m:       # the rounding tie at w = 1: lower cell farther, same Float32 sum, each alone among far cells in its own tile
            lo, hi = m["pair"]
            assert row.ws == (1,) and lo // ce.TILE < hi // ce.TILE and c.O[lo] == c.O[hi] and 0 < c.D[lo] - c.D[hi] < 0.5 * ce.gam(tab.d) * ce.RHO
            assert _expected(tab, row, 1)[0][0] == lo and np.sort(c.D)[2] >= 4 * ce.RHO
            continue
        lo, hi = m["cells"]
        n = m["beyond"]
        assert row.ws == (w,) and hi - lo == n + w
        order = np.lexsort((np.arange(tab.kc), c.D))
        assert sorted(order[:n + w].tolist()) == list(range(lo, hi)) and c.D[order[n + w]] >= 4 * ce.RHO
        assert (c.D[hi - w:hi - 1] < 1.001).all() and order[w - 1] == hi - 1           # the w-th: the site's highest cell
        assert sorted(order[w:w + n].tolist()) == list(range(lo, lo + n))              # the next n: its lowest
        if "k" in m:
            assert c.D[hi - 1] == ce.RHO and n == P - w + 1                            # ... enough of them to be the pool's last member
            eps = ce.eps_of(m["form"], tab.cent, row.q)
            assert np.abs((c.D[lo:lo + n] - ce.RHO) / (eps * 2.0 ** m["k"]) - 1).max() < 1e-6 and c.D[lo] < 2.5 * ce.RHO
            ks[m["form"]].append(m["k"])
        else:       # the rounding tie: same Float32 sum, the lower cell really farther -- by less than the relative inflation covers
            assert c.O[lo] == c.O[hi - 1] and c.D[lo] > c.D[hi - 1]
            assert c.D[lo] - c.D[hi - 1] < 0.5 * ce.gam(tab.d) * ce.RHO
            assert _expected(tab, row, w)[0][-1] == lo
    assert all(ks[f] == list(range(-6, 4)) for f in ce.FORMS)


def test_records_premise():
    tab = ce.table("records")
    assert tab.kc % 64 and tab.kc % 128
    for row in tab.rows:
        m = row.meta
        c = ce.context(tab, row)
        if m["family"] != "records":
            continue
        Tmax, eps = _t_max("f16", tab, row.q, ce.RHO + 64 * ce.ULP_RHO, listed=True)
        under = np.nonzero(c.D <= 2 * ce.RHO)[0]
        assert Tmax < 2 * ce.RHO and (c.D[np.setdiff1d(np.arange(tab.kc), under)] >= 4 * ce.RHO).all() and 4 * ce.RHO - eps > Tmax
        tiles = np.unique(under // ce.TILE)
        if "n" in m:
            assert under.size == m["n"] and tiles.size == 1 and (m["n"] != 64 or under[0] % ce.TILE == 0), row
            assert _expected(tab, row, 1)[0][0] == under[-1]
        elif "numbers" in m:
            assert sorted(under.tolist()) == sorted(m["numbers"]) and tiles.size == 8 and c.D[m["numbers"][7]] == ce.RHO and (c.D[m["numbers"][:7]] < 1.001).all()
        elif row.name.startswith("records: 8 winners"):
            assert under.size == 8 and tiles.size == 2, row
        elif m.get("origin"):
            assert under.tolist() == [tab.kc - 3, tab.kc - 2, tab.kc - 1] and c.qn == 0.0 and _expected(tab, row, 1)[0][0] == tab.kc - 1
        else:
            assert under.tolist() == [tab.kc - 4]
    big = ce.table("tiles")
    assert big.kc >= 8320
    for row in big.rows:
        c = ce.context(big, row)
        Tmax, eps = _t_max("f16", big, row.q, ce.RHO + 129 * ce.ULP_RHO, listed=True)
        under = np.nonzero(c.D <= 2 * ce.RHO)[0]
        n = row.meta["n"]
        assert Tmax < 2 * ce.RHO and 4 * ce.RHO - eps > Tmax
        assert under.size == n and np.unique(under // ce.TILE).size == n and c.D[np.setdiff1d(np.arange(big.kc), under)].min() >= 4 * ce.RHO
        assert _expected(big, row, 1)[0][0] == under[-1]                                # the nearest in the highest tile
    assert sorted(r.meta["n"] for r in big.rows) == [127, 128, 129] and ce.LISTED_MAX == 128


def test_norms_and_signs_premise():
    tab = ce.table("pool")
    row = tab.row("on a cell: twins")
    a, b, c3 = row.meta["twins"]
    assert b == a + 1 and np.array_equal(tab.cent[a], tab.cent[b]) and np.array_equal(tab.cent[a], tab.cent[c3])
    assert sorted(_expected(tab, row, 3)[0].tolist()) == sorted([a, b, c3]) and (_expected(tab, row, 3)[1] == 0).all()
    cmax = ce.cmaxn_of(tab.cent)
    far = tab.row("far outside, 8 ||c||")
    assert np.sqrt(ce.context(tab, far).qn) > 7.5 * cmax and not ce.flagged(tab.cent, far.q)
    for r in tab.rows:
        if "flagged" in r.meta:
            assert ce.flagged(tab.cent, r.q) == r.meta["flagged"], r
    big = ce.table("norm")
    norms = np.sqrt((big.cent.astype(np.float64) ** 2).sum(1))
    assert np.sort(norms)[-1] == 1024 * np.sort(norms)[-2]
    for r in big.rows:           # eps is set by a cell far from every query -- and is larger than every distance that matters
        c = ce.context(big, r)
        assert int(np.argmax(norms)) not in _expected(big, r, 48)[0] and ce.eps_of("f32", big.cent, r.q) > c.O[_expected(big, r, 48)[0]].max()


def test_two_level_premise():
    tab = ce.table("clumps")
    assert sorted(len(g) for g in tab.groups) == sorted(ce.CLUMPS) and tab.kc == sum(ce.CLUMPS) and max(16, tab.kc // 64) == len(tab.groups)
    eps = ce.tl_eps(tab.d)
    cr = [ce.group_centre_radius(tab.cent[g]) for g in tab.groups]
    # well separated: every member is closer to its own centre than to any other by a factor of 5
    for gi, g in enumerate(tab.groups):
        dd = np.array([[np.sqrt(((tab.cent[c].astype(np.float64) - ctr) ** 2).sum()) for ctr, _ in cr] for c in g])
        own = dd[:, gi].copy()
        dd[:, gi] = np.inf
        assert (5 * own <= dd.min(1)).all()
    zero = tab.row("two-level: champions tie across clumps")
    c = ce.context(tab, zero)
    champs = [int(g[-1]) for g in tab.groups if len(g) >= 2]
    assert (c.O[champs] == 392.0).all() and np.sort(c.O)[len(champs)] > 392.0
    bounds = [float(ce.group_bound(tab.cent[g], zero.q, eps)) for g in tab.groups]
    assert (np.diff(bounds) <= 0).all() and bounds[0] > bounds[-1]                   # the lowest cells lie in the clump with the largest bound
    spread = tab.row("two-level: winners spread over w clumps")
    cl, dd = _expected(tab, spread, 8)
    owner = {int(cc): gi for gi, g in enumerate(tab.groups) for cc in g}
    assert len({owner[int(x)] for x in cl}) == 8 and (np.diff(dd) > 0).all()
    inside = tab.row("two-level: inside the clump of 128")
    gi = next(i for i, g in enumerate(tab.groups) if len(g) == 128)
    assert bounds is not None and float(ce.group_bound(tab.cent[tab.groups[gi]], inside.q, eps)) == 0.0
    assert ce._seq_dist(cr[gi][0], inside.q) < cr[gi][1] ** 2
    for n in (2, 63, 64, 65, 129):       # the winner is the group's last member
        r = tab.row("two-level: next to the last member of the clump of %d" % n)
        g = next(g for g in tab.groups if len(g) == n)
        assert _expected(tab, r, 1)[0][0] == g[-1]
    tw = ce.table("twins")
    r = tw.rows[0]
    lo, hi = r.meta["twins"]
    assert lo < hi and np.array_equal(tw.cent[lo], tw.cent[hi]) and hi in tw.groups[0] and lo in tw.groups[-1]
    assert float(ce.group_bound(tw.cent[tw.groups[0]], r.q, eps)) == 0.0 == float(ce.group_bound(tw.cent[tw.groups[-1]], r.q, eps))
    nm = ce.table("normal")
    assert len(nm.groups) == 65 and nm.kc == 4160


# ---- 2. the model is the oracle ---------------------------------------------------------------------------------------------------------
def _cases(tab):
    for row in tab.rows:
        for w in row.ws:
            if w > tab.kc:
                continue
            for reader, form in ce.readers_of(tab, w):
                yield row, w, reader, form


@pytest.mark.parametrize("name", TABLES)
def test_the_model_is_the_oracle_under_every_adversary(name):
    tab = ce.table(name)
    n = 0
    for row, w, reader, form in _cases(tab):
        exp = _expected(tab, row, w)
        for pattern in ce.ADVERSARIES if reader != "twolevel" else ("zero",):
            got = ce.run(tab, row, w, reader, form, pattern, seed=n)
            assert _same(got[:2], exp), (name, row, w, reader, form, pattern, got[0], exp[0])
            n += 1
            # the pool edge: the certificate passes for t <= P - 1 and falls back for t >= P, under every adversary
            if reader == "refine" and row.meta["family"] == "pool":
                assert got[2] == (row.meta["t"] >= row.meta["P"]), (row, form, pattern)
    print("%s: %d (row, w, reader, form, adversary) cases" % (name, n))


def test_w_65_leaves_every_certified_path():
    assert ce.readers_of(ce.table("clumps"), 65) == [] and ("twolevel", "exact") in ce.readers_of(ce.table("clumps"), 64)


# ---- 3. every mutant is caught ----------------------------------------------------------------------------------------------------------
def _catches(tabs, mutant):
    kind = ce.MUTANTS[mutant][0]
    hits = []
    for name in tabs:
        tab = tabs[name] if isinstance(tabs, dict) else ce.table(name)
        for row, w, reader, form in _cases(tab):
            if reader != kind and not (kind == "refine" and reader == "listed" and mutant in ("no_eps", "no_gam", "ties_high", "trust_flagged")):
                continue
            exp = _expected(tab, row, w)
            for pattern in ce.ADVERSARIES if reader != "twolevel" else ("zero",):
                if not _same(ce.run(tab, row, w, reader, form, pattern, mutant, seed=len(hits))[:2], exp):
                    hits.append("%s / %s / w=%d / %s %s / %s" % (tab.name, row, w, reader, form, pattern))
                    break
    return hits


@pytest.mark.parametrize("mutant", list(ce.MUTANTS))
def test_every_mutant_is_caught(mutant):
    hits = _catches(TABLES, mutant)
    print("%s (%s): caught by %d cases: %s%s" % (mutant, ce.MUTANTS[mutant][1], len(hits), "; ".join(hits[:6]), " ..." if len(hits) > 6 else ""))
    assert hits, "no row catches `%s` (%s) -- a hole in the table" % (mutant, ce.MUTANTS[mutant][1])


def test_there_are_at_least_fourteen_mutants():
    assert len(ce.MUTANTS) >= 14 and {k for k, _ in ce.MUTANTS.values()} == {"refine", "listed", "twolevel"}


# ---- 4. the control ---------------------------------------------------------------------------------------------------------------------
def test_what_uniform_random_quantizers_catch():
    """Uniform-random quantizers of the table's sizes (kc = 384, 2088, 8320; for the two-level visit kc = 740 in 16 groups and kc = 4160 in
    65, by cell number) with uniform queries at the table's w: printed, not asserted."""
    rng = np.random.default_rng(99)
    tabs = {}
    for kc, grouped in ((384, False), (2088, False), (8320, False), (740, True), (4160, True)):
        cent = rng.random((kc, ce.D), dtype=f32)
        rows = [ce.Row("uniform %d" % i, rng.random(ce.D, dtype=f32), (1, 8, 48) if not grouped else (1, 8, 64), family="filler") for i in range(3)]
        step = (kc + 15) // 16 if kc == 740 else 64                 # 16 groups as the clump table has, 65 as the normal one
        groups = [np.arange(g0, min(g0 + step, kc)) for g0 in range(0, kc, step)] if grouped else None
        tabs["random kc=%d" % kc] = ce.Table("random kc=%d%s" % (kc, " grouped" if grouped else ""), cent, rows, groups)
    seen = {m: len(_catches(tabs, m)) for m in ce.MUTANTS}
    caught = [m for m, n in seen.items() if n]
    print("uniform-random quantizers catch %d of %d mutants: %s; never: %s" % (len(caught), len(seen), {m: seen[m] for m in caught},
                                                                              [m for m in seen if not seen[m]]))
