"""GPU tests of indexes with UInt16 codes at the edges the UInt8 suite covers: every coarse stage (MFMA filters, certified refine, the
two-level search), wide probes, sub-space geometry and the LDS boundary of u16_scan_kernel, tiles of codewords that are not a power of
two, ties across passes, chunks, pairs and lists, probe pruning, extreme magnitudes, non-finite queries, the serving entries and the
encoder.  The reference is tests/u16_ref.py; ids and distance bits are compared exactly.  A test about one path asserts through
get_stats() that this path ran."""
import threading

import numpy as np
import pytest

import u16_ref
from u16_ref import assert_exact

pytestmark = pytest.mark.gpu
f32 = np.float32


def u16_index(native, ix):
    return native.IVFADCIndex.from_arrays(ix.centroids, ix.codebooks, ix.labels, ix.offsets, ix.codes, ix.ids)


def ref_of(g):
    off, codes, ids = g._lists()
    return u16_ref.U16Index(g._centroids, g._codebooks, g._labels, off, codes, ids)


def assert_fast(g):
    st = g.get_stats()
    assert st["last_qg"] >= 1 and st["last_scan_lds"] > 0, st
    return st


def assert_generic(g):
    st = g.get_stats()
    assert st["last_qg"] == -2, st
    return st


def same_bytes(a, b, what):
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), what


def generic_of(g, q, K, w):
    """The generic path's answer on the same handle (the handle's tuning is restored to automatic afterwards)."""
    g.set_tuning(-2, 0)
    r = g.search_raw(q, K, w)
    assert_generic(g)
    g.set_tuning(0, 0)
    return r


def clustered(seed, n, d, kc, m, ksub, ncl, sigma, dup=0, nq=300):
    """Centroids with the structure of a trained quantizer (ncl true centres, kc centroids scattered round them); dup: the last `dup`
    centroids are exact copies of the first ones.  Queries drawn round the same centres."""
    rng = np.random.default_rng(seed)
    centres = rng.random((ncl, d), dtype=f32)
    cent = (centres[rng.integers(0, ncl, kc)] + sigma * rng.standard_normal((kc, d))).astype(f32)
    for i in range(dup):
        cent[kc - 1 - i] = cent[i]
    ix = u16_ref.make_index(seed, n, d, kc, m, ksub, centroids=cent)
    q = (centres[rng.integers(0, ncl, nq)] + sigma * rng.standard_normal((nq, d))).astype(f32)
    return ix, q


# ---- 1. coarse stages ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["random", "near_duplicates", "offset_300", "offset_5000"])
def test_coarse_stages(native, case):
    """kc = 2048 and a batch of 4096 queries: the 128 x 128 matrix-core filter (one f16 product in mode 0 / 2 / 4 / 7, the split bf16 in
    mode 8) with its certified refine, and the two-level search (mode 6) feed the list-major u16 scan; every mode returns the exact
    kernel's bytes (mode 1), and a sample equals u16_ref.  Near duplicates (80 exact copies of one centroid, pairs one ulp apart) and a
    large common offset make the certificate fail: the exact recompute must be taken."""
    kc, d, m, nq = 2048, 32, 4, 4096
    ix = u16_ref.make_index(500 + len(case), 20000, d, kc, m, 1024)
    rng = np.random.default_rng(len(case))
    qs = rng.random((nq, d), dtype=f32)
    if case == "near_duplicates":
        ix.centroids[1:80] = ix.centroids[0]
        ix.centroids[81::2] = ix.centroids[80::2]
        ix.centroids[81::4] = np.nextafter(ix.centroids[81::4], f32(2.0))
    elif case.startswith("offset"):
        off = f32(300.0 if case.endswith("300") else 5000.0)
        ix.centroids += off
        qs += off
    qs[:16] = ix.centroids[:16]
    qs[16:24] = ix.centroids[80:88]
    res = {}
    for mode in (1, 0, 2, 8, 4, 7, 6):
        g = u16_index(native, ix)
        g.set_coarse_mode(mode)
        res[mode] = g.search_raw(qs, 10, 16)
        st = assert_fast(g)
        assert st["coarse_mfma"] == (0 if mode in (1, 6) else 1), (mode, st)
        assert st["coarse_f16"] == (1 if mode in (0, 2, 4, 7) else 0), (mode, st)
        assert st["last_twolevel"] == (1 if mode == 6 else 0), (mode, st)
        if mode in (0, 8) and case != "random":
            assert st["coarse_fallbacks"] > 0, (mode, st)
    for mode in (0, 2, 8, 4, 7, 6):
        same_bytes(res[mode], res[1], "%s: coarse mode %d differs from the exact kernel" % (case, mode))
    pick = np.concatenate([np.arange(0, 24, 3), np.sort(rng.choice(np.arange(24, nq), 16, replace=False))])
    assert_exact(tuple(a[pick] for a in res[0]), u16_ref.knn(ix, qs[pick], 10, 16), "coarse %s" % case)
    # w and K across the register-selector range: the filter (w <= 48) and the exact kernel (w = 64) against mode 1
    g0, g1 = u16_index(native, ix), u16_index(native, ix)
    g1.set_coarse_mode(1)
    sub = pick[::3]
    for w in (1, 8, 32, 48, 64):
        exp = u16_ref.knn(ix, qs[sub], 64, w)
        for K in (1, 10, 64):
            got = g0.search_raw(qs, K, w)
            st = assert_fast(g0)
            assert st["coarse_mfma"] == (1 if w <= 48 else 0), (w, st)
            same_bytes(got, g1.search_raw(qs, K, w), "%s: mode 0 vs 1, K=%d w=%d" % (case, K, w))
            assert_exact(tuple(a[sub] for a in got), tuple(x[:, :K] if x.ndim == 2 else np.minimum(x, K) for x in exp),
                         "%s K=%d w=%d" % (case, K, w))


def test_two_level_coarse_search(native):
    """The certified two-level search with u16 codes: mode 6 on a clustered kc = 2048 quantizer with duplicate centroids and queries on
    them, and automatic mode (from kc = 4096 on) on a structured kc = 8192 quantizer (kept after the self-probe; a small visited
    fraction)."""
    ix, qs = clustered(62, 20000, 32, 2048, 4, 1024, 24, 0.02, dup=40)
    qs[:40] = ix.centroids[:40]
    g = u16_index(native, ix)
    g.set_coarse_mode(6)
    ge = u16_index(native, ix)
    ge.set_coarse_mode(1)
    sub = np.concatenate([np.arange(0, 40, 4), np.arange(40, 300, 20)])
    for K, w in ((10, 1), (10, 8), (1, 32), (64, 64), (5, 48)):
        g.reset_stats()
        got = g.search_raw(qs, K, w)
        st = assert_fast(g)
        assert st["last_twolevel"] == 1 and st["twolevel_groups"] >= 32, st
        same_bytes(got, ge.search_raw(qs, K, w), "two-level vs exact K=%d w=%d" % (K, w))
        assert_exact(tuple(a[sub] for a in got), u16_ref.knn(ix, qs[sub], K, w), "two-level K=%d w=%d" % (K, w))
    # automatic mode (kc >= 4096): the quantizer of the 8-bit automatic-mode test, with 16 duplicated centroids
    ix2, q2 = clustered(63, 30000, 32, 8192, 4, 257, 256, 0.02, dup=16)
    q2[:16] = ix2.centroids[:16]
    g2 = u16_index(native, ix2)
    g2.reset_stats()
    got = g2.search_raw(q2, 10, 8)
    st = assert_fast(g2)
    assert st["last_twolevel"] == 1 and 0.0 <= st["twolevel_probe_fraction"] <= 0.02, (st["last_twolevel"], st["twolevel_probe_fraction"])
    assert st["coarse_visited"] / (q2.shape[0] * 8192.0) < 0.2, st["coarse_visited"]
    sub2 = np.concatenate([np.arange(16), np.arange(16, 300, 30)])
    assert_exact(tuple(a[sub2] for a in got), u16_ref.knn(ix2, q2[sub2], 10, 8), "automatic two-level")


# ---- 2. wide probes --------------------------------------------------------------------------------------------------------------------
def test_wide_probes(native):
    """w = 65 / 200 / 2048 through the fast kernel (the wide top-w selection), w = 2049 through the generic path; kc = 2100 with every
    third list empty, K = 10 and 64."""
    ix = u16_ref.make_index(71, 6000, 16, 2100, 2, 257, empty_every=3)
    g = u16_index(native, ix)
    q = np.random.default_rng(71).random((64, 16), dtype=f32)
    sub = np.array([0, 31, 63])
    for w in (65, 200, 2048, 2049):
        exp = u16_ref.knn(ix, q[sub], 64, w)
        for K in (10, 64):
            got = g.search_raw(q, K, w)
            if w <= 2048:
                assert_fast(g)
                same_bytes(got, generic_of(g, q, K, w), "fast vs generic K=%d w=%d" % (K, w))
            else:
                assert_generic(g)
            assert_exact(tuple(a[sub] for a in got), (exp[0][:, :K], exp[1][:, :K], np.minimum(exp[2], K)), "K=%d w=%d" % (K, w))


# ---- 3. geometry -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dsub,m,ksub", [(5, 4, 1024), (7, 4, 257), (32, 4, 1024), (64, 2, 257), (128, 2, 1024), (16, 48, 1024)])
def test_sub_space_geometry(native, dsub, m, ksub):
    """dsub outside the common set (a partial 16-byte group after full ones; 32 ... 128), and the HD shape (d = 768, m = 48, k = 1024):
    the fast kernel equals u16_ref and the generic path byte for byte."""
    d = dsub * m
    ix = u16_ref.make_index(80 + dsub, 2000 if m == 48 else 4000, d, 16, m, ksub, ndistinct=300)
    g = u16_index(native, ix)
    q = np.random.default_rng(dsub).random((16, d), dtype=f32)
    for K, w in ((10, 4), (64, 2)):
        got = g.search_raw(q, K, w)
        assert_fast(g)
        assert_exact(got, u16_ref.knn(ix, q, K, w), "dsub=%d m=%d K=%d w=%d" % (dsub, m, K, w))
        same_bytes(got, generic_of(g, q, K, w), "fast vs generic dsub=%d m=%d" % (dsub, m))


def test_lds_boundary(native):
    """u16_lds_bytes = 8 m dsp 4 + 32 768 + 144: with m = 1 the fast kernel fits 160 KB at d = 4088 (163 728 B) and not at d = 4092
    (generic path).  The generic path needs (d + 8192) 4 B: at d = 32 772 the search is refused with the LDS message, and the handle
    still encodes, appends and stays usable."""
    for d, path in ((4088, "fast"), (4092, "generic")):
        ix = u16_ref.make_index(d, 300, d, 4, 1, 257, ndistinct=40)
        g = u16_index(native, ix)
        q = np.random.default_rng(d).random((3, d), dtype=f32)
        got = g.search_raw(q, 5, 2)
        if path == "fast":
            st = assert_fast(g)
            assert st["last_scan_lds"] == 163728, st
        else:
            assert_generic(g)
        assert_exact(got, u16_ref.knn(ix, q, 5, 2), "d=%d" % d)
    from ivfadc_jl_amd import _native as nat
    d = 32772
    ix = u16_ref.make_index(5, 6, d, 2, 1, 2)
    g = u16_index(native, ix)
    q = np.random.default_rng(5).random((2, d), dtype=f32)
    with pytest.raises(nat.IVFADCError, match="LDS") as e:
        g.search_raw(q, 3, 2)
    assert e.value.code == nat.ERR_INVALID
    pts = np.random.default_rng(6).random((4, d), dtype=f32)
    gl, gc = g.encode(pts)
    el, ec = u16_ref.encode(ix, pts)
    assert np.array_equal(gl, el) and np.array_equal(gc, ec)
    g._append(pts, np.arange(100, 104, dtype=np.uint32))
    off, codes, ids = g._lists()
    assert off[-1] == 10 and sorted(ids.tolist()) == sorted(ix.ids.tolist() + [100, 101, 102, 103])
    with pytest.raises(nat.IVFADCError, match="LDS"):
        g.search_raw(q, 3, 2)


# ---- 4. tile edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ksub", [2730, 2731, 8191, 8193, 65536])
def test_tile_edges(native, ksub):
    """Tiles of T = 8192 / nvalid codewords (2730, 1638, 1365, 1170 for 3, 5, 6, 7 pairs per item): lists probed by exactly 3, 5, 6, 7, 1,
    2, 4 and 8 queries, qg = 1, 2, 4, 8, and every list holding points whose codes are the first and the last codeword of every tile and
    ksub - 1.  Those codewords are the closest, so these points are the answers.  Against u16_ref and the generic path."""
    kc, d, m, per = 8, 16, 2, 1200
    rng = np.random.default_rng(ksub)
    cent = (rng.random((kc, d), dtype=f32) * f32(4.0)).astype(f32)
    ix = u16_ref.make_index(ksub, 0, d, kc, m, ksub, centroids=cent, list_sizes=[per] * kc)
    edges = {0, ksub - 1}
    for nvalid in range(1, 9):
        T = 8192 // nvalid
        for c0 in range(0, ksub, T):
            edges.update((c0, min(ksub, c0 + T) - 1))
    edges = np.array(sorted(edges))
    assert len(edges) <= per // 2
    ix.codebooks *= f32(8.0)                                     # far codewords everywhere ...
    ix.codebooks[:, edges] *= f32(1e-3)                          # ... except at the tile edges
    for l in range(kc):
        lo = int(ix.offsets[l])
        for ii in range(m):
            sel = edges[(np.arange(len(edges)) + 3 * ii + l) % len(edges)]
            ix.codes[lo + 7:lo + 7 + len(edges), ii] = ix.labels[ii][sel]
    cnt = [3, 5, 6, 7, 1, 2, 4, 8]
    owner = np.repeat(np.arange(kc), cnt)
    q = (ix.centroids[owner] + (rng.random((owner.shape[0], d), dtype=f32) - f32(0.5)) * f32(1e-3)).astype(f32)
    g = u16_index(native, ix)
    for K, w in ((64, 1), (10, 2)):
        exp = u16_ref.knn(ix, q, K, w)
        gen = generic_of(g, q, K, w)
        assert_exact(gen, exp, "generic ksub=%d K=%d w=%d" % (ksub, K, w))
        for qg in (1, 2, 4, 8):
            g.set_tuning(qg, 0)
            got = g.search_raw(q, K, w)
            st = assert_fast(g)
            assert st["last_qg"] == qg, st
            assert_exact(got, exp, "ksub=%d K=%d w=%d qg=%d" % (ksub, K, w, qg))
            same_bytes(got, gen, "fast vs generic ksub=%d qg=%d" % (ksub, qg))
        g.set_tuning(0, 0)


# ---- 5 / 6. ties across passes, chunks, pairs and lists; probe pruning -------------------------------------------------------------------
def _tie_indexes():
    """(name, index, queries): one code row for every point (ties inside and across lists of 10 000 - 20 000 points, two lists with the
    same centroid), and zero codebooks with queries on centroids (every sum equals dc: whole lists tie across probes)."""
    rng = np.random.default_rng(55)
    d, m, kc = 16, 2, 5
    cent = rng.random((kc, d), dtype=f32)
    cent[3] = cent[1]                                            # two lists with the same dc for every query
    sizes = [12000, 15000, 10000, 20000, 11000]
    one = u16_ref.make_index(56, 0, d, kc, m, 1024, ndistinct=1, centroids=cent, list_sizes=sizes)
    zero = u16_ref.make_index(57, 0, d, kc, m, 4096, centroids=cent, list_sizes=sizes)
    zero.codebooks[:] = 0
    q = (cent[rng.integers(0, kc, 32)] + (rng.random((32, d), dtype=f32) - f32(0.5)) * f32(0.2)).astype(f32)
    qz = q.copy()
    qz[:10] = cent[[0, 1, 2, 3, 4, 1, 3, 0, 1, 3]]              # on centroids: dc = +0, twice for lists 1 and 3
    return [("one_code_row", one, q), ("zero_codebooks", zero, qz)]


def test_ties_across_passes_chunks_pairs_and_lists(native):
    """Keys of equal distance everywhere: the visit order alone decides.  Chunks of 4096 / 8192 / automatic, qg = 1 / 2 / 4 / 8, K = 1 / 10
    / 64, probe pruning on and off -- all byte-equal to the generic path, which equals u16_ref on a sample."""
    for name, ix, q in _tie_indexes():
        g = u16_index(native, ix)
        for K, w in ((1, 1), (10, 2), (64, 3)):
            gen = generic_of(g, q, K, w)
            sub = np.array([0, 1, 3, 5, 20])
            assert_exact(tuple(a[sub] for a in gen), u16_ref.knn(ix, q[sub], K, w), "%s generic K=%d w=%d" % (name, K, w))
            for qg in (1, 2, 4, 8):
                for chunk in (4096, 8192, 0):
                    for prune in (False, True):
                        g.set_pruning(prune)
                        g.set_tuning(qg, chunk)
                        g.reset_stats()
                        got = g.search_raw(q, K, w)
                        st = assert_fast(g)
                        assert st["last_qg"] == qg and (chunk == 0 or st["last_chunk"] == chunk), st
                        if not prune:
                            assert st["pruned_points"] == 0, st
                        same_bytes(got, gen, "%s K=%d w=%d qg=%d chunk=%d pruning=%s" % (name, K, w, qg, chunk, prune))
        g.set_tuning(0, 0)
        g.set_pruning(True)


def test_pruning_fires_and_changes_nothing(native):
    """A structured index (well separated cells, small codebooks, queries next to the centroids): with pruning on, points are really
    skipped (pruned_points > 0); the results are byte-equal with pruning off and equal u16_ref."""
    rng = np.random.default_rng(90)
    kc, d, m, nq = 40, 32, 4, 2048
    cent = (rng.random((kc, d), dtype=f32) * f32(4.0)).astype(f32)
    ix = u16_ref.make_index(90, 40000, d, kc, m, 1024, centroids=cent, scale=0.05)
    q = (cent[rng.integers(0, kc, nq)] + (rng.random((nq, d), dtype=f32) - f32(0.5)) * f32(0.1)).astype(f32)
    g = u16_index(native, ix)
    sub = np.arange(0, nq, 256)
    fired = 0
    for qg in (1, 4):
        for K, w in ((10, 8), (1, 16)):
            res = {}
            for prune in (False, True):
                g.set_pruning(prune)
                g.set_tuning(qg, 1024)
                g.reset_stats()
                res[prune] = g.search_raw(q, K, w)
                st = assert_fast(g)
                assert st["last_qg"] == qg, st
                if prune:
                    fired += st["pruned_points"] > 0
                else:
                    assert st["pruned_points"] == 0, st
            same_bytes(res[True], res[False], "pruning on vs off qg=%d K=%d w=%d" % (qg, K, w))
            assert_exact(tuple(a[sub] for a in res[True]), u16_ref.knn(ix, q[sub], K, w), "pruned qg=%d K=%d w=%d" % (qg, K, w))
    assert fired > 0


# ---- 7. extreme magnitudes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["outlier_codewords", "zero_codebooks", "tiny_scale", "huge_scale", "dc_dominates_300", "dc_dominates_5000",
                                  "dc_zero_huge_entries", "overflow"])
def test_extreme_magnitudes(native, case):
    """The cases of the 8-bit test_integer_filter_extremes, plus `overflow`: codebooks of about 1e20, so every table entry and every sum
    is +inf and the visit order alone orders the keys.  The fast kernel and the generic path, both against u16_ref."""
    d, m, kc = 32, 4, 12
    ix = u16_ref.make_index(1400 + len(case), 20000, d, kc, m, 1024)
    rng = np.random.default_rng(len(case))
    qs = rng.random((48, d), dtype=f32)
    if case == "outlier_codewords":
        ix.codebooks[:, 7, :] *= f32(1000.0)
    elif case == "zero_codebooks":
        ix.codebooks[:] = 0
        qs[:8] = ix.centroids[:8]
    elif case == "tiny_scale":
        ix.codebooks *= f32(1e-21)
        ix.centroids *= f32(1e-21)
        qs *= f32(1e-21)
    elif case == "huge_scale":
        ix.codebooks *= f32(1e15)
        ix.centroids *= f32(1e15)
        qs *= f32(1e15)
    elif case.startswith("dc_dominates"):
        off = f32(300.0 if case.endswith("300") else 5000.0)
        ix.centroids += off
        ix.codebooks *= f32(1e-3)
        qs[24:] += off
    elif case == "dc_zero_huge_entries":
        ix.codebooks *= f32(1e3)
        qs[:12] = ix.centroids[:12]
    elif case == "overflow":
        u = rng.random(ix.codebooks.shape, dtype=f32)
        ix.codebooks[:] = np.where(u < 0.5, f32(-1.0), f32(1.0)) * (f32(1.0) + u) * f32(1e20)
    exp = u16_ref.knn(ix, qs, 10, 4)
    if case == "overflow":
        assert np.isinf(exp[1]).all()
    g = u16_index(native, ix)
    got = g.search_raw(qs, 10, 4)
    assert_fast(g)
    assert_exact(got, exp, "fast %s" % case)
    assert_exact(generic_of(g, qs, 10, 4), exp, "generic %s" % case)


# ---- 8. non-finite queries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["fast", "generic", "coarse_filter"])
def test_non_finite_queries_are_contained(native, plan):
    """The u16 twin of the 8-bit containment test: rows with NaN / +-inf / +-3e38 components get valid counts and stored ids, every
    finite query of the same batch equals u16_ref, and the handle answers a clean batch exactly afterwards."""
    d = 32
    ix = u16_ref.make_index(53, 6000, d, 256 if plan == "coarse_filter" else 64, 4, 1024)
    g = u16_index(native, ix)
    if plan == "generic":
        g.set_tuning(-2, 0)
    elif plan == "coarse_filter":
        g.set_coarse_mode(2)
    rng = np.random.default_rng(5)
    nq = 96
    qs = rng.random((nq, d), dtype=f32)
    bad = {1: np.nan, 3: np.inf, 4: -np.inf, 6: 3e38, 7: -3e38}
    qs[0, :] = np.nan
    for r, v in bad.items():
        qs[r, (7 * r) % d] = v
    qs[9, :] = np.inf
    bad_rows = sorted([0, 9] + list(bad))
    good = np.array([r for r in range(nq) if r not in bad_rows])
    K, w = 10, 4
    valid_ids = set(ix.ids.tolist())
    exp = u16_ref.knn(ix, qs[good], K, w)
    for rep in range(2):
        ids, dists, counts = g.search_raw(qs, K, w)
        st = g.get_stats()
        if plan == "generic":
            assert st["last_qg"] == -2, st
        else:
            assert st["last_qg"] >= 1 and st["last_scan_lds"] > 0, st
            assert st["coarse_mfma"] == (1 if plan == "coarse_filter" else 0), st
        assert ((counts >= 0) & (counts <= K)).all()
        for r in bad_rows:
            assert set(ids[r, :counts[r]].tolist()) <= valid_ids, (plan, r, ids[r])
        assert_exact((ids[good], dists[good], counts[good]), exp, "finite queries beside non-finite ones (%s)" % plan)
    q2 = rng.random((33, d), dtype=f32)
    assert_exact(g.search_raw(q2, K, w), u16_ref.knn(ix, q2, K, w), "after non-finite batches (%s)" % plan)


# ---- 9. serving entries ----------------------------------------------------------------------------------------------------------------
def test_serving_entries(native):
    """Next-batch hints, search_batches_raw beside a live view, device-pointer searches alternating between the index and a view on their
    own streams, two Python threads on one index, and a push that makes a live view stale.  The u16 path never takes the query-major
    rider: last_rider stays 0 and the bytes are the same."""
    import torch
    ix = u16_ref.make_index(99, 8000, 32, 32, 4, 1024, ndistinct=500)
    g = u16_index(native, ix)
    rng = np.random.default_rng(99)
    q = rng.random((300, 32), dtype=f32)
    K, w = 10, 6
    exp = g.search_raw(q, K, w)
    assert_fast(g)
    assert_exact(tuple(a[:12] for a in exp), u16_ref.knn(ix, q[:12], K, w), "search_raw")
    dq = torch.from_numpy(q).cuda()

    def dev_out():
        return (torch.zeros((300, K), dtype=torch.int32, device="cuda"), torch.zeros((300, K), dtype=torch.float32, device="cuda"),
                torch.zeros(300, dtype=torch.int32, device="cuda"))

    def host(o):
        return o[0].cpu().numpy().view(np.uint32), o[1].cpu().numpy(), o[2].cpu().numpy()

    # a hint for the search after the next one, then both searches
    torch.cuda.synchronize()
    g.set_next_queries(300, dq.data_ptr(), 7)
    o1, o2 = dev_out(), dev_out()
    torch.cuda.synchronize()
    g.search_device(300, dq.data_ptr(), K, w, o1[0].data_ptr(), o1[1].data_ptr(), o1[2].data_ptr())
    assert g.get_stats()["last_rider"] == 0
    g.set_query_token(7)
    g.search_device(300, dq.data_ptr(), K, w, o2[0].data_ptr(), o2[1].data_ptr(), o2[2].data_ptr())
    g.sync()
    assert g.get_stats()["last_rider"] == 0
    assert_exact(host(o1), exp, "hinted search")
    assert_exact(host(o2), exp, "search after the hint")
    # search_batches_raw while a view exists; device-pointer searches alternating between the index and the view
    v = g.clone_view()
    outs = g.search_batches_raw([q[:70], q[70:71], q[71:]], K, w)
    assert_exact(tuple(np.concatenate([o[i] for o in outs]) for i in range(3)), exp, "search_batches beside a view")
    assert g.get_stats()["last_rider"] == 0
    outs_g = [dev_out() for _ in range(3)]
    outs_v = [dev_out() for _ in range(3)]
    torch.cuda.synchronize()
    for og, ov in zip(outs_g, outs_v):
        g.search_device(300, dq.data_ptr(), K, w, og[0].data_ptr(), og[1].data_ptr(), og[2].data_ptr())
        v.search_device(300, dq.data_ptr(), K, w, ov[0].data_ptr(), ov[1].data_ptr(), ov[2].data_ptr())
    g.sync()
    v.sync()
    for og, ov in zip(outs_g, outs_v):
        assert_exact(host(og), exp, "index on its stream")
        assert_exact(host(ov), exp, "view on its stream")
    # two Python threads, different batch sizes, one index
    sets = [q[:7], q[:300], q[40:81], q[5:6], q[100:250]]
    exp_sets = [tuple(a[s] for a in exp) for s in (slice(0, 7), slice(0, 300), slice(40, 81), slice(5, 6), slice(100, 250))]
    errs = []

    def worker(order):
        try:
            for _ in range(5):
                for i in order:
                    ids, dists = native.knn_search(g, sets[i], K, w=w)
                    ei, ed, ec = exp_sets[i]
                    for r in range(sets[i].shape[0]):
                        c = int(ec[r])
                        assert np.array_equal(ids[r], ei[r, :c].astype(ids[r].dtype)), (i, r)
                        assert np.array_equal(dists[r].view(np.uint32), ed[r, :c].view(np.uint32)), (i, r)
        except Exception as e:      # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=worker, args=(o,)) for o in ([0, 1, 2, 3, 4], [4, 3, 1, 0, 2])]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs[0]
    # a push makes the live view stale; a fresh view and the index answer the new reference
    new = (ix.centroids[[2, 5]] + f32(0.001)).astype(f32)
    g._append(new, np.array([8000, 8001], np.uint32))
    with pytest.raises(Exception, match="changed since this view"):
        v.search_raw(q[:2], K, w)
    ref = ref_of(g)
    exp2 = u16_ref.knn(ref, q[:40], K, w)
    assert_exact(g.search_raw(q[:40], K, w), exp2, "index after push")
    assert_exact(g.clone_view().search_raw(q[:40], K, w), exp2, "fresh view after push")


# ---- 10. encoder -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["ksub65536_dsub1", "on_codewords", "d4088_m1"])
def test_encoder_edges(native, case):
    """encode_u16_kernel: ksub = 65536 with dsub = 1 (many exact ties, duplicate codewords far past index 256), points exactly on codewords,
    and d = 4088 with m = 1 (the per-sub-space minima behind a 16 KB residual); permuted labels throughout.  encode equals u16_ref.encode
    in lists and labels; an _append followed by a search equals the reference built from _lists()."""
    rng = np.random.default_rng(len(case))
    if case == "ksub65536_dsub1":
        d, m, kc, ksub = 2, 2, 6, 65536
    elif case == "on_codewords":
        d, m, kc, ksub = 32, 4, 16, 4096
    else:
        d, m, kc, ksub = 4088, 1, 4, 257
    ix = u16_ref.make_index(300 + len(case), 0, d, kc, m, ksub)
    if case == "ksub65536_dsub1":
        ix.codebooks[:, 40000] = ix.codebooks[:, 300]
        ix.codebooks[:, 65535] = ix.codebooks[:, 70]
        ix.codebooks[:, 1000:1100] = ix.codebooks[:, 60000:60100]
    if case == "on_codewords":
        ix.codebooks[:, 3000] = ix.codebooks[:, 17]             # a codeword on which points lie, twice
    n = 40 if case == "d4088_m1" else 400
    pts = rng.random((n, d), dtype=f32)
    if case == "ksub65536_dsub1":
        pts[:100] = ix.centroids[rng.integers(0, kc, 100)] + ix.codebooks[:, [300, 70, 60000, 60050]].T.repeat(25, 0).reshape(100, m)
    else:
        lst = rng.integers(0, kc, n)
        cw = rng.integers(0, ksub, (n, m))
        cw[::3] = 17
        pts[: n // 2] = (ix.centroids[lst] + ix.codebooks[np.arange(m), cw].reshape(n, d))[: n // 2]
    pts = pts.astype(f32)
    g = native.IVFADCIndex.from_arrays(ix.centroids, ix.codebooks, ix.labels, index_type=np.uint32)
    gl, gc = g.encode(pts)
    el, ec = u16_ref.encode(ix, pts)
    assert np.array_equal(gl, el), np.nonzero(gl != el)[0][:8]
    assert np.array_equal(gc, ec), np.argwhere(gc != ec)[:8]
    g._append(pts, np.arange(n, dtype=np.uint32))
    ref = ref_of(g)
    q = (pts[:6] + f32(0.003)).astype(f32)
    assert_exact(g.search_raw(q, 10, 2), u16_ref.knn(ref, q, 10, 2), "search after append (%s)" % case)
    assert_fast(g)
