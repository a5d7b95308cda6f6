"""GPU tests of the table-free entries of the UInt16 list scan (csrc/u16scan.hip.h: u16_direct_scan_kernel, K <= 64, and
u16_direct_wide_scan_kernel, 64 < K under table mode 10), reached through set_u16_tables(1 / 2) only.  What is new is the accumulate
phase: every point gathers the codeword its code names and forms its own table entry, in the entry's accumulator and order.  Every
comparison is exact -- counts, ids and distance bits -- against the same handle's generic path and against tests/u16_ref.py, and every
search asserts through get_stats() which form ran: last_striped 6 / 7 and last_scan_lds equal to a restatement of the new byte counts."""
import os
import re

import numpy as np
import pytest

import helpers
import u16_ref
from u16_ref import assert_exact
from test_gpu_u16_edges import _tie_indexes, assert_fast, assert_generic, clustered, generic_of, ref_of, same_bytes, u16_index

pytestmark = pytest.mark.gpu
f32 = np.float32
LDS_MAX = 160 << 10


def cap_of(K):
    p = 1
    while p < K + 64:
        p <<= 1
    return max(128, p)


def small_lds(m, dsub):
    """u16_lds_bytes (the table form, K <= 64)."""
    return 8 * m * ((dsub + 3) & ~3) * 4 + 32768 + 4 * 8 * 4 + 16


def direct_lds(m, dsub):
    """u16_direct_lds_bytes: residuals of 8 pairs (dsub rounded up to 4), the 16 KB wave-merge exchange, per-wave counts, two words."""
    return 8 * m * ((dsub + 3) & ~3) * 4 + 4 * 8 * 64 * 8 + 4 * 8 * 4 + 16


def direct_wide_lds(m, dsub, qg, cap):
    """u16_direct_wide_lds_bytes: residuals, selbuf[4 waves][qg][cap] u64, per-wave counts, two words."""
    return 8 * m * ((dsub + 3) & ~3) * 4 + 4 * qg * cap * 8 + 4 * 8 * 4 + 16


def planned_wide_qg(m, dsub, qg, K):
    while qg > 1 and direct_wide_lds(m, dsub, qg, cap_of(K)) > LDS_MAX:
        qg >>= 1
    return qg


def direct(g, q, K, w, qg=0, chunk=0):
    """A search that must have run the K <= 64 table-free entry: the results and the stats."""
    g.set_tuning(qg, chunk)
    got = g.search_raw(q, K, w)
    st = assert_fast(g)
    assert st["last_striped"] == 6, st
    assert st["last_scan_lds"] == direct_lds(g.m, g.d // g.m), st
    if qg:
        assert st["last_qg"] == qg, st
    if chunk:
        assert st["last_chunk"] == chunk, st
    g.set_tuning(0, 0)
    return got, st


def direct_wide(g, q, K, w, qg=0, chunk=0):
    g.set_tuning(qg, chunk)
    got = g.search_raw(q, K, w)
    st = assert_fast(g)
    assert st["last_striped"] == 7, st
    assert st["last_scan_lds"] == direct_wide_lds(g.m, g.d // g.m, st["last_qg"], cap_of(K)), st
    if qg:
        assert st["last_qg"] == planned_wide_qg(g.m, g.d // g.m, qg, K), st
    g.set_tuning(0, 0)
    return got, st


# ---- 1. the form runs and is exact -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_lists(native):
    ix = u16_ref.make_index(4242, 40000, 32, 4, 4, 1024, perm_labels=True, ndistinct=5000)
    g = u16_index(native, ix)
    q = np.random.default_rng(9).random((96, 32), dtype=f32)
    g.set_u16_tables(1)
    return ix, g, q


@pytest.mark.parametrize("w", [1, 4])
@pytest.mark.parametrize("K", [1, 10, 64])
def test_the_form_runs_and_is_exact(long_lists, K, w):
    """Four lists of ~10 000 points (several passes per chunk, several chunks, exact ties), 96 queries, forced qg 1 / 2 / 4 / 8 with chunks
    of 4096 and automatic, and the plan's own grouping: last_striped == 6, less LDS than the table form, the generic path's bytes, which
    equal numpy on the first 8 queries."""
    ix, g, q = long_lists
    gen = generic_of(g, q, K, w)
    assert_exact(tuple(a[:8] for a in gen), u16_ref.knn(ix, q[:8], K, w), "generic vs numpy K=%d w=%d" % (K, w))
    for qg in (1, 2, 4, 8):
        for chunk in (4096, 0):
            got, st = direct(g, q, K, w, qg, chunk)
            assert st["last_scan_lds"] < small_lds(4, 8), st
            assert_exact(got, gen, "K=%d w=%d qg=%d chunk=%d" % (K, w, qg, chunk))
            same_bytes(got, gen, "bytes K=%d w=%d qg=%d chunk=%d" % (K, w, qg, chunk))
    got, st = direct(g, q, K, w)
    same_bytes(got, gen, "automatic K=%d w=%d" % (K, w))


# ---- 2. sub-space geometry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dsub,m,ksub", [(1, 4, 65536), (5, 4, 1024), (6, 16, 1024), (7, 4, 257), (32, 4, 1024), (64, 2, 257), (128, 2, 1024),
                                         (16, 48, 1024)])
def test_sub_space_geometry(native, dsub, m, ksub):
    """Partial 16-byte groups (dsub 5, 6, 7), one-term codewords (dsub 1, k = 65536, codeword indices 0 and 65535 in probed lists),
    streamed codewords (32 ... 128) and the HD stride (m = 48)."""
    d = dsub * m
    ix = u16_ref.make_index(180 + dsub, 3000, d, 3, m, ksub, ndistinct=0 if ksub == 65536 else 300)
    if ksub == 65536:
        for l in range(3):                         # the first and the last codeword, in every list and sub-space
            lo = int(ix.offsets[l])
            ix.codes[lo + 1] = ix.labels[:, 0]
            ix.codes[lo + 2] = ix.labels[:, ksub - 1]
            ix.codes[lo + 3, ::2] = ix.labels[::2, 0]
            ix.codes[lo + 3, 1::2] = ix.labels[1::2, ksub - 1]
        assert (ix.inv[np.arange(m), ix.codes[int(ix.offsets[1]) + 2]] == ksub - 1).all()
    g = u16_index(native, ix)
    g.set_u16_tables(1)
    q = np.random.default_rng(dsub).random((16, d), dtype=f32)
    for K, w in ((10, 3), (64, 2)):
        exp = u16_ref.knn(ix, q[:8], K, w)
        gen = generic_of(g, q, K, w)
        assert_exact(tuple(a[:8] for a in gen), exp, "generic dsub=%d m=%d" % (dsub, m))
        for qg in (1, 8, 0):
            got, _ = direct(g, q, K, w, qg)
            same_bytes(got, gen, "dsub=%d m=%d ksub=%d K=%d w=%d qg=%d" % (dsub, m, ksub, K, w, qg))


# ---- 3. list ends ------------------------------------------------------------------------------------------------------------------------
def test_list_ends_and_stale_rows(native):
    """Lists that end everywhere round a wave, a 256-point row, a pass and a chunk; then ids are deleted so that stale rows lie behind several
    list_len, a few points are appended in place, and the searches are repeated against the handle's own lists.  An unpredicated gather,
    or a read of a lane without a point, shows here."""
    sizes = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097]
    kc, d, m = len(sizes), 16, 2
    ix = u16_ref.make_index(333, 0, d, kc, m, 1024, list_sizes=sizes)
    g = u16_index(native, ix)
    g.set_u16_tables(1)
    rng = np.random.default_rng(3)
    q = rng.random((24, d), dtype=f32)

    def check(ref, what):
        for K in (1, 64):
            exp = u16_ref.knn(ref, q[:8], K, kc)
            gen = generic_of(g, q, K, kc)
            assert_exact(tuple(a[:8] for a in gen), exp, "%s generic K=%d" % (what, K))
            for qg in (1, 8):
                got, _ = direct(g, q, K, kc, qg)
                same_bytes(got, gen, "%s K=%d qg=%d" % (what, K, qg))

    check(ix, "fresh")
    gone = []
    for l in (2, 4, 7, 9, 10, 13, 14):            # the last rows of these lists go stale, and some in the middle
        lo, hi = int(ix.offsets[l]), int(ix.offsets[l + 1])
        gone += ix.ids[max(lo, hi - 3):hi].tolist() + ix.ids[lo:lo + 1].tolist()
    assert g._delete_ids(np.array(sorted(set(gone)), np.uint32)) == len(set(gone))
    check(ref_of(g), "after delete")
    g._append(rng.random((5, d), dtype=f32), np.arange(100000, 100005, dtype=np.uint32))
    check(ref_of(g), "after append")


# ---- 4. ties -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_ties(native, which):
    """One code row everywhere / zero codebooks: the visit order alone decides."""
    name, ix, q = _tie_indexes()[which]
    g = u16_index(native, ix)
    g.set_u16_tables(1)
    sub = np.array([0, 1, 3, 5, 20])
    for K, w in ((1, 1), (10, 2), (64, 3)):
        gen = generic_of(g, q, K, w)
        assert_exact(tuple(a[sub] for a in gen), u16_ref.knn(ix, q[sub], K, w), "%s generic K=%d w=%d" % (name, K, w))
        for qg in (1, 4, 8):
            for chunk in (4096, 0):
                got, _ = direct(g, q, K, w, qg, chunk)
                same_bytes(got, gen, "%s K=%d w=%d qg=%d chunk=%d" % (name, K, w, qg, chunk))


# ---- 5. extremes and containment ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["overflow", "zero_codebooks", "non_finite_queries"])
def test_extremes_and_containment(native, case):
    """Codebooks of about 1e20 (every sum +inf), zero codebooks, queries with NaN / +-inf / +-3e38 rows: the bytes of the same handle under
    mode 0, valid counts and stored ids."""
    d, m, kc = 32, 4, 12
    ix = u16_ref.make_index(1500 + len(case), 20000, d, kc, m, 1024)
    rng = np.random.default_rng(len(case))
    qs = rng.random((48, d), dtype=f32)
    if case == "overflow":
        u = rng.random(ix.codebooks.shape, dtype=f32)
        ix.codebooks[:] = np.where(u < 0.5, f32(-1.0), f32(1.0)) * (f32(1.0) + u) * f32(1e20)
    elif case == "zero_codebooks":
        ix.codebooks[:] = 0
        qs[:8] = ix.centroids[:8]
    else:
        qs[0, :] = np.nan
        for r, v in {1: np.nan, 3: np.inf, 4: -np.inf, 6: 3e38, 7: -3e38}.items():
            qs[r, (7 * r) % d] = v
        qs[9, :] = np.inf
    g = u16_index(native, ix)
    K, w = 10, 4
    base = g.search_raw(qs, K, w)
    st = assert_fast(g)
    assert st["last_striped"] == 0 and st["last_scan_lds"] == small_lds(m, d // m), st
    g.set_u16_tables(1)
    valid_ids = set(ix.ids.tolist())
    for qg in (0, 1, 8):
        got, _ = direct(g, qs, K, w, qg)
        ids, dists, counts = got
        assert ((counts >= 0) & (counts <= K)).all()
        for r in range(qs.shape[0]):
            assert set(ids[r, :counts[r]].tolist()) <= valid_ids, (case, r)
        if qg == 0:
            same_bytes(got, base, "%s: table-free vs tables" % case)
        good = np.arange(10, 48)
        assert_exact(tuple(a[good] for a in got), tuple(a[good] for a in base), "%s qg=%d" % (case, qg))
    if case == "overflow":
        assert np.isinf(base[1]).all()
    if case != "non_finite_queries":
        assert_exact(tuple(a[:8] for a in base), u16_ref.knn(ix, qs[:8], K, w), case)


# ---- 6. pruning --------------------------------------------------------------------------------------------------------------------------
def test_pruning_changes_nothing(native):
    ix, q = clustered(91, 40000, 32, 40, 4, 1024, 8, 0.02, nq=512)
    g = u16_index(native, ix)
    g.set_u16_tables(1)
    sub = np.arange(0, 512, 64)
    exp = u16_ref.knn(ix, q[sub], 10, 8)
    fired = 0
    for qg in (1, 4):
        res = {}
        for prune in (False, True):
            g.set_pruning(prune)
            g.reset_stats()
            res[prune], st = direct(g, q, 10, 8, qg, 1024)
            if prune:
                fired += st["pruned_points"] > 0
            else:
                assert st["pruned_points"] == 0, st
        same_bytes(res[True], res[False], "pruning on vs off qg=%d" % qg)
        assert_exact(tuple(a[sub] for a in res[True]), exp, "pruned qg=%d" % qg)
    assert fired > 0


# ---- 7. the wide form --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [65, 100, 1000, 2048])
def test_wide_form(long_lists, K):
    """Table mode 10 and 64 < K: last_striped == 7, the wide restatement's LDS, the generic path's bytes; without table mode 10 the same K
    runs the generic path.  K = 2048 (cap = 4096, 128 KB of selectors at qg = 1) is past the table form's reach and inside this one's."""
    ix, g, q = long_lists
    w = 4
    gen = generic_of(g, q, K, w)
    assert_exact(tuple(a[:8] for a in gen), u16_ref.knn(ix, q[:8], K, w), "generic vs numpy K=%d" % K)
    same_bytes(g.search_raw(q, K, w), gen, "without table mode 10")
    assert_generic(g)
    g.set_table_mode(10)
    try:
        for qg in (1, 8, 0):
            for chunk in (4096, 0):
                got, st = direct_wide(g, q, K, w, qg, chunk)
                same_bytes(got, gen, "K=%d qg=%d chunk=%d" % (K, qg, chunk))
    finally:
        g.set_table_mode(0)


# ---- 8. serving entries ------------------------------------------------------------------------------------------------------------------
def test_serving_entries(native):
    from ivfadc_jl_amd import _native as nat
    ix = u16_ref.make_index(78, 8000, 32, 32, 4, 1024, perm_labels=True)
    g = u16_index(native, ix)
    q = np.random.default_rng(2).random((300, 32), dtype=f32)
    K, w = 10, 8
    before = g.clone_view()
    g.set_u16_tables(1)
    after = g.clone_view()
    exp, _ = direct(g, q, K, w)
    assert_exact(tuple(x[:8] for x in exp), u16_ref.knn(ix, q[:8], K, w), "search_raw")
    same_bytes(after.search_raw(q, K, w), exp, "view taken after the switch")
    st = assert_fast(after)
    assert st["last_striped"] == 6 and st["last_scan_lds"] == direct_lds(4, 8), st
    same_bytes(before.search_raw(q, K, w), exp, "view taken before the switch")
    st = assert_fast(before)
    assert st["last_striped"] == 0 and st["last_scan_lds"] == small_lds(4, 8), st
    before.set_u16_tables(1)                      # ... and a view takes its own setting afterwards
    same_bytes(before.search_raw(q, K, w), exp, "view switched itself")
    assert assert_fast(before)["last_striped"] == 6
    assert assert_fast(g)["last_striped"] == 6
    lists, dcs = g.coarse_search_raw(q, w)
    same_bytes(g.search_preassigned_raw(q, K, lists, dcs), exp, "preassigned")
    st = assert_fast(g)
    assert st["last_striped"] == 6 and st["last_scan_lds"] == direct_lds(4, 8), st
    outs = g.search_batches_raw([q[:100], q[100:101], q[101:]], K, w)
    same_bytes(tuple(np.concatenate([o[i] for o in outs]) for i in range(3)), exp, "search_batches")
    assert assert_fast(g)["last_striped"] == 6
    whole, _ = direct(g, q, 64, 32)               # ~18 KB of workspace per query: the smallest limit (1 MiB) cuts 300 into sub-batches
    g.set_workspace_limit(1 << 20)
    g.reset_stats()
    same_bytes(g.search_raw(q, 64, 32), whole, "sub-batches")
    st = assert_fast(g)
    assert st["last_striped"] == 6 and st["queries"] == 300, st
    g.set_workspace_limit(1 << 30)
    with pytest.raises(nat.IVFADCError) as e:
        g.set_list_partition(2, 0)
    assert e.value.code == nat.ERR_INVALID


# ---- 9. one handle, form after form ------------------------------------------------------------------------------------------------------
def test_form_after_form(native):
    ix = u16_ref.make_index(79, 12000, 32, 6, 4, 1024, ndistinct=2000)
    g = u16_index(native, ix)
    q = np.random.default_rng(4).random((64, 32), dtype=f32)
    K, w = 10, 3
    gen = generic_of(g, q, K, w)
    gen100 = generic_of(g, q, 100, w)
    assert_exact(tuple(a[:8] for a in gen), u16_ref.knn(ix, q[:8], K, w), "generic vs numpy")

    def tables():
        got = g.search_raw(q, K, w)
        st = assert_fast(g)
        assert st["last_striped"] == 0 and st["last_scan_lds"] == small_lds(4, 8), st
        same_bytes(got, gen, "mode 0")

    g.set_u16_tables(0)
    tables()
    g.set_u16_tables(1)
    same_bytes(direct(g, q, K, w)[0], gen, "mode 1")
    g.set_u16_tables(0)
    tables()
    g.set_table_mode(10)
    g.set_u16_tables(1)
    same_bytes(direct_wide(g, q, 100, w)[0], gen100, "wide, table-free")
    same_bytes(generic_of(g, q, K, w), gen, "generic again")
    same_bytes(direct(g, q, K, w)[0], gen, "mode 1 again")


# ---- 10. what the switch must not touch --------------------------------------------------------------------------------------------------
def test_8bit_handle_and_invalid_modes(native):
    from ivfadc_jl_amd import _native as nat
    oidx, data = helpers.build_index(15, 4000, 64, 40, 8, ksub=256, label_perm=True, mode="random", ndistinct=300)
    g = native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)
    assert g.code_type == np.uint8
    q = data[:48] + 0.01
    keys = ("last_qg", "last_chunk", "last_scan_lds", "last_striped", "last_nf")
    for K, w in ((10, 4), (100, 8)):
        res = {}
        for mode in (0, 1, 2):
            g.set_u16_tables(mode)
            got = g.search_raw(q, K, w)
            st = g.get_stats()
            res[mode] = (got, tuple(st[k] for k in keys))
        for mode in (1, 2):
            assert res[0][1] == res[mode][1], (K, mode, res[0][1], res[mode][1])
            same_bytes(res[0][0], res[mode][0], "8-bit K=%d: mode %d vs mode 0" % (K, mode))
    for h in (g, u16_index(native, u16_ref.make_index(5, 100, 8, 2, 2, 300))):
        for mode in (-1, 3, 11):
            with pytest.raises(nat.IVFADCError) as e:
                h.set_u16_tables(mode)
            assert e.value.code == nat.ERR_INVALID


# ---- 11. mode 2 --------------------------------------------------------------------------------------------------------------------------
def test_mode_2_follows_the_rule(native):
    """Two indexes on either side of min(avg_len, 1024) * U16_DIRECT_COST <= ksub, the constant read from the source."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ivfadc.jl_amd", "csrc", "scan_layouts.h")).read()   # (u16scan.hip.h includes it)
    cost = float(re.search(r"constexpr float U16_DIRECT_COST = ([0-9.]+)f;", src).group(1))
    assert cost >= 1.0
    d, m, kc = 16, 2, 4
    # avg_len = 50: table-free iff 50 cost <= ksub.  ksub on either side; cost < 20.48 keeps the first side non-empty below ksub = 1024
    ks_free = int(np.ceil(50 * cost)) + 1
    ks_tab = max(2, int(np.floor(50 * cost)) - 1)
    assert 50 * cost <= ks_free <= 65536 and 50 * cost > ks_tab
    q = np.random.default_rng(6).random((32, d), dtype=f32)
    for ksub, free in ((ks_free, True), (ks_tab, False)):
        ix = u16_ref.make_index(600 + ksub, 200, d, kc, m, ksub)
        g = u16_index(native, ix)
        g.set_u16_tables(2)
        for K, w in ((10, 2), (64, 4)):
            got = g.search_raw(q, K, w)
            st = assert_fast(g)
            assert st["last_striped"] == (6 if free else 0), (ksub, st)
            assert st["last_scan_lds"] == (direct_lds(m, 8) if free else small_lds(m, 8)), st
            assert_exact(tuple(a[:8] for a in got), u16_ref.knn(ix, q[:8], K, w), "mode 2 ksub=%d" % ksub)
            same_bytes(got, generic_of(g, q, K, w), "mode 2 ksub=%d vs generic" % ksub)
