"""GPU parity tests of the eight-wave list-major kernel (csrc/wg8scan.hip.h) at the sub-space widths beside the SIFT1B one: m = 8 and
d = 32 / 64 / 96 (dsub = 4 / 8 / 12; wg8_scan_kernel<NQ, DS>), both forms (four and eight queries per code stream).  Only the residual
fill and the table build know the width -- the residuals' row stride, the codebook's group offsets, the order of the sum over the
sub-space's dimensions -- and a mistake in any of them changes distance bits on the first query: every comparison is with the CPU
oracle, ids exact and distance bits identical (helpers.assert_same_results).  The kernel is forced as tests/test_gpu_wg8.py forces it
(set_tuning(4, chunk) + table mode 6 / 7) and every search asserts that it ran (last_striped, two workgroups' worth of LDS)."""
import os

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

M = 8
# (table mode, last_striped, queries per code stream) of the two forms
FORMS = {"q4": (6, 2, 4), "q8": (7, 3, 8)}
NEW_D = (32, 64, 96)
# The plan's own choice (no tuning, no table mode) on long lists, per d: True = the eight-wave kernel.  d = 128 is the measured SIFT1B
# shape; the narrower sub-spaces run the kernel on request only (not timed against the four-wave kernel yet).
DEFAULT_EIGHT_WAVE = {32: False, 64: False, 96: False, 128: True}


def gpu_index(native, oidx):
    return native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)


def wg8_index(native, oidx, form, chunk=0):
    g = gpu_index(native, oidx)
    g.set_tuning(4, chunk)
    g.set_table_mode(FORMS[form][0])
    return g


def ran_eight_wave(g, form, what=""):
    st = g.get_stats()
    assert st["last_striped"] == FORMS[form][1] and st["last_qg"] == FORMS[form][2] and st["last_scan_lds"] <= 80 * 1024, (what, st)


def same_bits(got, exp, what):
    helpers.assert_same_results(got, exp, what=what)
    assert np.array_equal(got[1][exp[1] < np.inf].view(np.uint32), exp[1][exp[1] < np.inf].view(np.uint32)), what


@pytest.mark.parametrize("case", ["random", "permuted_labels", "few_codes", "short_lists", "exact_hits"])
@pytest.mark.parametrize("form", ["q4", "q8"])
@pytest.mark.parametrize("d", NEW_D)
def test_eight_wave_kernel_other_widths(native, d, form, case):
    """14 lists of ~2 100 points and 61 queries: groups that are full, partial and several per list, one chunk and several per list,
    K = 1 / 10 / 17 / 64; permuted labels; lists of four distinct codes (ties across whole steps); 300 lists of ~100 points (idle waves,
    empty lists); queries that are centroid + codewords (table entries of 0).  Then nine queries on the same handle."""
    kc = 300 if case == "short_lists" else 14
    n = 30000
    oidx, _ = helpers.build_index(2600 + d + len(case), n, d, kc, M, 256, label_perm=(case == "permuted_labels"), mode="random",
                                  ndistinct=(4 if case == "few_codes" else None))
    rng = np.random.default_rng(277 + d + len(case))
    qs = rng.random((61, d), dtype=np.float32)
    if case == "exact_hits":
        for i in range(16):
            code = rng.integers(0, 256, M)
            qs[i] = oidx.centroids[i % kc] + np.concatenate([oidx.codebooks[ii, code[ii]] for ii in range(M)])
    for K, w, chunk in ((10, 3, 0), (1, 1, 1024), (64, 5, 4096), (17, 2, 2048)):
        what = "wg8 d=%d %s %s K=%d w=%d chunk=%d" % (d, form, case, K, w, chunk)
        exp = oidx.knn_search(qs, K, w)
        g = wg8_index(native, oidx, form, chunk)
        got = g.search_raw(qs, K, w)
        ran_eight_wave(g, form, what)
        same_bits(got, exp, what)
        got2 = g.search_raw(qs[:9], K, w)
        ran_eight_wave(g, form, what + ", second call")
        same_bits(got2, tuple(a[:9] for a in exp), what + ", second call")


@pytest.mark.parametrize("case", ["zero_codebooks", "tiny_scale", "huge_scale", "dc_dominates_5000"])
@pytest.mark.parametrize("form", ["q4", "q8"])
@pytest.mark.parametrize("d", NEW_D)
def test_eight_wave_kernel_other_widths_filter_extremes(native, d, form, case):
    """The filter's quantisation is built from the new tables: whatever their scale does -- all-zero tables (every point ties; the scale is
    not a normal number), entries in the denormal range, entries near the top of the float range, sums dominated by the coarse distance --
    it may only let MORE points through.  Set up as test_eight_wave_kernel_filter_extremes."""
    kc = 12
    oidx, _ = helpers.build_index(1500 + d + len(case), 40000, d, kc, M, 256, mode="random")
    rng = np.random.default_rng(d + len(case))
    if case == "zero_codebooks":
        oidx.codebooks[:] = 0
    elif case == "tiny_scale":
        oidx.codebooks *= np.float32(1e-21)
        oidx.centroids *= np.float32(1e-21)
    elif case == "huge_scale":
        oidx.codebooks *= np.float32(1e15)
        oidx.centroids *= np.float32(1e15)
    qs = rng.random((64, d), dtype=np.float32)
    if case == "dc_dominates_5000":
        oidx.centroids += np.float32(5000.0)
        oidx.codebooks *= np.float32(1e-3)
        qs[32:] += np.float32(5000.0)
    elif case == "tiny_scale":
        qs *= np.float32(1e-21)
    elif case == "huge_scale":
        qs *= np.float32(1e15)
    elif case == "zero_codebooks":
        qs[:8] = oidx.centroids[:8]
    for K, w in ((10, 4), (64, 2)):
        what = "wg8 filter d=%d %s %s K=%d" % (d, form, case, K)
        g = wg8_index(native, oidx, form, 8192)
        got = g.search_raw(qs, K, w)
        ran_eight_wave(g, form, what)
        same_bits(got, oidx.knn_search(qs, K, w), what)


@pytest.mark.parametrize("form", ["q4", "q8"])
def test_fuzz_eight_wave_kernel_other_widths(native, form):
    """test_fuzz_eight_wave_kernel's draws with d drawn from 32 / 64 / 96 as well: list counts and sizes from empty lists to a few thousand
    points, chunk sizes that give partial last steps and several chunks per list, K from 1 to 64, w up to kc, batches that leave partial
    groups, permuted labels, few distinct codes, pruning on and off, one push and one delete between searches.  Against the oracle, ids
    exact and distance bits equal.  IVFADC_FUZZ_DRAWS / IVFADC_FUZZ_SEED widen it for soak runs."""
    from oracle import oracle as ora
    rng = np.random.default_rng(int(os.environ.get("IVFADC_FUZZ_SEED", "8086")) + FORMS[form][2])
    for it in range(int(os.environ.get("IVFADC_FUZZ_DRAWS", "12"))):
        d = int(rng.choice(NEW_D))
        kc = int(rng.choice([1, 2, 5, 14, 33, 120]))
        n = int(rng.choice([0, 7, 300, 3000, 20000, 45000]))
        K = int(rng.choice([1, 2, 8, 9, 10, 16, 17, 33, 64]))
        w = int(rng.choice([1, 2, 3, 8, 14, 200]))
        nq = int(rng.choice([1, 4, 5, 37, 130]))
        chunk = int(rng.choice([0, 0, 1024, 2048, 8192]))
        oidx, data = helpers.build_index(7100 + it, n, d, kc, M, 256, label_perm=bool(rng.random() < 0.4),
                                         mode="encode" if (n and n <= 3000 and rng.random() < 0.4) else "random",
                                         ndistinct=(3 if rng.random() < 0.25 else None))
        qs = rng.random((nq, d), dtype=np.float32)
        if n:
            qs[: min(nq, 3)] = data[: min(nq, 3)]
        if rng.random() < 0.2:
            qs += np.float32(20.0)
        g = wg8_index(native, oidx, form, chunk)
        if rng.random() < 0.3:
            g.set_pruning(0)
        what = "wg8 fuzz %d (%s): d=%d kc=%d n=%d K=%d w=%d nq=%d chunk=%d" % (it, form, d, kc, n, K, w, nq, chunk)
        got = g.search_raw(qs, K, w)
        assert g.get_stats()["last_striped"] == FORMS[form][1], what
        same_bits(got, oidx.knn_search(qs, K, w), what)
        if it % 3 == 0:
            npush = int(rng.choice([1, 9, 200]))
            pts = rng.random((npush, d), dtype=np.float32)
            g._append(pts, np.arange(n, n + npush, dtype=np.uint32))
            if n + npush > 2:
                g._delete_ids(rng.integers(0, n + npush, int(rng.choice([1, 5, 60]))).astype(np.uint32))
            offsets, codes, ids = g._lists()
            o2 = ora.OracleIndex(oidx.centroids, oidx.codebooks, oidx.labels, offsets, codes, ids)
            same_bits(g.search_raw(qs, K, w), o2.knn_search(qs, K, w), what + " after edits")


@pytest.mark.parametrize("form", ["q4", "q8"])
def test_eight_wave_kernel_width_16_unchanged(native, form):
    """d = 128 through the kernel that is now a template on the width: the bytes of the reference-order kernel (table mode 1) and of the
    oracle, as before."""
    d, kc = 128, 14
    oidx, _ = helpers.build_index(2500 + len("random"), 30000, d, kc, M, 256, mode="random")
    qs = np.random.default_rng(177 + len("random")).random((61, d), dtype=np.float32)
    gref = gpu_index(native, oidx)
    gref.set_tuning(4, 0)
    gref.set_table_mode(1)
    for K, w, chunk in ((10, 3, 0), (1, 1, 1024), (64, 5, 4096), (17, 2, 2048)):
        what = "wg8 d=128 %s K=%d w=%d chunk=%d" % (form, K, w, chunk)
        g = wg8_index(native, oidx, form, chunk)
        got = g.search_raw(qs, K, w)
        ran_eight_wave(g, form, what)
        same_bits(got, oidx.knn_search(qs, K, w), what)
        ref = gref.search_raw(qs, K, w)
        assert gref.get_stats()["last_striped"] not in (2, 3)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), what + ": against the reference-order kernel"


@pytest.mark.parametrize("d", NEW_D)
def test_default_plan_other_widths(native, d):
    """No set_tuning, no table mode, on the smallest index whose lists count as long (sixteen lists of 33 000 points, 96 queries; w = 1 is
    6 probes per list, w = 2 is 12): the plan takes the eight-wave kernel where DESIGN.md 4.4 documents a measured win for the width and
    keeps the four-wave kernel elsewhere; the oracle's results either way."""
    kc, n = 16, 16 * 33000
    oidx, _ = helpers.build_index(5200 + d, n, d, kc, M, 256, mode="random")
    qs = np.random.default_rng(52 + d).random((96, d), dtype=np.float32)
    g = gpu_index(native, oidx)
    for w in (1, 2):
        got = g.search_raw(qs, 10, w)
        st = g.get_stats()
        print("default plan d = %d, w = %d: last_striped = %d, last_qg = %d" % (d, w, st["last_striped"], st["last_qg"]))
        if DEFAULT_EIGHT_WAVE[d]:
            form = "q8" if w == 2 else "q4"
            assert st["last_striped"] == FORMS[form][1] and st["last_qg"] == FORMS[form][2], st
        else:
            assert st["last_striped"] not in (2, 3), st
        same_bits(got, oidx.knn_search(qs, 10, w), "default plan d=%d w=%d" % (d, w))
