"""GPU parity tests of the eight-wave list-major kernel's WIDE-POOL form (csrc/wg8scan.hip.h, wg8_wide_scan_kernel<NQ, DS>: two pool entries
per lane, 64 < K <= 128), reached through table modes 8 / 9 (as 6 / 7, and the wide form above K = 64).  What is new in the kernel is the
pool -- entries l and l + 64 per lane, the swap target chosen over two ballots, the snapshot patched in the half that was addressed -- its
initialisation and the hand-over of both halves; the cold-start bounds take K-th sums deeper into a step than K <= 64 ever did.  A mistake
in any of them loses or duplicates a key: every comparison is with the CPU oracle, ids exact and distance bits identical.  The kernel is
forced as tests/test_gpu_wg8_dsub.py forces it (set_tuning(4, chunk) + the table mode) and every search asserts which kernel ran:
last_striped 4 / 5 (four / eight queries per code stream), last_qg 4 / 8, two workgroups' worth of LDS."""
import os

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

M = 8
# (table mode, last_striped of the wide form, queries per code stream, the narrow mode, last_striped of the narrow form)
FORMS = {"q4": (8, 4, 4, 6, 2), "q8": (9, 5, 8, 7, 3)}
ALL_D = (32, 64, 96, 128)
_CACHE = {}


def gpu_index(native, oidx):
    return native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)


def wide_index(native, oidx, form, chunk=0):
    g = gpu_index(native, oidx)
    g.set_tuning(4, chunk)
    g.set_table_mode(FORMS[form][0])
    return g


def ran_wide(g, form, what=""):
    st = g.get_stats()
    assert st["last_striped"] == FORMS[form][1] and st["last_qg"] == FORMS[form][2] and st["last_scan_lds"] <= 80 * 1024, (what, st)


def same_bits(got, exp, what):
    helpers.assert_same_results(got, exp, what=what)
    assert np.array_equal(got[1][exp[1] < np.inf].view(np.uint32), exp[1][exp[1] < np.inf].view(np.uint32)), what


def random_fixture(d):
    """(oracle index, 61 queries, {(K, w): oracle results}) of the `random` case at width d: built once, left unchanged."""
    if d not in _CACHE:
        oidx, _ = helpers.build_index(3600 + d, 30000, d, 14, M, 256, mode="random")
        _CACHE[d] = (oidx, np.random.default_rng(377 + d).random((61, d), dtype=np.float32), {})
    return _CACHE[d]


def random_expected(d, K, w):
    oidx, qs, res = random_fixture(d)
    if (K, w) not in res:
        res[(K, w)] = oidx.knn_search(qs, K, w)
    return res[(K, w)]


@pytest.mark.parametrize("case", ["random", "permuted_labels", "few_codes", "short_lists", "exact_hits"])
@pytest.mark.parametrize("form", ["q4", "q8"])
def test_wide_pool_kernel(native, form, case):
    """d = 128, 14 lists of ~2 100 points and 61 queries: K = 100 / 65 (one entry in the high half) / 128 (every entry of both halves) / 127,
    one chunk and several per list; permuted labels; lists of four distinct codes (exact ties across whole steps, the K-th key ties); 300
    lists of ~100 points (pools never fill: fewer than K keys handed over, the high half partly or wholly empty); queries that are
    centroid + codewords (table entries of 0).  Then nine queries on the same handle."""
    d = 128
    kc = 300 if case == "short_lists" else 14
    if case == "random":
        oidx, qs, _ = random_fixture(d)
    else:
        oidx, _ = helpers.build_index(3600 + d + len(case), 30000, d, kc, M, 256, label_perm=(case == "permuted_labels"), mode="random",
                                      ndistinct=(4 if case == "few_codes" else None))
        rng = np.random.default_rng(377 + d + len(case))
        qs = rng.random((61, d), dtype=np.float32)
        if case == "exact_hits":
            for i in range(16):
                code = rng.integers(0, 256, M)
                qs[i] = oidx.centroids[i % kc] + np.concatenate([oidx.codebooks[ii, code[ii]] for ii in range(M)])
    for K, w, chunk in ((100, 3, 0), (65, 1, 1024), (128, 5, 4096), (127, 2, 2048)):
        what = "wg8 wide %s %s K=%d w=%d chunk=%d" % (form, case, K, w, chunk)
        exp = random_expected(d, K, w) if case == "random" else oidx.knn_search(qs, K, w)
        g = wide_index(native, oidx, form, chunk)
        got = g.search_raw(qs, K, w)
        ran_wide(g, form, what)
        same_bits(got, exp, what)
        got2 = g.search_raw(qs[:9], K, w)
        ran_wide(g, form, what + ", second call")
        same_bits(got2, tuple(a[:9] for a in exp), what + ", second call")


@pytest.mark.parametrize("form", ["q4", "q8"])
@pytest.mark.parametrize("d", (32, 64, 96))
def test_wide_pool_kernel_other_widths(native, d, form):
    """The `random` case at the narrower sub-spaces (wg8_wide_scan_kernel<NQ, 4 / 8 / 12>), K = 100 and 128."""
    oidx, qs, _ = random_fixture(d)
    for K, w, chunk in ((100, 3, 0), (128, 5, 4096)):
        what = "wg8 wide d=%d %s K=%d w=%d chunk=%d" % (d, form, K, w, chunk)
        g = wide_index(native, oidx, form, chunk)
        got = g.search_raw(qs, K, w)
        ran_wide(g, form, what)
        same_bits(got, random_expected(d, K, w), what)


@pytest.mark.parametrize("form", ["q4", "q8"])
def test_wide_modes_below_the_limit(native, form):
    """K <= 64 under table modes 8 / 9: the narrow kernels of modes 6 / 7 (last_striped 2 / 3) and their bytes."""
    oidx, qs, _ = random_fixture(128)
    for K in (10, 64):
        g = wide_index(native, oidx, form)
        got = g.search_raw(qs, K, 3)
        st = g.get_stats()
        assert st["last_striped"] == FORMS[form][4] and st["last_qg"] == FORMS[form][2], st
        gn = gpu_index(native, oidx)
        gn.set_tuning(4, 0)
        gn.set_table_mode(FORMS[form][3])
        ref = gn.search_raw(qs, K, 3)
        assert gn.get_stats()["last_striped"] == FORMS[form][4]
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), "modes %d and %d at K=%d" % (FORMS[form][0], FORMS[form][3], K)
        same_bits(got, random_expected(128, K, 3), "mode %d K=%d" % (FORMS[form][0], K))


@pytest.mark.parametrize("form", ["q4", "q8"])
def test_wide_modes_beyond_the_limit(native, form):
    """K > 128 under table modes 8 / 9 leaves the eight-wave kernel as mode 6 does above 64: no eight-wave form runs, the oracle's results."""
    oidx, qs, _ = random_fixture(128)
    for K in (129, 200):
        g = wide_index(native, oidx, form)
        got = g.search_raw(qs, K, 3)
        assert g.get_stats()["last_striped"] not in (2, 3, 4, 5), g.get_stats()
        same_bits(got, random_expected(128, K, 3), "mode %d K=%d" % (FORMS[form][0], K))


def test_mode_6_keeps_the_four_wave_kernel_above_64(native):
    """Table mode 6 at K = 100 is what it was: no eight-wave kernel (tests/test_gpu_wg8.py asserts the same next to the narrow kernel)."""
    oidx, qs, _ = random_fixture(128)
    for mode in (6, 7):
        g = gpu_index(native, oidx)
        g.set_tuning(4, 0)
        g.set_table_mode(mode)
        got = g.search_raw(qs, 100, 3)
        assert g.get_stats()["last_striped"] not in (2, 3, 4, 5), g.get_stats()
        same_bits(got, random_expected(128, 100, 3), "mode %d K=100" % mode)


@pytest.mark.parametrize("case", ["zero_codebooks", "huge_scale", "dc_dominates_5000"])
@pytest.mark.parametrize("form", ["q4", "q8"])
def test_wide_pool_kernel_filter_extremes(native, form, case):
    """The cold-start bounds at K = 100 -- the 13th smallest integer sum of a wave's step, the 100th of a crowd's -- where the filter's scale
    does its worst: all-zero tables (every point ties; the scale is not a normal number and the bounds are not taken), entries near the top
    of the float range, sums dominated by the coarse distance.  The bounds may only let MORE points through.  Set up as
    test_eight_wave_kernel_filter_extremes (12 lists of ~3 300 points, chunks of 8192)."""
    d, kc = 128, 12
    oidx, _ = helpers.build_index(1700 + len(case), 40000, d, kc, M, 256, mode="random")
    rng = np.random.default_rng(len(case))
    if case == "zero_codebooks":
        oidx.codebooks[:] = 0
    elif case == "huge_scale":
        oidx.codebooks *= np.float32(1e15)
        oidx.centroids *= np.float32(1e15)
    qs = rng.random((64, d), dtype=np.float32)
    if case == "dc_dominates_5000":
        oidx.centroids += np.float32(5000.0)
        oidx.codebooks *= np.float32(1e-3)
        qs[32:] += np.float32(5000.0)
    elif case == "huge_scale":
        qs *= np.float32(1e15)
    elif case == "zero_codebooks":
        qs[:8] = oidx.centroids[:8]
    for K, w in ((100, 4), (100, 2)):
        what = "wg8 wide filter %s %s K=%d w=%d" % (form, case, K, w)
        g = wide_index(native, oidx, form, 8192)
        got = g.search_raw(qs, K, w)
        ran_wide(g, form, what)
        same_bits(got, oidx.knn_search(qs, K, w), what)


@pytest.mark.parametrize("form", ["q4", "q8"])
def test_fuzz_wide_pool_kernel(native, form):
    """test_fuzz_eight_wave_kernel_other_widths' draws with K from 65 .. 128 and d from all four widths: list counts and sizes from empty
    lists to a few thousand points, chunk sizes that give partial last steps and several chunks per list, w up to kc, batches that leave
    partial groups, permuted labels, few distinct codes, pruning on and off, one push and one delete between searches.  Against the oracle,
    ids exact and distance bits equal.  IVFADC_FUZZ_DRAWS / IVFADC_FUZZ_SEED widen it for soak runs."""
    from oracle import oracle as ora
    rng = np.random.default_rng(int(os.environ.get("IVFADC_FUZZ_SEED", "8086")) + FORMS[form][2])
    for it in range(int(os.environ.get("IVFADC_FUZZ_DRAWS", "12"))):
        d = int(rng.choice(ALL_D))
        kc = int(rng.choice([1, 2, 5, 14, 33, 120]))
        n = int(rng.choice([0, 7, 300, 3000, 20000, 45000]))
        K = int(rng.choice([65, 66, 96, 100, 127, 128]))
        w = int(rng.choice([1, 2, 3, 8, 14, 200]))
        nq = int(rng.choice([1, 4, 5, 37, 130]))
        chunk = int(rng.choice([0, 0, 1024, 2048, 8192]))
        oidx, data = helpers.build_index(7200 + it, n, d, kc, M, 256, label_perm=bool(rng.random() < 0.4),
                                         mode="encode" if (n and n <= 3000 and rng.random() < 0.4) else "random",
                                         ndistinct=(3 if rng.random() < 0.25 else None))
        qs = rng.random((nq, d), dtype=np.float32)
        if n:
            qs[: min(nq, 3)] = data[: min(nq, 3)]
        if rng.random() < 0.2:
            qs += np.float32(20.0)
        g = wide_index(native, oidx, form, chunk)
        if rng.random() < 0.3:
            g.set_pruning(0)
        what = "wg8 wide fuzz %d (%s): d=%d kc=%d n=%d K=%d w=%d nq=%d chunk=%d" % (it, form, d, kc, n, K, w, nq, chunk)
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
def test_list_partitioned_mode_on_the_wide_pool_kernel(native, form):
    """Two parts at K = 100, set up as tests/test_gpu_wg8_partition.py (40 lists of ~750 points, 75 queries, w = 6): the handle plays both
    ranks, each partial search runs the wide form, and ivfadc_merge_partials_device gives the oracle's full scan."""
    import torch
    d, NQ, K, w, nparts = 128, 75, 100, 6, 2
    oidx, _ = helpers.build_index(1940 + d, 30000, d, 40, M, 256, mode="random")
    qs = np.random.default_rng(d + 19).random((NQ, d), dtype=np.float32)
    exp = oidx.knn_search(qs, K, w)
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(qs).to(dev)
    g = wide_index(native, oidx, form)
    what = "list-partitioned wg8 wide %s nparts=%d K=%d w=%d" % (form, nparts, K, w)
    keys_all = torch.zeros((nparts, NQ, K), dtype=torch.int64, device=dev)
    cnts_all = torch.zeros((nparts, NQ), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()       # (torch fills the outputs on ITS stream: finished before the library's stream writes into them)
    for part in range(nparts):
        g.set_list_partition(nparts, part)
        g.search_device_partial(NQ, qd.data_ptr(), K, w, keys_all[part].data_ptr(), cnts_all[part].data_ptr())
        torch.cuda.synchronize()
        ran_wide(g, form, what + " part %d" % part)
        rk, rc, _ = helpers.numpy_partial_keys(oidx, qs[:12], K, w, nparts, part)
        gk = keys_all[part].cpu().numpy().view(np.uint64)[:12]
        gc = cnts_all[part].cpu().numpy()[:12]
        assert np.array_equal(gc, rc) and all(np.array_equal(gk[r, :rc[r]], rk[r, :rc[r]]) for r in range(12)), what + ": partial keys of part %d" % part
    ids = torch.zeros(NQ * K, dtype=torch.int32, device=dev)
    dist = torch.zeros(NQ * K, dtype=torch.float32, device=dev)
    cnt = torch.zeros(NQ, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g.merge_partials_device(NQ, K, nparts, keys_all.data_ptr(), cnts_all.data_ptr(), ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    torch.cuda.synchronize()
    got = (ids.cpu().numpy().view(np.uint32).reshape(NQ, K), dist.cpu().numpy().reshape(NQ, K), cnt.cpu().numpy())
    same_bits(got, exp, what)


@pytest.mark.parametrize("form", ["q4", "q8"])
def test_view_runs_the_wide_pool_kernel(native, form):
    """A view taken after set_table_mode(8 / 9) carries the setting: it runs the wide form and returns the index's bytes."""
    oidx, qs, _ = random_fixture(128)
    g = wide_index(native, oidx, form)
    got = g.search_raw(qs, 100, 3)
    ran_wide(g, form, "the index")
    v = g.clone_view()
    gotv = v.search_raw(qs, 100, 3)
    ran_wide(v, form, "the view")
    assert all(np.array_equal(a, b) for a, b in zip(got, gotv))
    same_bits(gotv, random_expected(128, 100, 3), "view, %s" % form)
