"""GPU parity tests of the eight-wave list-major kernel (csrc/wg8scan.hip.h) at SIXTEEN sub-quantizers: m = 16, d = 128 (PQ16, dsub = 8)
and d = 64 (dsub = 4), wg8_m16_scan_kernel<NQ, DS>, both forms (four and eight queries per code stream).  What is new at m = 16 -- the
16-byte code stream with one point per request, the dword rotation and the lane-dependent address selectors, the two-trip table build and
the quantisation by label, the 11-bit filter fields, four-point candidate passes over rows of sixteen lanes -- changes ids or distance bits
when it is wrong: every comparison is with the CPU oracle, ids exact and distance bits identical (helpers.assert_same_results), and byte
for byte with the same handle's reference-order kernel (table mode 1).  The kernel runs on request only: set_tuning(4, chunk) + table mode
6 / 7, and every search asserts that it ran (last_striped 2 / 3, groups of 4 / 8, two workgroups' worth of LDS) -- on the code before this
kernel an m = 16 index never reached it, so these assertions are what shows the feature."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

M = 16
FORMS = {"q4": (6, 2, 4), "q8": (7, 3, 8)}      # (table mode, last_striped, queries per code stream)
ALL_D = (128, 64)
COMBOS = ((10, 3, 0), (1, 1, 1024), (64, 5, 4096), (17, 2, 2048))     # (K, w, chunk)
_CACHE = {}


def gpu_index(native, oidx):
    return native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)


def m16_index(native, oidx, form, chunk=0):
    g = gpu_index(native, oidx)
    g.set_tuning(4, chunk)
    g.set_table_mode(FORMS[form][0])
    return g


def ran_m16(g, form, what=""):
    st = g.get_stats()
    assert st["last_striped"] == FORMS[form][1] and st["last_qg"] == FORMS[form][2] and st["last_scan_lds"] <= 80 * 1024, (what, st)


def same_bits(got, exp, what):
    helpers.assert_same_results(got, exp, what=what)
    assert np.array_equal(got[1][exp[1] < np.inf].view(np.uint32), exp[1][exp[1] < np.inf].view(np.uint32)), what


def against_mode_1(g, form, got, qs, K, w, what):
    """The same handle under table mode 1 (the reference-order four-wave kernel), byte for byte; the handle goes back to its form."""
    g.set_table_mode(1)
    ref = g.search_raw(qs, K, w)
    assert g.get_stats()["last_striped"] not in (2, 3, 4, 5), what
    g.set_table_mode(FORMS[form][0])
    # (entries behind a query's count are not part of the result: lists shorter than K leave them as each kernel's merge found them)
    assert np.array_equal(got[2], ref[2]), what + ": counts against the reference-order kernel"
    valid = np.arange(K)[None, :] < got[2][:, None]
    assert np.array_equal(got[0][valid], ref[0][valid]) and np.array_equal(got[1][valid].view(np.uint32), ref[1][valid].view(np.uint32)), \
        what + ": against the reference-order kernel"


def fixture(d, case):
    """(oracle index, 61 queries, {(K, w): oracle results}) of a case at width d: built once, left unchanged."""
    if (d, case) not in _CACHE:
        if case == "short_lists":
            oidx, _ = helpers.build_index(4600 + d, 3000, d, 300, M, 256, mode="random")      # ~10 points per list: no pool ever fills at K = 17 / 64
        else:
            oidx, _ = helpers.build_index(4600 + d + len(case), 30000, d, 14, M, 256, label_perm=(case == "permuted_labels"), mode="random",
                                          ndistinct=(4 if case == "few_codes" else None))
        qs = np.random.default_rng(477 + d + len(case)).random((61, d), dtype=np.float32)
        _CACHE[(d, case)] = (oidx, qs, {})
    return _CACHE[(d, case)]


def expected(d, case, K, w):
    oidx, qs, res = fixture(d, case)
    if (K, w) not in res:
        res[(K, w)] = oidx.knn_search(qs, K, w)
    return res[(K, w)]


@pytest.mark.parametrize("case", ["random", "permuted_labels", "few_codes", "short_lists"])
@pytest.mark.parametrize("form", ["q4", "q8"])
@pytest.mark.parametrize("d", ALL_D)
def test_m16_kernel(native, d, form, case):
    """14 lists of ~2 100 points and 61 queries (odd: groups that do not fill): one chunk and several per list, K = 1 / 10 / 17 / 64;
    permuted labels; lists of four distinct codes (duplicates within and across lists: the visit order decides); 300 lists of ~10 points
    (pools that never fill, idle waves, empty lists).  Then nine queries on the same handle."""
    oidx, qs, _ = fixture(d, case)
    for K, w, chunk in COMBOS:
        what = "wg8 m16 d=%d %s %s K=%d w=%d chunk=%d" % (d, form, case, K, w, chunk)
        exp = expected(d, case, K, w)
        g = m16_index(native, oidx, form, chunk)
        got = g.search_raw(qs, K, w)
        ran_m16(g, form, what)
        same_bits(got, exp, what)
        got2 = g.search_raw(qs[:9], K, w)
        ran_m16(g, form, what + ", second call")
        same_bits(got2, tuple(a[:9] for a in exp), what + ", second call")
        against_mode_1(g, form, got, qs, K, w, what)


@pytest.mark.parametrize("form", ["q4", "q8"])
@pytest.mark.parametrize("d", ALL_D)
def test_m16_kernel_pruning_off(native, d, form):
    oidx, qs, _ = fixture(d, "random")
    g = m16_index(native, oidx, form, 1024)
    g.set_pruning(0)
    got = g.search_raw(qs, 10, 3)
    ran_m16(g, form, "pruning off")
    same_bits(got, expected(d, "random", 10, 3), "wg8 m16 d=%d %s pruning off" % (d, form))


@pytest.mark.parametrize("case", ["outlier_codewords", "zero_codebooks", "tiny_scale", "huge_scale", "dc_dominates_5000"])
@pytest.mark.parametrize("form", ["q4", "q8"])
@pytest.mark.parametrize("d", ALL_D)
def test_m16_kernel_filter_extremes(native, d, form, case):
    """The 11-bit fields and the sixteen-term budget on the inputs of test_eight_wave_kernel_filter_extremes: one far codeword per
    sub-quantizer that flattens every other entry to 0, all-zero tables (every point ties; the scale is not a normal number), entries in
    the denormal range and near the top of the float range, sums dominated by the coarse distance -- the filter and the bounds taken from
    the integer sums may only let MORE points through.  Twelve lists of ~1 700 points: two steps per wave, the cold-start exchange runs."""
    kc = 12
    oidx, _ = helpers.build_index(1600 + d + len(case), 20000, d, kc, M, 256, mode="random")
    rng = np.random.default_rng(d + len(case))
    if case == "outlier_codewords":
        oidx.codebooks[:, 7, :] *= np.float32(1000.0)
    elif case == "zero_codebooks":
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
        what = "wg8 m16 filter d=%d %s %s K=%d" % (d, form, case, K)
        g = m16_index(native, oidx, form, 8192)
        got = g.search_raw(qs, K, w)
        ran_m16(g, form, what)
        same_bits(got, oidx.knn_search(qs, K, w), what)


@pytest.mark.parametrize("form", ["q4", "q8"])
@pytest.mark.parametrize("d", ALL_D)
def test_m16_kernel_push_and_delete_between_searches(native, d, form):
    from oracle import oracle as ora
    oidx, qs, _ = fixture(d, "random")
    g = m16_index(native, oidx, form, 2048)
    same_bits(g.search_raw(qs, 10, 3), expected(d, "random", 10, 3), "before edits")
    ran_m16(g, form, "before edits")
    rng = np.random.default_rng(d)
    n = oidx.ids.shape[0]
    g._append(rng.random((200, d), dtype=np.float32), np.arange(n, n + 200, dtype=np.uint32))
    g._delete_ids(rng.integers(0, n + 200, 60).astype(np.uint32))
    offsets, codes, ids = g._lists()
    o2 = ora.OracleIndex(oidx.centroids, oidx.codebooks, oidx.labels, offsets, codes, ids)
    got = g.search_raw(qs, 10, 3)
    ran_m16(g, form, "after edits")
    same_bits(got, o2.knn_search(qs, 10, 3), "wg8 m16 d=%d %s after a push and a delete" % (d, form))


@pytest.mark.parametrize("form", ["q4", "q8"])
def test_view_runs_the_m16_kernel(native, form):
    """A view taken after set_table_mode(6 / 7) carries the setting: it runs the kernel and returns the index's bytes."""
    oidx, qs, _ = fixture(128, "random")
    g = m16_index(native, oidx, form)
    got = g.search_raw(qs, 10, 3)
    ran_m16(g, form, "the index")
    v = g.clone_view()
    gotv = v.search_raw(qs, 10, 3)
    ran_m16(v, form, "the view")
    assert all(np.array_equal(a, b) for a, b in zip(got, gotv))
    same_bits(gotv, expected(128, "random", 10, 3), "view, %s" % form)


@pytest.mark.parametrize("form", ["q4", "q8"])
@pytest.mark.parametrize("d", ALL_D)
def test_list_partitioned_mode_on_the_m16_kernel(native, d, form):
    """Two parts, set up as tests/test_gpu_wg8_partition.py: the handle plays both ranks, each partial search runs the kernel, and
    ivfadc_merge_partials_device gives the unpartitioned answer -- the oracle's full scan."""
    import torch
    oidx, qs, _ = fixture(d, "random")
    NQ, K, w, nparts = qs.shape[0], 10, 5, 2
    exp = expected(d, "random", K, w)
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(qs).to(dev)
    g = m16_index(native, oidx, form)
    what = "list-partitioned wg8 m16 d=%d %s" % (d, form)
    keys_all = torch.zeros((nparts, NQ, K), dtype=torch.int64, device=dev)
    cnts_all = torch.zeros((nparts, NQ), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()       # (torch fills the outputs on ITS stream: finished before the library's stream writes into them)
    for part in range(nparts):
        g.set_list_partition(nparts, part)
        g.search_device_partial(NQ, qd.data_ptr(), K, w, keys_all[part].data_ptr(), cnts_all[part].data_ptr())
        torch.cuda.synchronize()
        ran_m16(g, form, what + " part %d" % part)
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
    g.set_list_partition(1, 0)
    full = g.search_raw(qs, K, w)
    ran_m16(g, form, what + ", partition off")
    assert all(np.array_equal(a, b) for a, b in zip(got, full)), what + ": merged parts against the unpartitioned search"


@pytest.mark.parametrize("mode", [6, 8])
def test_m16_above_64_leaves_the_kernel(native, mode):
    """K = 100 at m = 16: neither table mode 6 nor 8 (the wide pool is m = 8 only) takes an eight-wave kernel; the oracle's bytes."""
    oidx, qs, _ = fixture(128, "random")
    g = gpu_index(native, oidx)
    g.set_tuning(4, 0)
    g.set_table_mode(mode)
    got = g.search_raw(qs, 100, 3)
    assert g.get_stats()["last_striped"] not in (2, 3, 4, 5), g.get_stats()
    same_bits(got, expected(128, "random", 100, 3), "m16 mode %d K=100" % mode)


@pytest.mark.parametrize("d", ALL_D)
def test_m16_default_plan_is_unchanged(native, d):
    """No table mode: an m = 16 index keeps the kernels it had (admission to the default plan waits for a measured win)."""
    oidx, qs, _ = fixture(d, "random")
    g = gpu_index(native, oidx)
    g.set_tuning(4, 0)
    got = g.search_raw(qs, 10, 3)
    assert g.get_stats()["last_striped"] not in (2, 3, 4, 5), g.get_stats()
    same_bits(got, expected(d, "random", 10, 3), "m16 default plan d=%d" % d)
