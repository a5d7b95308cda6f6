"""The list-partitioned multi-GPU mode (ivfadc_set_list_partition / ivfadc_search_device_partial / ivfadc_merge_partials_device) through the
eight-wave list-major kernel (csrc/wg8scan.hip.h), rehearsed on ONE GPU: the handle plays every rank in turn, the ranks' partial keys are
stacked as the all-gather would leave them, and the merge must give the oracle's full search -- ids exact, distance bits identical.  The
partition is applied in front of the scan (the top-w kernel counts this rank's lists only, the bucket kernels build work items from that
count) and behind it (the merge): a rank's work items are ordinary ones, and every partial search asserts that the eight-wave kernel ran
them.  Forced as tests/test_gpu_wg8.py forces it: set_tuning(4, 0) + table mode 6 / 7."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

M = 8
FORMS = {"q4": (6, 2, 4), "q8": (7, 3, 8)}      # (table mode, last_striped, queries per code stream)
NQ = 75
_INDEX = {}


def gpu_index(native, oidx):
    return native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)


def fixture_index(variant):
    """(oracle index, queries, {(K, w): oracle results}) of a variant, built once and left unchanged."""
    if variant not in _INDEX:
        d = 96 if variant == "d96" else 128
        oidx, _ = helpers.build_index(940 + d + len(variant), 30000, d, 40, M, 256, mode="random", ndistinct=(4 if variant == "d128_ties" else None))
        qs = np.random.default_rng(d + len(variant)).random((NQ, d), dtype=np.float32)
        _INDEX[variant] = (oidx, qs, {})
    return _INDEX[variant]


def oracle_results(variant, K, w):
    oidx, qs, cache = fixture_index(variant)
    if (K, w) not in cache:
        cache[(K, w)] = oidx.knn_search(qs, K, w)
    return cache[(K, w)]


def ran_eight_wave(g, form, what):
    st = g.get_stats()
    assert st["last_striped"] == FORMS[form][1] and st["last_qg"] == FORMS[form][2] and st["last_scan_lds"] <= 80 * 1024, (what, st)


@pytest.mark.parametrize("variant", ["d128", "d128_ties", "d96"])
@pytest.mark.parametrize("form", ["q4", "q8"])
def test_list_partitioned_mode_on_the_eight_wave_kernel(native, form, variant):
    """40 lists of ~750 points, 75 queries; 2, 3 and 8 parts (eight parts of 16 probes: some ranks hold none of a query's lists -- empty
    partials); K = 10 and 64; four distinct codes (ties across ranks); d = 96 (the partition and the narrower sub-spaces together)."""
    import torch
    oidx, qs, _ = fixture_index(variant)
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(qs).to(dev)
    g = gpu_index(native, oidx)
    g.set_tuning(4, 0)
    g.set_table_mode(FORMS[form][0])
    for nparts, K, w in ((2, 10, 6), (3, 64, 5), (8, 10, 16)):
        what = "list-partitioned wg8 %s %s nparts=%d K=%d w=%d" % (variant, form, nparts, K, w)
        exp = oracle_results(variant, K, w)
        keys_all = torch.zeros((nparts, NQ, K), dtype=torch.int64, device=dev)
        cnts_all = torch.zeros((nparts, NQ), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()       # (torch fills the outputs on ITS stream: finished before the library's stream writes into them)
        for part in range(nparts):
            g.set_list_partition(nparts, part)
            g.search_device_partial(NQ, qd.data_ptr(), K, w, keys_all[part].data_ptr(), cnts_all[part].data_ptr())
            torch.cuda.synchronize()
            ran_eight_wave(g, form, what + " part %d" % part)
            if K == 10:
                rk, rc, _ = helpers.numpy_partial_keys(oidx, qs[:12], K, w, nparts, part)
                gk = keys_all[part].cpu().numpy().view(np.uint64)[:12]
                gc = cnts_all[part].cpu().numpy()[:12]
                assert np.array_equal(gc, rc) and all(np.array_equal(gk[r, :rc[r]], rk[r, :rc[r]]) for r in range(12)), \
                    what + ": partial keys of part %d" % part
        ids = torch.zeros(NQ * K, dtype=torch.int32, device=dev)
        dist = torch.zeros(NQ * K, dtype=torch.float32, device=dev)
        cnt = torch.zeros(NQ, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        g.merge_partials_device(NQ, K, nparts, keys_all.data_ptr(), cnts_all.data_ptr(), ids.data_ptr(), dist.data_ptr(), cnt.data_ptr())
        torch.cuda.synchronize()
        got = (ids.cpu().numpy().view(np.uint32).reshape(NQ, K), dist.cpu().numpy().reshape(NQ, K), cnt.cpu().numpy())
        helpers.assert_same_results(got, exp, what=what)
        assert np.array_equal(got[1][exp[1] < np.inf].view(np.uint32), exp[1][exp[1] < np.inf].view(np.uint32)), what


@pytest.mark.parametrize("form", ["q4", "q8"])
def test_partition_off_again_on_the_eight_wave_kernel(native, form):
    """A handle that played a rank and is switched back (set_list_partition(1, 0)): an ordinary search, the oracle's results, still on the
    eight-wave kernel."""
    import torch
    oidx, qs, _ = fixture_index("d128")
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(qs).to(dev)
    g = gpu_index(native, oidx)
    g.set_tuning(4, 0)
    g.set_table_mode(FORMS[form][0])
    keys = torch.zeros((NQ, 10), dtype=torch.int64, device=dev)
    cnts = torch.zeros(NQ, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g.set_list_partition(3, 1)
    g.search_device_partial(NQ, qd.data_ptr(), 10, 6, keys.data_ptr(), cnts.data_ptr())
    torch.cuda.synchronize()
    ran_eight_wave(g, form, "rank 1 of 3")
    g.set_list_partition(1, 0)
    got = g.search_raw(qs, 10, 6)
    ran_eight_wave(g, form, "partition off")
    helpers.assert_same_results(got, oracle_results("d128", 10, 6), what="wg8 %s, partition off" % form)
