"""The four-wave kernels at the shapes where neighbouring LDS regions touch (csrc/scan_layouts.h: FwLds, FwTail, SqLds).

tests/test_scan_lds.py proves on the CPU that the layout's regions are disjoint; here the kernels that carve by it run on the smallest
shapes at which a region misplaced by one step would be written by its neighbour: the exchange area exactly as large as the tables
(m = 1), LDS selectors between residuals and counters with the filter table in front and the parking buffers last (m = 8, K = 65),
five-dword parked entries (m = 16), the short-row scratch behind five 32-entry probe arrays (w = 24) and three 64-entry arrays filling the
probe area (w = 32 | 33, 64), sq_kernel's row of coarse distances ending with the allocation (kc = 2048) and off the 16-byte grid
(kc = 2045), the masked kernel on LDS selectors, and the matrix-core rounds' tail behind LbCfg::END.  Lists hold a handful of distinct
codes, so exact ties crowd the parking buffers and the selectors.  Every case compares counts, ids and distance bits with the C oracle
(helpers.assert_same_results) and asserts that the planned LDS bytes are the figure of the frozen Python models (tests/sequences.py,
tests/masked.py; the LB and small-batch sums are restated below as they stood before the layout was written down once).

Already covered bit for bit elsewhere, and not repeated: m = 8 / m = 16 groups of four on LDS selectors at K = 100 / K = 65 after every
other form (tests/test_gpu_sequences.py: "four-wave LDS selectors K=100", "K=65 under mode 8 leaves the kernel")."""
import functools

import numpy as np
import pytest

import helpers
import masked as mk
import sequences as sq
from oracle import oracle as ora

pytestmark = pytest.mark.gpu

NQ = 64


@functools.lru_cache(maxsize=None)
def _index(m, dsub, kc, n, seed):
    oidx, data = helpers.build_index(seed, n, m * dsub, kc, m, mode="random", ndistinct=5)
    rng = np.random.default_rng(seed + 7)
    qs = np.ascontiguousarray(data[rng.choice(n, NQ, replace=False)] + rng.normal(0, 0.01, (NQ, m * dsub)).astype(np.float32))
    qs.setflags(write=False)
    return oidx, qs


@functools.lru_cache(maxsize=None)
def _expected(m, dsub, kc, n, seed, K, w, nq=NQ):
    oidx, qs = _index(m, dsub, kc, n, seed)
    return oidx.knn_search(qs[:nq], K, w, nthreads=ora.max_threads())


def _gpu(native, oidx):
    return native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)


def _list_major_lds(m, dsub, K):
    return sq.scan_lds_bytes(m, dsub, 256, 4, sq.cap_of(K), K <= 64, True, True)


def _query_major_lds(m, dsub, K):
    """the plan takes one or two probes per round (prune_est); either way the figure is the model's"""
    return {sq.scan_lds_bytes(m, dsub, 256, pg, sq.cap_of(K), K <= 64, False, True) for pg in (1, 2)}


# (m, dsub, kc, n, seed): lists of ~250 points made of five distinct codes
M1 = (1, 4, 8, 2000, 11)
M8 = (8, 16, 8, 3000, 12)
M16 = (16, 8, 8, 3000, 13)


@pytest.mark.parametrize("K", [10, 65])
@pytest.mark.parametrize("major", ["query", "list"])
def test_one_sub_quantizer_exchange_area_as_large_as_the_tables(native, major, K):
    oidx, qs = _index(*M1)
    g = _gpu(native, oidx)
    g.set_tuning(-1 if major == "query" else 4, 0)
    got = g.search_raw(qs, K, 4)
    st = g.get_stats()
    helpers.assert_same_results(got, _expected(*M1, K, 4), what="m=1 %s-major K=%d" % (major, K))
    if major == "query":
        assert st["last_qg"] == 0 and st["last_scan_lds"] in _query_major_lds(1, 4, K), st
    else:
        assert st["last_qg"] == 4 and st["last_striped"] == 0 and st["last_scan_lds"] == _list_major_lds(1, 4, K), st


@pytest.mark.parametrize("shape,K", [(M8, 10), (M8, 65), (M16, 10), (M16, 100)])
def test_striped_groups_of_four_parking_buffers_last(native, shape, K):
    m, dsub = shape[0], shape[1]
    oidx, qs = _index(*shape)
    g = _gpu(native, oidx)
    g.set_tuning(4, 0)
    got = g.search_raw(qs, K, 4)
    st = g.get_stats()
    helpers.assert_same_results(got, _expected(*shape, K, 4), what="m=%d striped K=%d" % (m, K))
    assert st["last_qg"] == 4 and st["last_striped"] == 1 and st["last_nf"] == 0 and st["last_scan_lds"] == _list_major_lds(m, dsub, K), st


FUSED = (8, 16, 64, 4000, 14)


@pytest.mark.parametrize("w", [24, 32, 33, 64])
def test_fused_top_w_probe_arrays_and_short_row_scratch(native, w):
    oidx, qs = _index(*FUSED)
    g = _gpu(native, oidx)
    g.set_tuning(-1, 0)
    got = g.search_raw(qs, 10, w)
    st = g.get_stats()
    helpers.assert_same_results(got, _expected(*FUSED, 10, w), what="fused top-w, w=%d" % w)
    assert st["last_qg"] == 0 and st["last_scan_lds"] in _query_major_lds(8, 16, 10), st


@pytest.mark.parametrize("kc", [2048, 2045])
@pytest.mark.parametrize("m,dsub", [(2, 4), (8, 16)])
def test_small_batch_kernel_row_of_coarse_distances(native, m, dsub, kc):
    shape = (m, dsub, kc, 4000, 15)
    oidx, qs = _index(*shape)
    g = _gpu(native, oidx)
    g.set_coarse_mode(5)     # the coarse search inside the launch: the row lies in LDS behind the selection's scratch
    got = g.search_raw(qs[:1], 10, 8)
    st = g.get_stats()
    helpers.assert_same_results(got, _expected(*shape, 10, 8, 1), what="sq_kernel m=%d kc=%d" % (m, kc))
    # (the sum as ivfadc_hip.hip spelled it: the carve of one query, 64 bytes of scratch and alignment, the row)
    assert st["last_qg"] == -3 and st["last_scan_lds"] == sq.scan_lds_bytes(m, dsub, 256, 1, 64, True, False, True) + 64 + kc * 4, st


def test_masked_groups_of_four_on_lds_selectors(native):
    m, dsub, kc, n, seed = M8
    oidx, qs = _index(*M8)
    keep = np.random.default_rng(16).random(n) < 0.7          # by stored id
    sel = keep[oidx.ids]
    lens = np.diff(oidx.offsets)
    lst = np.repeat(np.arange(kc), lens)
    off = np.zeros(kc + 1, np.int64)
    np.cumsum(np.bincount(lst[sel], minlength=kc), out=off[1:])
    # the kept points alone, in their lists' order: the same sums, the same order among ties
    sub = ora.OracleIndex(oidx.centroids, oidx.codebooks, oidx.labels, off, np.ascontiguousarray(oidx.codes[sel]), np.ascontiguousarray(oidx.ids[sel]))
    exp = sub.knn_search(qs, 65, 4, nthreads=ora.max_threads())
    g = _gpu(native, oidx)
    g.set_tuning(4, 0)
    ms = g.maskset(masks=[keep])
    got = g.search_masked_raw(qs, 65, ms, None, 4)
    st = g.get_stats()
    helpers.assert_same_results(got, exp, what="masked qg=4 K=65")
    assert st["last_qg"] == 4 and st["last_scan_lds"] == mk.scan_lds_bytes(m, m * dsub, 4, 65), st


def _lb_lds_bytes(m, dsub, pg):
    """lb_lds_bytes as scan_layouts.h spelled it before it became LbCfg::END + the four-wave tail"""
    b = (pg * (m * 256 + 32) + 15) // 16 * 16
    b += m * pg * ((dsub + 3) & ~3) * 4
    b += 2 * m * pg * 4 + 128 + 256
    b += m * dsub * 4
    b += 4 * (54 if pg >= 4 else 16) * (m // 4 + 2) * 4
    b += 4 * 64 * 8
    b += 4 * pg * 4 + 16 + pg * 40 + 3 * 256
    return b


def test_matrix_core_rounds_tail_behind_their_own_regions(native):
    shape = (16, 6, 64, 4000, 17)
    oidx, qs = _index(*shape)
    g = _gpu(native, oidx)
    g.set_tuning(-1, 0)
    g.set_table_mode(2)      # the rounds on request at m = 16: four probes per round from w = 3 on
    got = g.search_raw(qs, 10, 32)
    st = g.get_stats()
    helpers.assert_same_results(got, _expected(*shape, 10, 32), what="LB rounds m=16 dsub=6 w=32")
    assert st["last_qg"] == 0 and st["last_lb"] == 1 and st["last_scan_lds"] == _lb_lds_bytes(16, 6, 4), st
