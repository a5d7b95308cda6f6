"""ivfadc_score_ids on the GPU: ids, found flags and Float32 bit patterns against the search itself and against the numpy model of
tests/score_ref.py (the CPU side is tests/test_score_model.py: the model is the oracle's search, and the case table tells it from twelve
wrong implementations).

Small indexes (a few hundred points) of the shapes the kernel has paths for -- d / m / dsub = 32 / 8 / 4, 10 / 2 / 5 (40-byte rows: no
16-byte loads), 6 / 1 / 6, 96 / 16 / 6, 128 / 8 / 16, 768 / 48 / 16 at kc = 4; ksub = 2 and 256 with permuted labels; UInt16 handles with
ksub = 300; code strides 8 and 4 -- on rounding-hostile quantizers and queries (graded sub-space magnitudes, dc-dominated sums, exact hits).
Edges: C = 1 / 63 / 64 / 65 / 257, nq = 1 / 3, absent ids, repeated ids and 0xFFFFFFFF, ragged counts with a zero, the shared row against
the same ids given per query, stale rows after a delete, an in-place append, a plain view, a subset view, an :opq file, synthetic lists, the
device entry on torch tensors, a workspace limit that forces several slices, two threads on one handle, the refusals, knn_among."""
import os
import threading

import numpy as np
import pytest

import helpers
import list_end as le
import reconstruct_ref as rr
import score_ref as sr
import write_path as wp
from oracle import oracle as ora
from test_reconstruct_model import stale_case

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def handle_of(native, case):
    off, codes, ids = case.st.arrays()
    return native.IVFADCIndex.from_arrays(case.qz.centroids, case.qz.codebooks, case.qz.labels, off, codes, ids)


def check(g, st, qz, qs, ids, counts, what):
    """score_raw on handle g against the model over (st, qz): found flags and distance bits identical."""
    got = g.score_raw(qs, ids, counts)
    nq, ncand = len(qs), np.shape(ids)[-1]
    assert got[0].dtype == np.float32 and got[0].shape == (nq, ncand) and got[1].dtype == bool and got[1].shape == (nq, ncand)
    diff = sr.first_difference(got, sr.score(st, qz, qs, ids, counts), ids)
    assert diff is None, "%s: %s" % (what, diff)
    return got


@pytest.mark.parametrize("name", sorted(sr.case_table()))
def test_against_the_search(native, name):
    """search_raw(K = n, w = kc) yields (id, distance) for every stored entry; score_raw of those ids, shuffled, returns the same bits"""
    case = sr.case_table()[name]
    g = handle_of(native, case)
    n = len(case.stored_ids())
    qs = case.queries
    s_ids, s_dists, s_counts = g.search_raw(qs, n, case.qz.kc)
    assert (s_counts == n).all()
    rng = np.random.default_rng(12)
    rows = np.stack([rng.permutation(s_ids[q]) for q in range(len(qs))]).astype(np.uint32)
    dists, found = g.score_raw(qs, rows)
    assert found.all()
    uniq, cnt = np.unique(case.stored_ids(), return_counts=True)
    repeated = uniq[cnt > 1]
    for q in range(len(qs)):
        order = np.argsort(s_ids[q], kind="stable")
        at = order[np.searchsorted(s_ids[q][order], rows[q])]                     # the (first) search slot of every scored id
        once = ~np.isin(rows[q], repeated)
        gb, eb = dists[q].view(np.uint32), s_dists[q][at].view(np.uint32)
        bad = np.nonzero((gb != eb) & once)[0]
        assert bad.size == 0, "%s, query %d, id %d: scored %s, the search reports %s (%d of %d ids differ)" % (
            name, q, rows[q, bad[0]], float(dists[q, bad[0]]).hex(), float(s_dists[q][at][bad[0]]).hex(), bad.size, n)
        for j in np.nonzero(~once)[0]:                                             # a repeated id: the distance of one of its entries
            assert (s_dists[q][s_ids[q] == rows[q, j]].view(np.uint32) == gb[j]).any()
    # and the model says which entry: every bit, repeated ids included
    check(g, case.st, case.qz, qs, rows, None, name + ", every stored id")


@pytest.mark.parametrize("name", sorted(sr.case_table()))
def test_edges_against_the_model(native, name):
    case = sr.case_table()[name]
    g = handle_of(native, case)
    for ncand in sr.EDGE_C:
        for nq in (1, 3):
            check(g, case.st, case.qz, case.queries[:nq], case.rows(ncand, nq=nq), None, "%s, C = %d, nq = %d" % (name, ncand, nq))
    rows = case.rows(65)
    assert 0xFFFFFFFF in rows
    counts = case.ragged_counts(65)
    got = check(g, case.st, case.qz, case.queries, rows, counts, name + ", ragged counts")
    dead = np.arange(65)[None, :] >= counts[:, None]
    assert (counts == 0).any() and (got[0][dead].view(np.uint32) == sr.INF_BITS).all() and not got[1][dead].any()
    absent = ~got[1] & ~dead
    assert absent.any() and (got[0][absent].view(np.uint32) == sr.INF_BITS).all()
    # the shared row against the same ids given per query, with and without counts
    row = case.rows(65, seed=1, nq=1)[0]
    for cnt in (None, counts):
        shared = check(g, case.st, case.qz, case.queries, row, cnt, name + ", shared row")
        tiled = g.score_raw(case.queries, np.tile(row, (len(case.queries), 1)), cnt)
        assert sr.same_answer(shared, tiled), name + ": the shared row and the same ids per query differ"
    # nothing to score
    assert g.score_raw(case.queries[:0], np.zeros((0, 5), np.uint32))[0].shape == (0, 5)
    assert g.score_raw(case.queries, np.zeros((len(case.queries), 0), np.uint32))[0].shape == (len(case.queries), 0)


def test_python_entries(native):
    case = sr.case_table()["d32_m8"]
    g = handle_of(native, case)
    rows = case.rows(65)
    exp_d, exp_f = sr.score(case.st, case.qz, case.queries, rows)
    assert rr.same_bits(native.score(g, case.queries, rows), exp_d)
    one = native.score(g, case.queries[2], rows[2])
    assert one.shape == (65,) and rr.same_bits(one, exp_d[2])
    assert rr.same_bits(native.score(g, [q for q in case.queries], rows[0]), sr.score(case.st, case.qz, case.queries, rows[0])[0])
    # knn_among against a host sort of score: (distance, position in the row), absent ids dropped
    for k in (1, 10, 65):
        got_i, got_d = native.knn_among(g, case.queries, rows, k)
        for q in range(len(case.queries)):
            order = sorted(np.nonzero(exp_f[q])[0], key=lambda j: (float(exp_d[q, j]), j))[:k]
            assert got_i[q].tolist() == rows[q][order].tolist() and rr.same_bits(got_d[q], exp_d[q][order]), (k, q)
    got_i, got_d = native.knn_among(g, case.queries[1], rows[1], 5)
    assert got_i.shape == (5,) and (np.diff(got_d) >= 0).all()
    # merged with search results: the scored distance of a search's own results is the search's
    s_ids, s_dists, s_counts = g.search_raw(case.queries, 10, 3)
    assert (s_counts == 10).all() and rr.same_bits(g.score_raw(case.queries, s_ids)[0], s_dists)


@pytest.mark.parametrize("kind", ("m8_d32", "u16"))
def test_stale_rows_after_a_delete(native, kind):
    """the decoys of list_end.hostile_case are deleted in place: their rows and ids stay behind list_len and are no entries"""
    hc = le.hostile_case(kind)
    g = wp.gpu_handle(native, hc.ref)
    g.search_raw(hc.qs[-1:], 1, 1)                             # the device layout is current: the delete below edits it in place
    assert g._delete_ids(le.all_decoy_ids(hc)) == len(le.all_decoy_ids(hc))
    case, only_stale = stale_case(kind)
    assert len(only_stale) >= 16
    qs = np.ascontiguousarray(hc.qs[:3], np.float32)
    dists, found = g.score_raw(qs, only_stale[:64])
    assert not found.any() and (dists.view(np.uint32) == sr.INF_BITS).all(), "an id behind list_len was scored as an entry"
    live = case.stored_ids()
    ids = np.random.default_rng(3).permutation(np.concatenate([live[::40], only_stale[:40]])).astype(np.uint32)
    check(g, case.st, case.qz, qs, ids, None, "stale rows, " + kind)
    check(g, case.st, case.qz, qs, np.tile(ids[:65], (3, 1)), np.array([65, 0, 17], np.int32), "stale rows, per query, " + kind)


def test_after_an_in_place_append_and_a_shift(native):
    case = sr.case_table()["d32_m8"]
    qz = case.qz
    g = handle_of(native, case)
    g.search_raw(qz.centroids[:1], 1, 1)                       # layout current: capacity len + max(32, len / 8) per list
    n = len(g)
    rng = np.random.default_rng(9)
    pts = (qz.centroids[rng.integers(0, qz.kc, 20)] + np.float32(0.01) * rng.standard_normal((20, qz.d)).astype(np.float32)).astype(np.float32)
    before = g.get_stats()["inplace_appends"]
    g._append(pts, np.arange(n, n + 20, dtype=np.uint32))
    assert g.get_stats()["inplace_appends"] == before + 1, "20 points over 7 lists fit the spare room"
    st = rr.Stored.from_lists(*g._lists())
    ids = np.concatenate([np.arange(n - 5, n + 25), case.rows(65, nq=1)[0]]).astype(np.uint32)
    got = check(g, st, qz, case.queries, ids, None, "after an in-place append")
    assert got[1][:, 5:25].all() and not got[1][:, 25:30].any()
    # an append that overflows a list: the mirror is ahead of the device copy until the entry lays the lists out again
    big = int(np.argmax(st.len))
    room = int(wp.capacity(np.array(st.len))[big]) - st.len[big]
    g._append(np.repeat(qz.centroids[big:big + 1], room + 50, 0), np.arange(n + 20, n + 70 + room, dtype=np.uint32))
    st = rr.Stored.from_lists(*g._lists())
    check(g, st, qz, case.queries, np.arange(n, n + 70 + room, dtype=np.uint32)[::3], None, "after an overflowing append")
    g._shift_ids(1)
    st = rr.Stored.from_lists(*g._lists())
    check(g, st, qz, case.queries[:2], np.array([0, 1, n + 70 + room, n + 69 + room], np.uint32), None, "after a shift")


def test_views_and_refusals(native):
    from ivfadc_jl_amd import _native as nat
    case = sr.case_table()["d96_m16"]
    g = handle_of(native, case)
    qs = case.queries
    rows = case.rows(65)
    v = g.clone_view()
    check(v, case.st, case.qz, qs, rows, case.ragged_counts(65), "plain view")
    stored = case.stored_ids()
    keep = np.sort(stored)[::3]
    s = g.subset(ids=keep)
    dropped = np.setdiff1d(stored, keep)
    ids = np.random.default_rng(4).permutation(np.concatenate([keep[:150], dropped[:60]])).astype(np.uint32)
    on_view, on_index = s.score_raw(qs, ids), g.score_raw(qs, ids)
    was_dropped = np.isin(ids, dropped)
    assert not on_view[1][:, was_dropped].any() and (on_view[0][:, was_dropped].view(np.uint32) == sr.INF_BITS).all(), "a dropped id is absent"
    assert on_view[1][:, ~was_dropped].all() and rr.same_bits(on_view[0][:, ~was_dropped], on_index[0][:, ~was_dropped]), \
        "a kept id has the bits it has on the index"
    assert on_index[1].all()
    # the refusals, as ivfadc_locate refuses them: a list partition, a stale view
    g.set_list_partition(2, 0)
    with pytest.raises(nat.IVFADCError) as e:
        g.score_raw(qs, rows)
    assert e.value.code == nat.ERR_STATE and "list-partitioned" in str(e.value)
    g.set_list_partition(1, 0)
    check(g, case.st, case.qz, qs, rows, None, "after the partition is switched off")
    g._delete_ids(stored[:1])
    for stale in (v, s):
        with pytest.raises(nat.IVFADCError) as e:
            stale.score_raw(qs, rows)
        assert e.value.code == nat.ERR_STATE
    # a handle that was never given lists: whatever ivfadc_locate says of it, ivfadc_score_ids says too
    bare = native.IVFADCIndex.from_arrays(case.qz.centroids, case.qz.codebooks, case.qz.labels)
    try:
        located = bare.locate_raw(rows[0])
    except nat.IVFADCError as err:
        assert err.code == nat.ERR_STATE
        with pytest.raises(nat.IVFADCError) as e:
            bare.score_raw(qs, rows)
        assert e.value.code == nat.ERR_STATE and "no inverted lists" in str(e.value)
    else:
        assert (located[0] == -1).all()
        dists, found = bare.score_raw(qs, rows)
        assert not found.any() and (dists.view(np.uint32) == sr.INF_BITS).all()


def test_device_synthesised_lists(native):
    """no host mirror and no id array: the id is the position; the oracle regenerates the codes from the seed"""
    cent, cbs, labels = helpers.make_quantizers(6200, 24, len(rr.CASE_LENS), 8, 256)
    offsets = np.zeros(len(rr.CASE_LENS) + 1, np.int64)
    np.cumsum(rr.CASE_LENS, out=offsets[1:])
    n = int(offsets[-1])
    g = native.IVFADCIndex.from_arrays(cent, cbs, labels)
    g.synth_lists(offsets, 4242)
    qz = rr.Quantizers(cent, cbs, labels)
    st = rr.Stored.from_lists(offsets, ora.synth_fill(4242, 0, n, 8), np.arange(n, dtype=np.uint32))
    rng = np.random.default_rng(5)
    qs = rng.random((3, 24), dtype=np.float32)
    check(g, st, qz, qs, rng.permutation(n).astype(np.uint32), None, "synthetic, every id")
    check(g, st, qz, qs, np.array([[n, 0, n - 1, 0xFFFFFFFF, 5, 5]] * 3, np.uint32), None, "synthetic, absent and repeated")
    s_ids, s_dists, _ = g.search_raw(qs, 20, 4)
    assert rr.same_bits(g.score_raw(qs, s_ids)[0], s_dists)


def test_opq_loaded_golden_file(native):
    """the scan does not apply the rotation, so neither does ivfadc_score_ids"""
    idx = native.load_ivfadc_index(os.path.join(GOLDEN, "persistency_hand_f32_u16_opq.bin"))
    assert idx.rotated
    st = rr.Stored.from_lists(*idx._lists())
    qz = rr.Quantizers(idx._centroids, idx._codebooks, idx._labels)
    stored = np.concatenate([st.ids[l] for l in range(len(st.len))]).astype(np.uint32)
    qs = np.random.default_rng(6).random((3, qz.d), dtype=np.float32)
    check(idx, st, qz, qs, np.concatenate([stored, stored[::-1], [len(stored) + 3]]).astype(np.uint32), None, ":opq file")
    s_ids, s_dists, s_counts = idx.search_raw(qs, len(stored), qz.kc)
    assert (s_counts == len(stored)).all() and rr.same_bits(idx.score_raw(qs, s_ids)[0], s_dists)


def test_device_entry_on_torch_tensors(native):
    """ids that a search left in device memory are scored in device memory; nothing is synchronised before ivfadc_sync"""
    import torch
    case = sr.case_table()["d128_m8"]
    qz = case.qz
    g = handle_of(native, case)
    dev = "cuda:0"
    nq, K = 6, 10
    qs = case.queries
    dq = torch.from_numpy(qs).to(dev)
    di = torch.zeros((nq, K), dtype=torch.int32, device=dev)
    dd = torch.zeros((nq, K), dtype=torch.float32, device=dev)
    dc = torch.zeros(nq, dtype=torch.int32, device=dev)
    out = torch.full((nq, K), 7.0, dtype=torch.float32, device=dev)
    fnd = torch.full((nq, K), 7, dtype=torch.uint8, device=dev)
    rows = case.rows(65)
    drow = torch.from_numpy(rows.view(np.int32)).to(dev)
    cnts = np.array([65, 0, -4, 99, 17, 64], np.int32)                            # the device entry clamps
    dcnt = torch.from_numpy(cnts).to(dev)
    out2 = torch.full((nq, 65), 7.0, dtype=torch.float32, device=dev)
    fnd2 = torch.full((nq, 65), 7, dtype=torch.uint8, device=dev)
    out3 = torch.full((nq, 65), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    g.search_device(nq, dq.data_ptr(), K, 4, di.data_ptr(), dd.data_ptr(), dc.data_ptr())
    g.score_device(nq, dq.data_ptr(), K, K, di.data_ptr(), None, out.data_ptr(), fnd.data_ptr())
    g.score_device(nq, dq.data_ptr(), 65, 65, drow.data_ptr(), dcnt.data_ptr(), out2.data_ptr(), fnd2.data_ptr())
    g.score_device(nq, dq.data_ptr(), 65, 0, drow[3].data_ptr(), None, out3.data_ptr(), None)       # one shared row, no found array
    g.sync()
    assert (dc.cpu().numpy() == K).all() and fnd.cpu().numpy().all()
    assert rr.same_bits(out.cpu().numpy(), dd.cpu().numpy()), "the scored distance of a search's results is the search's"
    exp = sr.score(case.st, qz, qs, rows, np.clip(cnts, 0, 65))
    diff = sr.first_difference((out2.cpu().numpy(), fnd2.cpu().numpy().astype(bool)), exp, rows)
    assert diff is None, "device entry, clamped counts: " + diff
    assert rr.same_bits(out3.cpu().numpy(), sr.score(case.st, qz, qs, rows[3])[0])
    # the host entry on the same ids gives the same bytes
    assert sr.same_answer(g.score_raw(qs, rows, np.clip(cnts, 0, 65)), exp)


def test_workspace_limit_forces_several_slices(native):
    """1 MiB of workspace (the smallest limit) holds the locate of 127 queries of 257 slots: 300 queries are three slices"""
    case = sr.case_table()["d10_m2"]
    g = handle_of(native, case)
    nq, ncand = 300, 257
    rng = np.random.default_rng(21)
    qs = np.ascontiguousarray(case.queries[rng.integers(0, len(case.queries), nq)] + rng.random((nq, 10), dtype=np.float32))
    rows = case.rows(ncand, nq=nq)
    counts = case.ragged_counts(ncand, nq=nq)
    whole = g.score_raw(qs, rows, counts)
    g.set_workspace_limit(1)
    sliced = g.score_raw(qs, rows, counts)
    shared = g.score_raw(qs, rows[7])
    g.set_workspace_limit(8 << 30)
    assert sr.same_answer(whole, sliced), "the slices change nothing"
    assert sr.same_answer(shared, g.score_raw(qs, rows[7]))
    pick = np.array([0, 126, 127, 128, 253, 254, 255, 299])                        # both sides of every cut
    diff = sr.first_difference((sliced[0][pick], sliced[1][pick]), sr.score(case.st, case.qz, qs[pick], rows[pick], counts[pick]), rows[pick])
    assert diff is None, diff


def test_two_threads_on_one_handle(native):
    case = sr.case_table()["u16"]
    g = handle_of(native, case)
    rows = [case.rows(257, seed=s) for s in range(4)]
    exp = [sr.score(case.st, case.qz, case.queries, r) for r in rows]
    errors = []

    def run(first):
        try:
            for rep in range(6):
                k = (first + rep) % 4
                assert sr.same_answer(g.score_raw(case.queries, rows[k]), exp[k]), (first, rep)
        except Exception as e:                                  # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    ts = [threading.Thread(target=run, args=(0,)), threading.Thread(target=run, args=(2,))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[0]
