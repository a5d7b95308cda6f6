"""The numpy model of ivfadc_score_ids (tests/score_ref.py) against the oracle's search, and the case table against the ways an
implementation goes wrong.  CPU only.

1. The model is the search: for every stored id of every index of the table, the model's distance is the distance the oracle's
   knn_search(w = kc, K = n) reports for that id, bit for bit.  (The C oracle serves 8-bit codes; the UInt16 indexes of the table are
   held against tests/u16_ref.py, the numpy restatement of the same loop that the UInt16 suite is pinned to.  An index with repeated
   stored ids reports one distance per stored ENTRY: the model's is the one of the entry locate names.)
2. The case table has teeth: each of score_ref.MUTANTS changes at least one distance bit or found flag somewhere on the table, so what
   tests/test_gpu_score.py compares the device with is a comparison none of them would pass.  The arithmetic mutants (a contracted
   multiply-add, dc added last, reversed sub-space sums, a pairwise sum, the reconstructed point's distance, float64 tables) are
   caught on the rounding-hostile inputs; the others on repeated ids, stale rows, absent ids, ragged counts, permuted labels and the
   shared row."""
import numpy as np
import pytest

import reconstruct_ref as rr
import score_ref as sr
import u16_ref
from oracle import oracle as ora
from test_reconstruct_model import stale_case

ARITHMETIC = ("fma", "dc_last", "reversed", "pairwise", "reconstruct", "f64")


def search_everything(case):
    """(ids, dists) per query of the exhaustive search over the case's live lists."""
    off, codes, ids = case.st.arrays()
    n = len(ids)
    qz = case.qz
    if case.u16:
        ix = u16_ref.U16Index(qz.centroids, qz.codebooks, qz.labels, off, codes, ids)
        out = [u16_ref.knn_one(ix, q, n, qz.kc) for q in case.queries]
        return [o[0] for o in out], [o[1] for o in out]
    oidx = ora.OracleIndex(qz.centroids, qz.codebooks, qz.labels, off, codes, ids)
    gi, gd, gc = oidx.knn_search(case.queries, n, qz.kc)
    assert (gc == n).all()
    return list(gi), list(gd)


@pytest.mark.parametrize("name", sorted(sr.case_table()))
def test_model_is_the_distance_the_search_reports(name):
    case = sr.case_table()[name]
    stored = case.stored_ids()
    uniq, cnt = np.unique(stored, return_counts=True)
    once = uniq[cnt == 1]
    dists, found = sr.score(case.st, case.qz, case.queries, uniq)                  # the shared row: every stored id against every query
    assert found.all() and np.isfinite(dists).all()
    s_ids, s_dists = search_everything(case)
    for q in range(len(case.queries)):
        order = np.argsort(s_ids[q], kind="stable")
        ids_sorted, d_sorted = s_ids[q][order], s_dists[q][order]
        at = np.searchsorted(ids_sorted, once)
        assert np.array_equal(ids_sorted[at], once)
        got, exp = dists[q][np.searchsorted(uniq, once)], d_sorted[at]
        assert rr.same_bits(got, exp), "%s, query %d: %d of %d ids differ from the search" % (
            name, q, int((got.view(np.uint32) != np.ascontiguousarray(exp).view(np.uint32)).sum()), len(once))
        for v in uniq[cnt > 1]:                                                    # a repeated id: one of its entries' distances
            mine = dists[q][np.searchsorted(uniq, v)]
            theirs = s_dists[q][s_ids[q] == v]
            assert len(theirs) > 1 and (theirs.view(np.uint32) == mine.view(np.uint32)).any(), (name, q, int(v))
    if name == "duplicates":
        assert (cnt > 1).sum() >= 2


def test_table_covers_the_kernels_paths():
    t = sr.case_table()
    shapes = {(c.qz.d, c.qz.m, c.qz.dsub) for c in t.values()}
    assert {(32, 8, 4), (10, 2, 5), (6, 1, 6), (96, 16, 6), (128, 8, 16), (768, 48, 16)} <= shapes
    assert t["d768_m48"].qz.kc == 4 and t["d10_m2"].qz.d * 4 % 16 != 0
    assert t["ksub2"].qz.ksub == 2 and t["u16"].qz.ksub == 300 and t["u16"].u16 and t["u16_m2"].u16
    for name in ("d32_m8", "ksub2", "u16"):
        qz = t[name].qz
        assert any(not np.array_equal(qz.labels[i], np.arange(qz.ksub)) for i in range(qz.m)), name + ": permuted labels"
    assert {c.kind for c in t.values()} == set(sr.KINDS)
    for c in t.values():
        assert 150 <= len(c.stored_ids()) <= 1200, "small indexes"


def _table_inputs():
    """(what, st, qz, queries, ids, counts) the GPU test also walks: per-query rows of the edge sizes with ragged counts, and a shared row"""
    for name, case in sr.case_table().items():
        for C in sr.EDGE_C:
            yield "%s, C = %d" % (name, C), case.st, case.qz, case.queries[:3], case.rows(C, nq=3), None
        yield name + ", ragged counts", case.st, case.qz, case.queries, case.rows(65), case.ragged_counts(65)
        yield name + ", shared row", case.st, case.qz, case.queries, case.rows(65, seed=1, nq=1)[0], None
    case, only_stale = stale_case()
    live = case.stored_ids()
    ids = np.random.default_rng(3).permutation(np.concatenate([live[::40], only_stale[:40]])).astype(np.uint32)
    qs = np.random.default_rng(4).random((2, case.qz.d), dtype=np.float32)
    yield "stale rows", case.st, case.qz, qs, ids, None


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_case_table_tells_the_model_from_every_wrong_implementation(mutant):
    seen = []
    for what, st, qz, qs, ids, counts in _table_inputs():
        if mutant in ARITHMETIC and not what.endswith("shared row"):
            continue                                                              # (one walk of every case suffices for the sums)
        if not sr.same_answer(sr.score(st, qz, qs, ids, counts), sr.score(st, qz, qs, ids, counts, mutant)):
            seen.append(what)
    assert seen, "no input of the table tells the model from `%s`" % mutant
    where = {"first_list": "duplicates", "to_capacity": "stale rows", "counts_ignored": "ragged counts", "shared_stride_c": "shared row",
             "label_as_index": "d32_m8"}.get(mutant)
    if where:
        assert any(where in s for s in seen), (mutant, seen)
    if mutant in ARITHMETIC:
        kinds = {sr.case_table()[s.split(",")[0]].kind for s in seen}
        assert kinds & {"graded", "graded_reversed", "dc_dominant", "exact_hits"}, (mutant, seen)


def test_absent_dead_and_repeated_slots():
    case = sr.case_table()["d32_m8"]
    ids = case.rows(65)
    counts = case.ragged_counts(65)
    dists, found = sr.score(case.st, case.qz, case.queries, ids, counts)
    stored = set(case.stored_ids().tolist())
    assert (counts == 0).any() and (counts == 65).any()
    for q in range(len(case.queries)):
        for j in range(65):
            live = j < counts[q]
            assert found[q, j] == (live and int(ids[q, j]) in stored)
            if not found[q, j]:
                assert dists[q, j].view(np.uint32) == sr.INF_BITS
        row = ids[q, :counts[q]]
        for v in np.unique(row):
            at = np.nonzero(row == v)[0]
            assert len(set(dists[q, at].view(np.uint32).tolist())) == 1, "a repeated id has one distance"
    assert 0xFFFFFFFF in ids and (~found[counts == 65]).any()
    # the shared row is the same row given to every query
    shared = sr.score(case.st, case.qz, case.queries, ids[1])
    per_query = sr.score(case.st, case.qz, case.queries, np.tile(ids[1], (len(case.queries), 1)))
    assert sr.same_answer(shared, per_query)
