"""The masked range search's definition, its case table and the teeth of that table, on the CPU (tests/range_masked_ref.py; no GPU, no
native library).

* the reference (per query masked._knn over subset.filtered_lists with K = every stored point, then range_ref.cut) equals the second
  statement of the same thing (every probed entry with its terms; mask; running sums; sort) on every row of the table, for both widths.
* the two quantizer edits of range_ref.case work on the UInt16 cases: the twin cells tie, the hit query's residual is the codeword row
  exactly, and the entries at d == dc_hit are there.
* the table cannot go hollow: at w = kc at most 2 of the 20 table queries (the two "none" masks) have an empty row at r = +inf.
* every mutant differs from the reference somewhere on the table.
"""
import numpy as np
import pytest

import masked as mk
import range_masked_ref as rm


@pytest.mark.parametrize("stride", rm.STRIDES)
def test_reference_equals_the_second_statement(stride):
    for w in rm.WS:
        qis, radii, _ = rm.table(stride, w)
        assert rm.same(rm.model(stride, qis, radii, w), rm.expected(stride, w)), (stride, w)


@pytest.mark.parametrize("stride", rm.STRIDES)
def test_minus_one_is_the_plain_range_search(stride):
    """mask -1 for every query: the reference over the unfiltered lists"""
    c, _, _ = rm.case(stride)
    w = 3
    qis, radii, _ = rm.table(stride, w)
    none = np.full(len(qis), -1, np.int32)
    rows = [rm.cut(*mk._knn(c, c.ref, c.qs[qi], rm.N, w), r) for qi, r in zip(qis, radii)]
    assert rm.same(rm.reference(stride, qis, radii, w, none), rm.pack(rows))
    assert rm.same(rm.model(stride, qis, radii, w, none), rm.pack(rows))


@pytest.mark.parametrize("stride", rm.STRIDES)
def test_edits_and_hit_queries(stride):
    c, moq, hit_id = rm.case(stride)
    w = rm.KC
    # the twin cells: same centroid, so the same coarse distance for every query
    for qi in range(rm.NQ):
        cells, dcs = rm.coarse_order(stride, qi)
        assert dcs[list(cells).index(rm.TWIN_A)] == dcs[list(cells).index(rm.TWIN_B)]
    # the hit: the point's distance is its probe's dc itself, and a whole tie run sits there
    q_in, q_out = rm.NQ - 2, rm.NQ - 1
    cells, dcs = rm.coarse_order(stride, q_in)
    dchit = dcs[list(cells).index(rm.HIT)]
    E = rm.entries(stride, q_in)
    d = rm._running(E["dcs"][E["rank"]], E["T"])[:, -1]
    at = (E["lst"] == rm.HIT) & (d == dchit)
    assert at.sum() >= 2 and hit_id in E["id"][at], "the exact hit and its code row's ties sit at d == dc_hit"
    print("%s: %d entries at d == dc_hit" % (stride, int(at.sum())))
    if stride == "u16_m8":
        assert int(at.sum()) == 15
    if stride == "u16_m5":
        assert int(at.sum()) == 18
    assert (E["T"][at] == 0).all(), "every term of the hit row is +0"
    qis, radii, kinds = rm.table(stride, w)
    lims, ids, dd = rm.expected(stride, w)
    for row, (qi, kind) in enumerate(zip(qis, kinds)):
        got = ids[lims[row]:lims[row + 1]]
        if kind == "dchit" and qi == q_in:
            assert hit_id in got, "the mask selects the hit point: d == dc == r belongs to the result"
        if kind == "dchit-" and qi == q_in:
            assert hit_id not in got
        if qi == q_out:
            assert hit_id not in got, "the mask excludes the hit point"
    assert moq[q_in] >= 0 and moq[q_out] >= 0 and moq[q_in] != moq[q_out]


def test_table_is_not_hollow():
    for stride in rm.STRIDES:
        for w in rm.WS:
            qis, radii, kinds = rm.table(stride, w)
            lims = rm.expected(stride, w)[0]
            cnt = np.diff(lims)
            empty = [int(qi) for qi, k, n in zip(qis, kinds, cnt) if k == "inf" and n == 0 and qi < rm.NQ_TABLE]
            if w >= rm.KC:
                assert len(empty) <= 2, "at w = kc only the two 'none' masks give empty rows: %s" % empty
                assert all(mk.MASKS[mk.MASK_OF_QUERY[qi]][0] == "none" for qi in empty)
            else:
                assert len(empty) <= 10, (stride, w, empty)
            # neg keeps nothing; inf keeps every selected probed point; dmid- is a strict prefix of dmid wherever the row is not empty
            for row, k in enumerate(kinds):
                if k == "neg":
                    assert cnt[row] == 0
                if k == "dmid" and cnt[row] > 0:
                    assert cnt[row + 1] < cnt[row]
    # a tie run crosses D[mid] for several queries at w = kc: the inclusive cut is exercised
    for stride in rm.STRIDES:
        crossing = 0
        for qi in range(rm.NQ_TABLE):
            D = rm.full_sorted(stride, qi, rm.KC)[1]
            if len(D) > 2:
                mid = len(D) // 2
                crossing += bool(D[mid - 1] == D[mid] or (mid + 1 < len(D) and D[mid + 1] == D[mid]))
        assert crossing >= 3, (stride, crossing)


def _differs(name, mistake, strides):
    n = 0
    for stride in strides:
        for w in rm.WS:
            qis, radii, _ = rm.table(stride, w)
            n += not rm.same(rm.model(stride, qis, radii, w, mistake=mistake), rm.expected(stride, w))
    return n


@pytest.mark.parametrize("name", sorted(rm.MUTANTS))
def test_mutant_is_told_from_the_reference(name):
    assert _differs(name, rm.MUTANTS[name], rm.STRIDES) > 0, "mutant '%s' gives the reference's answer on every row of the table" % name
    if name.startswith("early-out"):
        assert _differs(name, rm.MUTANTS[name], rm.U16_STRIDES) > 0, "the early-out lives in the UInt16 form"


@pytest.mark.parametrize("name", sorted(rm.U16_MUTANTS))
def test_u16_mutant_is_told_from_the_reference(name):
    assert _differs(name, rm.U16_MUTANTS[name], rm.U16_STRIDES) > 0, "mutant '%s' gives the reference's answer on every UInt16 row" % name


def test_mutant_list():
    assert len(rm.MUTANTS) == 9 and len(rm.U16_MUTANTS) == 2
