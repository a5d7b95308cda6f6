"""The model of the masked search (tests/masked.py) on the CPU: it is the reference over the filtered lists, it agrees with the plain
reference where nothing is filtered, and the read-back the GPU test makes -- K = 1963 and K = 64 at w = kc, on the case table -- tells
every wrong implementation of masked.MUTANTS from it.  The one mutant that only renumbers the keys is shown EQUIVALENT: ids and distances
cannot tell it, which is why the kernels may keep the original visit numbers."""
import numpy as np
import pytest

import masked as mk
import subset as sb

# the mutants run on one 8-bit and one 16-bit stride (they edit which entries are kept, not how a distance is formed); the model's own
# identities run on every stride
MUTANT_STRIDES = ("u8_m8", "u16_m5")


def test_case_table_is_the_one_the_gpu_test_needs():
    c = mk.case("u8_m8")
    assert tuple(np.diff(c.ref.offsets)) == mk.LENS and c.ref.kc == mk.KC and c.qs.shape[0] == mk.NQ == 20
    assert sorted(c.ref.ids.tolist()) == list(range(mk.N)), "ids are a permutation"
    assert len(np.unique(c.ref.codes, axis=0)) <= mk.POOL
    kept = mk.kept("u8_m8")
    assert kept[mk.MASKS.index(("all", "max_plus_1"))] == mk.N and kept[mk.MASKS.index(("none", "max_plus_1"))] == 0
    assert (kept <= mk.K_REG - 7).sum() >= 4, "several masks come back whole at K = 64"
    assert len(set(kept.tolist())) >= 8, kept
    # every group of four (in query order) holds four different mask numbers or -1; the first and the last mix masked and unmasked slots
    moq = mk.MASK_OF_QUERY
    for g in range(0, mk.NQ, 4):
        grp = moq[g:g + 4]
        assert len(set(grp[grp >= 0].tolist())) == (grp >= 0).sum()
    assert (moq[:4] < 0).any() and (moq[:4] >= 0).any() and (moq[-4:] < 0).any() and (moq[-4:] >= 0).any()


@pytest.mark.parametrize("stride", sorted(mk.STRIDES))
def test_model_equals_the_plain_reference_where_nothing_is_filtered(stride):
    c = mk.case(stride)
    ones = [np.ones(mk.N, bool)]
    plain = mk.plain_reference(c, mk.K_REG, mk.KC)
    assert mk.same_answer(mk.masked_reference(c, ones, np.zeros(mk.NQ, np.int32), mk.K_REG, mk.KC), plain), "all-ones mask"
    assert mk.same_answer(mk.masked_reference(c, mk.masks(stride), np.full(mk.NQ, -1, np.int32), mk.K_REG, mk.KC), plain), "-1"
    assert mk.same_answer(mk.masked_reference(c, ones, np.zeros(mk.NQ, np.int32), 10, 3), mk.plain_reference(c, 10, 3)), "w < kc"


@pytest.mark.parametrize("stride", sorted(mk.STRIDES))
@pytest.mark.parametrize("K, w", [(mk.K_ALL, mk.KC), (mk.K_REG, mk.KC), (10, 3)])
def test_original_visit_numbers_give_the_model(stride, K, w):
    """removing entries keeps the order of the rest: the first K kept entries of the unfiltered order ARE the filtered-lists result"""
    c = mk.case(stride)
    model = mk.masked_reference(c, mk.masks(stride), mk.MASK_OF_QUERY, K, w)
    assert mk.same_answer(mk.original_keys(c, mk.masks(stride), mk.MASK_OF_QUERY, K, w), model)
    kept = mk.kept(stride)
    if w == mk.KC:
        for qi, r in enumerate(mk.MASK_OF_QUERY):
            assert model[2][qi] == min(K, mk.N if r < 0 else kept[r])


@pytest.mark.parametrize("stride", MUTANT_STRIDES)
@pytest.mark.parametrize("name", sorted(mk.MUTANTS))
def test_the_read_back_tells_every_mutant_from_the_model(stride, name):
    c = mk.case(stride)
    for K in (mk.K_ALL, mk.K_REG):
        model = mk.masked_reference(c, mk.masks(stride), mk.MASK_OF_QUERY, K, mk.KC)
        got = mk.MUTANTS[name](c, mk.masks(stride), mk.MASK_OF_QUERY, K, mk.KC)
        if name == "filter behind the top-K" and K >= mk.N:
            # no result to change: a top-K that holds every probed entry loses nothing to a filter behind it; K = 64 is where it shows
            assert mk.same_answer(got, model)
            continue
        assert not mk.same_answer(got, model), "%s is not seen at K = %d" % (name, K)


@pytest.mark.parametrize("stride", MUTANT_STRIDES)
def test_renumbered_keys_are_equivalent_not_caught(stride):
    """EQUIVALENT, and meant to be: a key's visit number only orders ties, and a filter keeps the order of what it keeps"""
    c = mk.case(stride)
    (name, fn), = mk.EQUIVALENT.items()
    for K in (mk.K_ALL, mk.K_REG):
        assert mk.same_answer(fn(c, mk.masks(stride), mk.MASK_OF_QUERY, K, mk.KC),
                              mk.original_keys(c, mk.masks(stride), mk.MASK_OF_QUERY, K, mk.KC)), name


def test_forced_width_restatement():
    """what a forced width narrows to (masked.forced_qg, the GPU test's expectation for last_qg): only the hard 160 KB limit narrows it"""
    assert mk.forced_qg("u8_m8", 64, 4) == 4 and mk.forced_qg("u8_m8", mk.K_ALL, 4) == 2 and mk.forced_qg("u8_m8", mk.K_ALL, 2) == 2
    assert mk.forced_qg("u8_m48", 64, 4) == 2 and mk.forced_qg("u8_m48", mk.K_ALL, 4) == 1
    assert mk.forced_qg("u8_m3", 64, 4) == 4 and sb.code_stride("u8_m3") == 4
