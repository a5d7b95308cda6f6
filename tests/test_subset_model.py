"""The subset read-back has teeth (CPU; the GPU side is tests/test_gpu_subset.py).

tests/test_gpu_subset.py compares a subset view's exhaustive search (w = kc, K = everything) with the reference over
subset.filtered_lists.  Here, on the same case table -- lists, masks, both choices of nbits -- every wrong compaction of
subset.MUTANTS is put in filtered_lists' place: wherever its lists differ from the right ones at all, the reference's read-back over
them (helpers.numpy_knn_batch / u16_ref.knn, ids and distance bits) differs too, and every mutant does differ on the masks that are
there to catch it.  This is the role tests/test_write_path_model.py plays for the write path."""
import numpy as np
import pytest

import subset as sb

# where each mutant MUST show (the masks that are in the table for its sake); elsewhere it may coincide with the right lists
MUST_DIFFER = {
    "unstable order within a chunk": [("random_half", "max_plus_1"), ("every_other", "max_plus_1"), ("all", "max_plus_1")],
    "chunk edge dropped": [("all", "max_plus_1"), ("last_only", "max_plus_1"), ("run_at_chunk", "max_plus_1")],
    "chunk edge duplicated": [("all", "max_plus_1"), ("every_other", "max_plus_1"), ("run_at_chunk", "max_plus_1")],
    "bit looked up in word id >> 6": [("random_half", "max_plus_1"), ("first_only", "max_plus_1"), ("random_1pct", "max_plus_1")],
    "ids at or above nbits kept": [(m, "half_of_max") for m in sb.MASKS],
    "code rows left at their old positions": [("every_other", "max_plus_1"), ("random_half", "max_plus_1"), ("last_only", "max_plus_1")],
    "list_len left at the index's value": [(m, "max_plus_1") for m in sb.MASKS if m != "all"],
}


def test_the_table_has_the_lengths_the_kernels_can_go_wrong_at():
    C = sb.chunk()
    assert C % 256 == 0 and C >= 256
    assert set(sb.lens()) >= {0, 1, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 1} and len(sb.lens()) == sb.KC
    assert sorted(sb.code_stride(s) for s in sb.STRIDES) == [4, 8, 12, 12, 16, 48]


def test_filtered_lists_is_the_literal_filter():
    """filtered_lists against a per-entry Python loop: stored order, stored ids, ids at or above nbits dropped."""
    c = sb.case("u8_m3")
    off, codes, ids = c.lists()
    mask, nbits = c.mask("random_half", "half_of_max")
    exp_off, exp_codes, exp_ids = [0], [], []
    for l in range(sb.KC):
        for p in range(int(off[l]), int(off[l + 1])):
            i = int(ids[p])
            if i < nbits and mask[i]:
                exp_codes.append(codes[p])
                exp_ids.append(i)
        exp_off.append(len(exp_ids))
    got = sb.filtered_lists(off, codes, ids, mask)
    assert np.array_equal(got[0], exp_off) and np.array_equal(got[1], np.array(exp_codes)) and np.array_equal(got[2], exp_ids)
    assert 0 < len(exp_ids) < int((mask.sum()) * 1.01) and int(ids.max()) >= nbits


def test_pack_is_little_endian_within_a_word():
    m = np.zeros(64, bool)
    m[[0, 31, 32, 63]] = True
    assert sb.pack(m).tolist() == [0x80000001, 0x80000001]
    assert sb.pack(np.ones(33, bool)).tolist() == [0xFFFFFFFF, 1] and sb.pack(np.zeros(0, bool)).shape == (0,)


@pytest.mark.parametrize("nbits_kind", sb.NBITS)
@pytest.mark.parametrize("mask_kind", sb.MASKS)
@pytest.mark.parametrize("stride", ["u8_m8", "u16_m5"])
def test_every_mutant_changes_the_read_back(stride, mask_kind, nbits_kind):
    c = sb.case(stride)
    mask, nbits = c.mask(mask_kind, nbits_kind)
    assert len(mask) == nbits
    good = sb.filtered_lists(*c.lists(), mask)
    answer = c.exhaustive(good)
    assert (answer[2] == int(good[0][-1])).all(), "the read-back returns every kept entry"
    for name, mutant in sb.MUTANTS.items():
        bad = mutant(*c.lists(), mask)
        differs = not sb.same_lists(bad, good)
        if (mask_kind, nbits_kind) in MUST_DIFFER[name]:
            assert differs, "%s: the mutant coincides with the right compaction on a mask that is there to catch it" % name
        if differs:
            assert not sb.same_answer(c.exhaustive(bad), answer), "%s: wrong lists, same read-back (%s, %s, %s)" % (name, stride, mask_kind, nbits_kind)
