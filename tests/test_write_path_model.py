"""CPU side of the write-path suite (tests/write_path.py; the GPU side is tests/test_gpu_write_path.py).

(i)  The vectorised restatements np_delete / np_shift / np_append, and the step-by-step numpy restatement of the compaction and
     append kernels (DeviceModel), leave the lists the literal model of utils.jl (_RefModel) leaves, on the `chunks` geometry and for
     every deletion pattern the GPU file applies.
(ii) The exhaustive read-back has teeth: for each of four deliberately wrong compactions / appends, the reference's exhaustive
     answer over the wrong lists differs from its answer over the right ones, on the very shapes and the very two queries the GPU
     file uses.  Whether the checks the suite had before (48 queries, K = 10 / w = 5 and K = 4 / w = kc) would have seen each
     mutant is computed and printed (pytest -s), not asserted: it is a finding."""
import numpy as np
import pytest

import helpers
import write_path as wp
from test_gpu_parity import _RefModel


def _same_lists(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


@pytest.fixture(scope="module")
def small_case():
    """The `chunks` lists at the one-dword stride (the lists' maintenance does not look at the code bytes)."""
    ref, _ = wp.chunks_case("u8_cs4")
    return ref


@pytest.mark.parametrize("pattern", wp.PATTERNS)
def test_np_delete_equals_literal_model(small_case, pattern):
    ref = small_case
    dele = wp.pattern_ids(pattern, ref.offsets, ref.ids)
    model = _RefModel(ref.offsets, ref.codes, ref.ids)
    model.delete((dele.astype(np.int64) + 1).tolist())                        # delete_from_index! takes 1-based points
    exp = model.arrays(ref.m)
    got = wp.np_delete(ref.offsets, ref.codes, ref.ids, dele)
    assert _same_lists(got, exp), pattern
    assert got[3] == int(ref.offsets[-1]) - model.n()
    if pattern == "absent_and_duplicates":
        assert got[3] == 3
        assert wp.np_delete(ref.offsets, ref.codes, ref.ids, wp.absent_ids(int(ref.offsets[-1])))[3] == 0
    dev = wp.DeviceModel(*wp.lists_of(ref))                                  # the kernel's chunked, column-wise form, restated
    dev.compact(dele)
    assert _same_lists(dev.arrays(), exp), pattern


def test_np_shift_and_append_equal_literal_model(small_case):
    ref = small_case
    n = int(ref.offsets[-1])
    _, lst, codes = wp.append_batch(ref, 5, 70)
    model = _RefModel(ref.offsets, ref.codes, ref.ids)
    for i in range(70):
        model.push(int(lst[i]), codes[i], False)                            # push!: id = length(ivfadc)
    got = wp.np_append(ref.offsets, ref.codes, ref.ids, lst, codes, np.arange(n, n + 70, dtype=np.uint32))
    assert _same_lists(got, model.arrays(ref.m))
    dev = wp.DeviceModel(*wp.lists_of(ref))
    keep = np.array([i for i in range(70) if np.count_nonzero(lst[:i + 1] == lst[i]) <= 32])    # what fits the spare room
    dev.append(lst[keep], codes[keep], np.arange(len(keep), dtype=np.uint32) + 9000)
    assert _same_lists(dev.arrays(), wp.np_append(ref.offsets, ref.codes, ref.ids, lst[keep], codes[keep],
                                                  np.arange(len(keep), dtype=np.uint32) + 9000))
    model.push(int(lst[0]), codes[0], True)                                  # pushfirst!: every id up by one, then id 0
    got = wp.np_shift(*got, 1)
    got = wp.np_append(*got, lst[:1], codes[:1], np.array([0], np.uint32))
    assert _same_lists(got, model.arrays(ref.m))
    model.pop(True)                                                          # popfirst! == delete id 0
    assert _same_lists(wp.np_delete(*got, np.array([0], np.uint32)), model.arrays(ref.m))
    assert np.array_equal(wp.np_shift(ref.offsets, ref.codes, np.array([0xFFFFFFFF, 5], np.uint32), 1)[2], [0, 6])


@pytest.mark.parametrize("stride", sorted(wp.STRIDES))
@pytest.mark.parametrize("mutant", wp.MUTANTS)
def test_read_back_sees_the_mutant(stride, mutant):
    if not wp.mutant_applies(mutant, stride):
        ref, good, bad = wp.run_mutant(stride, mutant)
        if mutant == "second_column_from_destination":
            assert _same_lists(good, bad)            # a one-dword stride has no second column: the mutant is the same program
        return
    ref, good, bad = wp.run_mutant(stride, mutant)
    assert not _same_lists(good, bad)
    qs = wp.chunk_queries(stride, 2)
    rg, rb = wp.ref_with_lists(ref, *good), wp.ref_with_lists(ref, *bad)
    K = max(int(good[0][-1]), int(bad[0][-1]))
    assert not wp.same_answer(wp.ref_knn(rb, qs, K, ref.kc), wp.ref_knn(rg, qs, K, ref.kc)), \
        "the exhaustive read-back cannot tell %s from the right lists at %s" % (mutant, stride)
    for one in range(2):                             # ... and either query alone would do
        assert not wp.same_answer(wp.ref_knn(rb, qs[one:one + 1], K, ref.kc), wp.ref_knn(rg, qs[one:one + 1], K, ref.kc))
    print("FINDING %s at %s: the pre-existing style of check (48 queries, K=10/w=5 and K=4/w=kc) %s it"
          % (mutant, stride, "sees" if wp.pre_existing_check_sees(ref, good, bad) else "MISSES"))


def test_mutants_on_the_geometry_the_suite_had():
    """The targeted test the suite had (test_delete_pop_pushfirst_in_place_on_device): 900 points in 13 lists, cb = cs = 8.  One list
    there is longer than a chunk (by 29 points), the other twelve are not; the stride has no padding, so the cb / cs mix-up is the
    right program there.  Whether its own searches would have seen the other mutants on its own lists is printed, as above."""
    oidx, _ = helpers.build_index(610, 900, 24, 13, 8, 256)
    lens = np.diff(oidx.offsets)
    assert np.count_nonzero(lens > wp.CHUNK) == 1 and lens.max() < 2 * wp.CHUNK
    _, good, bad = wp.run_mutant_on(oidx, "append_at_len_times_cb")
    assert _same_lists(good, bad)
    its_request = np.random.default_rng(610).integers(0, 900, 57).astype(np.uint32)      # that test deletes 57 random ids
    for mutant in wp.MUTANTS[:3]:
        for name, dele in (("every other point", None), ("57 random ids", its_request)):
            _, good, bad = wp.run_mutant_on(oidx, mutant, dele)
            assert not _same_lists(good, bad), mutant
            print("FINDING %s on the 900-point geometry, %s deleted: the pre-existing style of check %s it"
                  % (mutant, name, "sees" if wp.pre_existing_check_sees(oidx, good, bad) else "MISSES"))
