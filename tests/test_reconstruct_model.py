"""The numpy model of ivfadc_locate / ivfadc_reconstruct (tests/reconstruct_ref.py) against the reference, and the case table against the
ways an implementation goes wrong.  CPU only.

1. On unique ids the model is the literal restatement of utils.jl:41-81 (the loop of _pop!, findfirst, centre + _decode_point): same
   list, same position, same Float32 bits, for every stored id of every case with unique ids.
2. On repeated stored ids -- which the reference cannot build but a caller's lists can hold -- the model is still that loop: the last
   list, the first position.
3. The case table tells the model from each of the wrong implementations of reconstruct_ref.MUTANTS: for every one there is a case and a
   request size of the table on which its answer differs from the model's.  What tests/test_gpu_reconstruct.py compares the device with
   is therefore a comparison none of them would pass.
4. The stale-row case: after the decoys of list_end.hostile_case are deleted, ids that live only in stale rows behind list_len are absent
   for the model and present for the implementation that reads up to the capacity."""
import numpy as np
import pytest

import list_end as le
import reconstruct_ref as rr
import write_path as wp

UNIQUE = ("m8", "m3", "dsub5", "u16", "perm8", "perm16", "edge_lens", "upper_ids", "bit_patterns")


def stale_case(kind="m8_d32"):
    """(Case over the device model after the decoys' deletion, ids that lie ONLY behind a list's end)."""
    hc = le.hostile_case(kind)
    _, model, _ = le.walk_states(hc, "decoys_deleted")
    st = rr.Stored.from_device_model(model)
    qz = rr.Quantizers(hc.ref.centroids, hc.ref.codebooks, hc.ref.labels)
    case = rr.Case("stale_" + kind, qz, st)
    behind = np.concatenate([st.ids[l][st.len[l]:] for l in range(len(st.len))])
    only_stale = np.setdiff1d(behind, case.stored_ids())
    return case, only_stale.astype(np.uint32)


@pytest.mark.parametrize("name", UNIQUE)
def test_model_is_the_literal_loop_on_unique_ids(name):
    case = rr.case_table()[name]
    ids = case.stored_ids()
    assert len(set(ids.tolist())) == len(ids)
    pick = ids if len(ids) <= 300 else ids[np.random.default_rng(5).choice(len(ids), 300, replace=False)]
    lists, pos = rr.locate(case.st, pick)
    vec, found = rr.reconstruct(case.st, case.qz, pick)
    assert found.all()
    for j, v in enumerate(pick):
        cl, idx, rec = rr.literal(case.st, case.qz, int(v))
        assert (cl, idx) == (lists[j], pos[j]) and rr.same_bits(rec, vec[j]), (name, int(v))


def test_model_is_the_literal_loop_on_repeated_ids():
    case = rr.case_table()["duplicates"]
    for kind, v, l, p in case.notes:
        lists, pos = rr.locate(case.st, [v])
        assert (int(lists[0]), int(pos[0])) == (l, p), kind
        cl, idx, rec = rr.literal(case.st, case.qz, v)
        assert (cl, idx) == (l, p) and rr.same_bits(rec, rr.reconstruct(case.st, case.qz, [v])[0][0])


def test_absent_ids_and_request_order():
    case = rr.case_table()["upper_ids"]
    req = case.requests(65)
    lists, pos = rr.locate(case.st, req)
    vec, found = rr.reconstruct(case.st, case.qz, req)
    stored = set(case.stored_ids().tolist())
    assert not found.all() and found.any() and len(set(req.tolist())) < len(req), "absent ids and repeats are both in the request"
    for j, v in enumerate(req.tolist()):
        assert found[j] == (v in stored) == (lists[j] >= 0) == (pos[j] >= 0)
        if not found[j]:
            assert rr.same_bits(vec[j], np.zeros(case.qz.d, np.float32)), "+0.0, not -0.0"
        else:
            assert case.st.ids[lists[j]][pos[j]] == v
    assert {0xFFFFFFFF, 0x80000000, 0} <= stored and (req >= 0x80000000).any()


def test_bit_pattern_case_holds_the_patterns():
    case = rr.case_table()["bit_patterns"]
    vec, found = rr.reconstruct(case.st, case.qz, case.stored_ids())
    bits = vec.view(np.uint32)
    expo = (bits >> 23) & 0xFF
    assert found.all()
    assert (bits == 0x80000000).any(), "-0.0 results"
    assert ((expo == 0) & ((bits & 0x7FFFFF) != 0)).any(), "subnormal results"
    assert (np.abs(vec[np.isfinite(vec)]) > 1e38).any(), "large results"


def _differs(case, req, mutant):
    l0, p0 = rr.locate(case.st, req)
    v0, f0 = rr.reconstruct(case.st, case.qz, req)
    l1, p1 = rr.locate(case.st, req, mutant)
    v1, f1 = rr.reconstruct(case.st, case.qz, req, mutant)
    return not (np.array_equal(l0, l1) and np.array_equal(p0, p1) and np.array_equal(f0, f1) and rr.same_bits(v0, v1))


@pytest.mark.parametrize("mutant", rr.MUTANTS)
def test_case_table_tells_the_model_from_every_wrong_implementation(mutant):
    table = rr.case_table()
    seen = []
    if mutant == "to_capacity":
        case, only_stale = stale_case()
        assert len(only_stale) > 0
        if _differs(case, only_stale[:64], mutant):
            seen.append(case.name)
    else:
        for name, case in table.items():
            for size in rr.REQUEST_SIZES:
                req = case.requests(size)
                if name == "duplicates":
                    req = np.concatenate([req, np.array([v for _, v, _, _ in case.notes], np.uint32)])
                if _differs(case, req, mutant):
                    seen.append((name, size))
                    break
    assert seen, "no case of the table tells the model from `%s`" % mutant
    where = {"first_list": "duplicates", "last_position": "duplicates", "other_lists_centre": "duplicates", "label_as_index": "perm8",
             "signed_ids": "upper_ids"}.get(mutant)
    if where:
        assert any(s[0] == where for s in seen), (mutant, seen)


def test_stale_ids_are_absent():
    case, only_stale = stale_case()
    lists, pos = rr.locate(case.st, only_stale)
    assert (lists == -1).all() and (pos == -1).all()
    l1, _ = rr.locate(case.st, only_stale, "to_capacity")
    assert (l1 >= 0).all()
    # and the model over the device model's live part is the model over the lists the reference's maintenance leaves
    hc = le.hostile_case("m8_d32")
    lists_ref, _, _ = le.walk_states(hc, "decoys_deleted")
    assert all(np.array_equal(a, b) for a, b in zip(case.st.arrays(), lists_ref))
    assert wp.is_u16(hc.ref) is False
