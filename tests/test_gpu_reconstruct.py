"""ivfadc_locate / ivfadc_reconstruct on the GPU against the numpy model of tests/reconstruct_ref.py: locations exact, vector bits
identical (the CPU side is tests/test_reconstruct_model.py: the case table tells the model from eight wrong implementations).

Small indexes (d = 24, kc = 13, n about 900): code strides 8 and 4 (m = 8, m = 3), dsub = 5 (d = 50, m = 10), a UInt16 handle (ksub = 300),
permuted labels on both code widths, list lengths on both sides of a wave and of a workgroup, request sizes 1 / 2 / 64 / 65 / 1000 with
repeats, absent ids and ids >= 2^31 (0xFFFFFFFF among them), stored duplicates within and across lists, subnormal / -0.0 / large
components; ids that live only in stale rows behind list_len after a delete (lists built as tests/list_end.py builds them); in-place and
overflowing appends; a plain view, a subset view, a stale view; device-synthesised lists against the oracle's regeneration rule; an
:opq-loaded golden file (no rotation applied); the _device entries fed straight from ivfadc_search_device; two threads on an index and
its view; the pop / popfirst loop on the rewired path.  Every request with a narrow id span takes the exact bitmap, every request that
holds 0 and 0xFFFFFFFF the hashed filter (csrc/reconstruct_plan.h), so both prefilters are compared on every case."""
import os
import threading

import numpy as np
import pytest

import helpers
import list_end as le
import reconstruct_ref as rr
import write_path as wp
from oracle import oracle as ora
from test_reconstruct_model import stale_case

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def handle_of(native, case):
    off, codes, ids = case.st.arrays()
    return native.IVFADCIndex.from_arrays(case.qz.centroids, case.qz.codebooks, case.qz.labels, off, codes, ids)


def check(g, st, qz, req, what):
    """locate and reconstruct of `req` on handle g against the model over (st, qz): exact."""
    req = np.asarray(req, np.uint32)
    el, ep = rr.locate(st, req)
    ev, ef = rr.reconstruct(st, qz, req)
    gl, gp = g.locate_raw(req)
    gv, gf = g.reconstruct_raw(req)
    assert gl.dtype == np.int32 and gp.dtype == np.int64 and gv.dtype == np.float32 and gv.shape == (len(req), qz.d)
    bad = np.nonzero((gl != el) | (gp != ep))[0]
    assert bad.size == 0, "%s: request slot %d (id %d): located at (%d, %d), the model says (%d, %d)" % (
        what, bad[0], req[bad[0]], gl[bad[0]], gp[bad[0]], el[bad[0]], ep[bad[0]])
    assert np.array_equal(gf, ef), "%s: found flags differ at slot %d" % (what, int(np.nonzero(gf != ef)[0][0]))
    gb, eb = gv.view(np.uint32), ev.view(np.uint32)
    if not np.array_equal(gb, eb):
        j, t = (int(x[0]) for x in np.nonzero(gb != eb))
        raise AssertionError("%s: slot %d (id %d) component %d: %s, the model says %s" % (what, j, req[j], t, float(gv[j, t]).hex(),
                                                                                        float(ev[j, t]).hex()))


def requests_of(case):
    """The table's request sizes (mixed: hashed filter), the same sizes from stored ids of a narrow span (exact bitmap), everything stored."""
    stored = case.stored_ids()
    rng = np.random.default_rng(77)
    low = stored[stored < 0x10000]
    out = [("mixed %d" % s, case.requests(s)) for s in rr.REQUEST_SIZES]
    out += [("narrow %d" % s, rng.choice(low, s, replace=s > len(low)).astype(np.uint32)) for s in rr.REQUEST_SIZES[:4]]
    out.append(("every stored id", rng.permutation(stored)))
    out += [("note %s" % kind, np.array([v, v], np.uint32)) for kind, v, _, _ in case.notes]
    return out


@pytest.mark.parametrize("name", sorted(rr.case_table()))
def test_case_table(native, name):
    case = rr.case_table()[name]
    g = handle_of(native, case)
    for what, req in requests_of(case):
        check(g, case.st, case.qz, req, "%s, %s" % (name, what))
    # n == 0 is fine, and says nothing
    assert g.locate_raw(np.zeros(0, np.uint32))[0].shape == (0,) and g.reconstruct_raw(np.zeros(0, np.uint32))[0].shape == (0, case.qz.d)


def test_python_entries_and_absent_ids(native):
    case = rr.case_table()["upper_ids"]
    g = handle_of(native, case)
    stored = case.stored_ids()
    lists, pos = native.locate(g, stored[:5])
    assert np.array_equal(lists, rr.locate(case.st, stored[:5])[0]) and np.array_equal(pos, rr.locate(case.st, stored[:5])[1])
    vec = native.reconstruct(g, [0xFFFFFFFF, 0, 0x80000000])
    assert rr.same_bits(vec, rr.reconstruct(case.st, case.qz, [0xFFFFFFFF, 0, 0x80000000])[0])
    absent = int(np.setdiff1d(np.arange(3000), stored)[0])
    with pytest.raises(AssertionError, match="id %d is not stored" % absent):
        native.reconstruct(g, [int(stored[0]), absent, 0xFFFFFFFD])
    vec, found = g.reconstruct_raw([absent])
    assert not found[0] and rr.same_bits(vec, np.zeros((1, case.qz.d), np.float32))


def test_empty_index_and_states(native):
    from ivfadc_jl_amd import _native as nat
    case = rr.case_table()["m8"]
    g = native.IVFADCIndex.from_arrays(case.qz.centroids, case.qz.codebooks, case.qz.labels)          # never given lists: an empty index
    lists, pos = g.locate_raw([0, 5, 0xFFFFFFFF])
    assert (lists == -1).all() and (pos == -1).all() and not g.reconstruct_raw([0])[1].any()
    g = handle_of(native, case)
    g.set_list_partition(2, 0)
    with pytest.raises(nat.IVFADCError) as e:
        g.locate_raw([0])
    assert e.value.code == nat.ERR_STATE
    g.set_list_partition(1, 0)
    check(g, case.st, case.qz, case.requests(64), "after the partition is switched off")


@pytest.mark.parametrize("kind", ("m8_d32", "u16"))
def test_ids_in_stale_rows_are_absent(native, kind):
    """the decoys of list_end.hostile_case are deleted in place: their rows and ids stay behind list_len"""
    hc = le.hostile_case(kind)
    g = wp.gpu_handle(native, hc.ref)
    g.search_raw(hc.qs[-1:], 1, 1)                             # the device layout is current: the delete below edits it in place
    assert g._delete_ids(le.all_decoy_ids(hc)) == len(le.all_decoy_ids(hc))
    case, only_stale = stale_case(kind)
    assert len(only_stale) >= 16
    lists, pos = g.locate_raw(only_stale)
    assert (lists == -1).all() and (pos == -1).all(), "an id behind list_len was read as an entry (list %d)" % lists.max()
    vec, found = g.reconstruct_raw(only_stale[:64])
    assert not found.any() and not vec.view(np.uint32).any()
    live = case.stored_ids()
    req = np.random.default_rng(3).permutation(np.concatenate([live[::40], only_stale[:40]]))
    check(g, case.st, case.qz, req, "stale rows, " + kind)
    check(g, case.st, case.qz, np.array([0xFFFFFFFF, 0], np.uint32), "stale rows, hashed, " + kind)


def test_after_appends_in_place_and_overflowing(native):
    case = rr.case_table()["m8"]
    qz = case.qz
    g = handle_of(native, case)
    g.search_raw(qz.centroids[:1], 1, 1)                       # layout current: capacity len + max(32, len / 8) per list
    n = len(g)
    rng = np.random.default_rng(9)
    pts = (qz.centroids[rng.integers(0, qz.kc, 20)] + np.float32(0.01) * rng.standard_normal((20, qz.d))).astype(np.float32)
    before = g.get_stats()["inplace_appends"]
    g._append(pts, np.arange(n, n + 20, dtype=np.uint32))
    assert g.get_stats()["inplace_appends"] == before + 1, "20 points over 13 lists fit the spare room"
    st = rr.Stored.from_lists(*g._lists())
    assert sum(st.len) == n + 20
    check(g, st, qz, np.concatenate([np.arange(n - 5, n + 25), case.requests(64)]).astype(np.uint32), "after an in-place append")
    # one list overflows: the mirror is ahead of the device copy until the entry lays the lists out again
    big = int(np.argmax(st.len))
    room = int(wp.capacity(np.array(st.len))[big]) - st.len[big]
    many = np.repeat(qz.centroids[big:big + 1], room + 50, 0)
    g._append(many, np.arange(n + 20, n + 70 + room, dtype=np.uint32))
    assert g.get_stats()["inplace_appends"] == before + 1, "this one did not fit"
    st = rr.Stored.from_lists(*g._lists())
    assert st.len[big] >= room + 50
    check(g, st, qz, np.concatenate([np.arange(n, n + 70 + room)[::3], case.requests(65)]).astype(np.uint32), "after an overflowing append")
    g._shift_ids(1)
    st = rr.Stored.from_lists(*g._lists())
    check(g, st, qz, np.array([0, 1, n + 70 + room, n + 69 + room], np.uint32), "after a shift")


def test_views(native):
    from ivfadc_jl_amd import _native as nat
    case = rr.case_table()["edge_lens"]
    g = handle_of(native, case)
    v = g.clone_view()
    for what, req in requests_of(case)[:6]:
        check(v, case.st, case.qz, req, "plain view, " + what)
    stored = case.stored_ids()
    keep = np.sort(stored)[::3]
    s = g.subset(ids=keep)
    off, codes, ids = case.st.arrays()
    sel = np.isin(ids, keep)
    sub_off = np.concatenate([[0], np.cumsum([sel[off[l]:off[l + 1]].sum() for l in range(case.qz.kc)])]).astype(np.int64)
    sub = rr.Stored.from_lists(sub_off, codes[sel], ids[sel])
    dropped = np.setdiff1d(stored, keep)
    assert (s.locate_raw(dropped[:100])[0] == -1).all(), "an id the subset dropped is absent"
    check(s, sub, case.qz, np.random.default_rng(4).permutation(np.concatenate([keep[:200], dropped[:60]])), "subset view")
    # positions are the subset's own: at least one kept id moved
    assert (s.locate_raw(keep)[1] != g.locate_raw(keep)[1]).any()
    g._delete_ids(stored[:1])
    for stale in (v, s):
        for call in (lambda h: h.locate_raw(keep[:3]), lambda h: h.reconstruct_raw(keep[:3])):
            with pytest.raises(nat.IVFADCError) as e:
                call(stale)
            assert e.value.code == nat.ERR_STATE


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
    check(g, st, qz, rng.permutation(n).astype(np.uint32), "synthetic, every id")
    check(g, st, qz, np.array([n, 0, n - 1, 0xFFFFFFFF, 5, 5], np.uint32), "synthetic, absent and repeated")
    check(g.clone_view(), st, qz, rng.integers(0, n, 65).astype(np.uint32), "synthetic, view")


def test_opq_loaded_golden_file(native):
    """_decode_point does not apply the rotation (utils.jl:71-81), so neither does ivfadc_reconstruct"""
    import ctypes as C
    from ivfadc_jl_amd import _native as nat
    idx = native.load_ivfadc_index(os.path.join(GOLDEN, "persistency_hand_f32_u16_opq.bin"))
    rotated = C.c_int(0)
    nat.check(nat.lib().ivfadc_get_rotation(idx._h, C.byref(rotated), None))
    assert rotated.value == 1
    st = rr.Stored.from_lists(*idx._lists())
    qz = rr.Quantizers(idx._centroids, idx._codebooks, idx._labels)
    stored = np.concatenate([st.ids[l] for l in range(len(st.len))])
    check(idx, st, qz, np.concatenate([stored, stored[::-1], [len(stored) + 3]]).astype(np.uint32), ":opq file")


def test_device_entries_fed_from_search_device(native):
    """ids that a search left in device memory become locations and vectors in device memory"""
    import torch
    case = rr.case_table()["upper_ids"]
    qz = case.qz
    g = handle_of(native, case)
    dev = "cuda:0"
    nq, K = 24, 10
    qs = np.random.default_rng(6).random((nq, qz.d), dtype=np.float32)
    dq = torch.from_numpy(qs).to(dev)
    di = torch.zeros((nq, K), dtype=torch.int32, device=dev)
    dd = torch.zeros((nq, K), dtype=torch.float32, device=dev)
    dc = torch.zeros(nq, dtype=torch.int32, device=dev)
    dl = torch.full((nq * K,), 7, dtype=torch.int32, device=dev)
    dp = torch.full((nq * K,), 7, dtype=torch.int64, device=dev)
    dv = torch.full((nq * K, qz.d), 7.0, dtype=torch.float32, device=dev)
    df = torch.full((nq * K,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.search_device(nq, dq.data_ptr(), K, 4, di.data_ptr(), dd.data_ptr(), dc.data_ptr())
    g.locate_device(nq * K, di.data_ptr(), dl.data_ptr(), dp.data_ptr())
    g.reconstruct_device(nq * K, di.data_ptr(), dv.data_ptr(), df.data_ptr())
    g.sync()
    req = di.cpu().numpy().view(np.uint32).reshape(-1)
    assert (dc.cpu().numpy() == K).all() and (req >= 0x80000000).any()
    el, ep = rr.locate(case.st, req)
    ev, ef = rr.reconstruct(case.st, qz, req)
    assert np.array_equal(dl.cpu().numpy(), el) and np.array_equal(dp.cpu().numpy(), ep)
    assert np.array_equal(df.cpu().numpy().astype(bool), ef) and ef.all() and rr.same_bits(dv.cpu().numpy(), ev)
    # absent ids, no found array, and the reconstruction of a neighbour is near its query's
    mixed = torch.from_numpy(case.requests(65).view(np.int32)).to(dev)
    torch.cuda.synchronize()
    g.reconstruct_device(65, mixed.data_ptr(), dv.data_ptr(), None)
    g.sync()
    assert rr.same_bits(dv.cpu().numpy()[:65], rr.reconstruct(case.st, qz, case.requests(65))[0])
    # the host entries on the same ids give the same bytes
    assert rr.same_bits(g.reconstruct_raw(req)[0], ev)


def test_more_wanted_ids_than_the_lds_filter_takes(native):
    """16 384 wanted ids of a wide or unknown span are the hashed filter's cap (csrc/reconstruct_plan.h): one more, and the pass runs
    behind a bitmap over the span, which the device entry's kernels read from the sorted ids.  Both sides of the cap, both entries."""
    import torch
    case = rr.case_table()["upper_ids"]
    g = handle_of(native, case)
    stored = case.stored_ids()
    cap = 16384
    rng = np.random.default_rng(8)
    dev = "cuda:0"
    for nwant in (cap, cap + 1):
        absent = (0x90000000 + 3 * np.arange(nwant - len(stored) - 1)).astype(np.uint32)
        req = rng.permutation(np.concatenate([stored, absent, [0xFFFFFFFD]]).astype(np.uint32))
        assert len(np.unique(req)) == nwant and int(req.max()) - int(req.min()) > 1 << 30
        el, ep = rr.locate(case.st, stored)
        ev, _ = rr.reconstruct(case.st, case.qz, stored)
        where = np.concatenate([np.nonzero(req == v)[0] for v in stored])
        gl, gp = g.locate_raw(req)
        gv, gf = g.reconstruct_raw(req)
        dr = torch.from_numpy(req.view(np.int32)).to(dev)
        dl = torch.zeros(len(req), dtype=torch.int32, device=dev)
        dp = torch.zeros(len(req), dtype=torch.int64, device=dev)
        dv = torch.zeros((len(req), case.qz.d), dtype=torch.float32, device=dev)
        df = torch.zeros(len(req), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        g.locate_device(len(req), dr.data_ptr(), dl.data_ptr(), dp.data_ptr())
        g.reconstruct_device(len(req), dr.data_ptr(), dv.data_ptr(), df.data_ptr())
        g.sync()
        for what, (l_, p_, v_, f_) in {"host": (gl, gp, gv, gf), "device": (dl.cpu().numpy(), dp.cpu().numpy(), dv.cpu().numpy(),
                                                                              df.cpu().numpy().astype(bool))}.items():
            what = "%s entry, %d wanted" % (what, nwant)
            assert np.array_equal(l_[where], el) and np.array_equal(p_[where], ep) and rr.same_bits(v_[where], ev), what
            rest = np.ones(len(req), bool)
            rest[where] = False
            assert f_[where].all() and not f_[rest].any() and (l_[rest] == -1).all() and (p_[rest] == -1).all() and not v_[rest].view(np.uint32).any(), what


def test_two_threads_on_an_index_and_its_view(native):
    case = rr.case_table()["duplicates"]
    g = handle_of(native, case)
    v = g.clone_view()
    reqs = [case.requests(1000, seed=s) for s in range(4)]
    exp = [(rr.locate(case.st, r), rr.reconstruct(case.st, case.qz, r)) for r in reqs]
    errors = []

    def run(h, first):
        try:
            for rep in range(6):
                k = (first + rep) % 4
                gl, gp = h.locate_raw(reqs[k])
                gv, gf = h.reconstruct_raw(reqs[k])
                (el, ep), (ev, ef) = exp[k]
                assert np.array_equal(gl, el) and np.array_equal(gp, ep) and np.array_equal(gf, ef) and rr.same_bits(gv, ev), (first, rep)
        except Exception as e:                                  # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    ts = [threading.Thread(target=run, args=(g, 0)), threading.Thread(target=run, args=(v, 2))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[0]


def test_pop_and_popfirst_loop_on_the_rewired_path(native):
    """the pop / popfirst sequence of test_delete_pop_pushfirst_in_place_on_device: every popped vector is the model's reconstruction
    of the id the reference pops, bit for bit, and the lists afterwards are the literal model's"""
    from test_gpu_parity import _RefModel
    oidx, data = helpers.build_index(610, 900, 24, 13, 8, 256)
    g = native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)
    model = _RefModel(oidx.offsets, oidx.codes, oidx.ids)
    qz = rr.Quantizers(oidx.centroids, oidx.codebooks, oidx.labels)
    rng = np.random.default_rng(610)
    pts = rng.integers(1, 901, 57).tolist() + [1, 900, 900, 5000]
    native.delete_from_index(g, pts)
    model.delete(pts)
    for step in range(6):
        first = step % 2 == 0
        vecid = 0 if first else model.n() - 1
        exp, found = rr.reconstruct(rr.Stored.from_lists(*model.arrays(8)), qz, [vecid])
        assert found[0]
        rec = native.popfirst(g) if first else native.pop(g)
        assert rec.shape == (24,) and rec.dtype == np.float32 and rr.same_bits(rec, exp[0]), "pop %d" % step
        model.pop(first)
        off, codes, ids = g._lists()
        moff, mcodes, mids = model.arrays(8)
        assert np.array_equal(off, moff) and np.array_equal(ids, mids) and np.array_equal(codes, mcodes), "lists after pop %d" % step
        check(g, rr.Stored.from_lists(moff, mcodes, mids), qz, mids[::50], "device copy after pop %d" % step)
    p = (data[3] + np.float32(0.01)).astype(np.float32)
    native.pushfirst(g, p)
    cl, code = oidx.encode(p)
    model.push(int(cl[0]), code[0], True)
    exp, _ = rr.reconstruct(rr.Stored.from_lists(*model.arrays(8)), qz, [0])
    assert rr.same_bits(native.popfirst(g), exp[0]), "the point just pushed first comes back as its quantization"
    native.delete_from_index(g, list(range(1, len(g) + 1)))
    with pytest.raises(AssertionError, match="empty index"):
        native.pop(g)
