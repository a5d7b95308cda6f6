"""Subset views on the device (ivfadc_clone_subset; csrc/subset.hip.h): a view whose own lists hold the entries a bitmap over stored ids
selects, in stored order, with stored ids.

The model is tests/subset.py (filtered_lists); tests/test_subset_model.py shows on the CPU that the exhaustive read-back used here tells
every wrong compaction of subset.MUTANTS from the right one.  A subset view is compared, bit for bit, with the reference over the
filtered lists AND with a fresh handle that was given the filtered lists through set_lists: by construction the two handles run the
same kernels on lists that differ only in where they lie."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import helpers
import subset as sb
import u16_ref
import write_path as wp
from oracle import oracle as ora
from test_gpu_bitwise import FORMS as FORMS_BITWISE
from test_gpu_sequences import forms_8bit

pytestmark = pytest.mark.gpu
ERR_STATE = 4
NAMING = ("last_qg", "last_striped", "last_nf", "last_lb", "last_chunk", "last_scan_lds")     # what get_stats() says about the form that ran


def same(got, exp, what, u16=False):
    if u16:
        u16_ref.assert_exact(got, exp, what)
    else:
        helpers.assert_same_results(got, exp, what=what)


def refuses(call, code=ERR_STATE, match=None):
    from ivfadc_jl_amd import _native as nat
    with pytest.raises(nat.IVFADCError, match=match) as e:
        call()
    assert e.value.code == code, e.value


def with_lists(ref, lists):
    return wp.ref_with_lists(ref, *lists)


def random_mask(ref, p, seed):
    """a boolean mask over ids 0 .. max id, each set with probability p"""
    return np.random.default_rng(seed).random(int(ref.ids.max()) + 1) < p


# ---- 1. read-back at the edges -------------------------------------------------------------------------------------------------------
_PARENTS = {}


def parent_of(native, stride):
    if stride not in _PARENTS:
        _PARENTS[stride] = wp.gpu_handle(native, sb.case(stride).ref)
    return _PARENTS[stride]


@pytest.mark.parametrize("nbits_kind", sb.NBITS)
@pytest.mark.parametrize("mask_kind", sb.MASKS)
@pytest.mark.parametrize("stride", list(sb.STRIDES))
def test_read_back_at_the_edges(native, stride, mask_kind, nbits_kind):
    """The case table: one list per length around a wave's round, a workgroup and the work item, every mask, nbits above every id and
    in the middle of them, every code stride.  w = kc, K = kept + 7: every kept entry comes back with its id and distance bits."""
    t0 = time.time()
    c = sb.case(stride)
    g = parent_of(native, stride)
    mask, nbits = c.mask(mask_kind, nbits_kind)
    model = sb.filtered_lists(*c.lists(), mask)
    kept = int(model[0][-1])
    v = g.subset(mask=mask)
    what = "%s / %s / %s" % (stride, mask_kind, nbits_kind)
    assert v._subset_n == kept and len(v) == kept and v.size == (c.ref.d, kept), what
    assert np.array_equal(v.list_sizes(), np.diff(model[0])), what
    assert "Subset view" in repr(v) and ("%d Float32 vectors" % kept) in repr(v)
    assert len(g) == int(c.ref.offsets[-1]), "the index itself is untouched"
    K = kept + 7
    got = v.search_raw(c.qs, K, c.ref.kc)
    assert (got[2] == kept).all(), "%s: counts %s, kept %d" % (what, got[2], kept)
    same(got, c.exhaustive(model, K), what + ": the reference over the filtered lists", c.u16)
    if not c.u16 and K <= 1024:                           # (the C oracle's insertion is quadratic in K: the small cases only)
        same(got, with_lists(c.ref, model).knn_search(c.qs, K, c.ref.kc), what + ": the C oracle over the filtered lists")
    fresh = wp.gpu_handle(native, with_lists(c.ref, model))
    same(got, fresh.search_raw(c.qs, K, c.ref.kc), what + ": a fresh handle given the filtered lists", c.u16)
    # the same through ids instead of a mask, where that is the same bitmap
    if nbits_kind == "max_plus_1" and mask_kind in ("random_1pct", "first_only", "none"):
        v2 = g.subset(ids=np.nonzero(mask)[0])
        assert len(v2) == kept
        same(v2.search_raw(c.qs, K, c.ref.kc), got, what + ": subset(ids=...)", c.u16)
    print("subset read-back %s: kept %d of %d, %.2f s" % (what, kept, len(g), time.time() - t0))


def test_device_bitmap_entry(native):
    """ivfadc_clone_subset_device: the same view from a bitmap that already lies in device memory."""
    import torch
    from ivfadc_jl_amd import index as ix
    c = sb.case("u8_m10")
    g = parent_of(native, "u8_m10")
    mask, nbits = c.mask("random_half", "half_of_max")
    words, nb = ix.pack_bitmap(mask=mask)
    dbits = torch.from_numpy(words.view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    v = g.subset_device(dbits.data_ptr(), nb)
    model = sb.filtered_lists(*c.lists(), mask)
    assert len(v) == int(model[0][-1]) and np.array_equal(v.list_sizes(), np.diff(model[0]))
    K = len(v) + 7
    same(v.search_raw(c.qs, K, c.ref.kc), g.subset(mask=mask).search_raw(c.qs, K, c.ref.kc), "device bitmap against host bitmap")
    same(v.search_raw(c.qs, K, c.ref.kc), c.exhaustive(model, K), "device bitmap against the reference")


# ---- 2. every scan form ----------------------------------------------------------------------------------------------------------------
def _f(name, qg, chunk=0, table=0, prune=1, K=None, nq=None, u16_tables=None, **expect):
    return dict(name=name, qg=qg, chunk=chunk, table=table, prune=prune, K=K, nq=nq, u16_tables=u16_tables, expect=expect)


def forms_of(shape):
    """The form-forcing settings of tests/test_gpu_bitwise.py (FORMS) for the BITWISE_SHAPES, the wide-pool and m = 16 eight-wave forms
    of tests/test_gpu_sequences.py (forms_8bit), the four UInt16 forms, and the generic path at K = 2500 for every shape."""
    out = []
    if shape in FORMS_BITWISE:
        for name, f in FORMS_BITWISE[shape].items():
            out.append(_f(name, f["qg"], f["chunk"], f["table"] or 0, 1 if f["prune"] is None else f["prune"], **f["expect"]))
    if shape in ("m8", "m16_d128"):
        m, dsub = (8, 16) if shape == "m8" else (16, 8)
        for f in forms_8bit(m, dsub):
            wanted = ("wide pool" in f["name"] or shape == "m16_d128") and not f["parts"] and f["nq"] is None
            if wanted:
                out.append(_f(f["name"], f["qg"], f["chunk"], f["table"], f["prune"], K=f["K"], **f["expect"]))
    if shape == "kc2048":                               # (m = 8, dsub = 8; half of 30 000 points in 2048 lists: most lists a handful, many empty)
        out += [_f("query-major", -1, last_qg=0), _f("query-major, stand-alone top-w", -3, last_qg=0), _f("generic (forced)", -2, last_qg=-2)]
        out += [_f("list-major qg=%d reference tables" % qg, qg, 1024, table=1, last_qg=qg) for qg in (1, 2, 4)]
    if shape == "u16":
        out += [
            _f("u16 tables, register selectors", 0, table=0, K=10, u16_tables=0, qg_min=1, not_striped=(6, 7)),
            _f("u16 tables, LDS selectors", 0, table=10, K=100, u16_tables=0, qg_min=1, not_striped=(6, 7)),
            _f("u16 table-free, register selectors", 0, table=0, K=10, u16_tables=1, qg_min=1, last_striped=6),
            _f("u16 table-free, LDS selectors", 0, table=10, K=100, u16_tables=1, qg_min=1, last_striped=7),
        ]
    out.append(_f("generic path by K", 0, K=2500, nq=8, u16_tables=0 if shape == "u16" else None, last_qg=-2))
    return out


SHAPES = dict(helpers.BITWISE_SHAPES)
SHAPES["m16_d128"] = (9106, 30000, 128, 14, 16, 256, 10, 3)
SHAPES["u16"] = (4242, 40000, 32, 4, 4, 1024, 10, 3)


def apply_form(g, f):
    g.set_tuning(f["qg"], f["chunk"])
    g.set_table_mode(f["table"])
    g.set_pruning(f["prune"])
    if f["u16_tables"] is not None:
        g.set_u16_tables(f["u16_tables"])
    g.reset_stats()


def check_form(st, f, what):
    for key, val in f["expect"].items():
        if key == "lb":
            assert st["lb_survivors"] > 0, (what, st)
        elif key == "qg_min":
            assert st["last_qg"] >= val, "%s ran as last_qg = %d (%s)" % (what, st["last_qg"], st)
        elif key == "not_striped":
            assert st["last_striped"] not in val, "%s ran as last_striped = %d (%s)" % (what, st["last_striped"], st)
        elif key == "lds_max":
            assert st["last_scan_lds"] <= val, (what, st)
        else:
            assert st[key] == val, "%s did not run as the form it names: %s = %s, expected %s (%s)" % (what, key, st[key], val, st)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_scan_form_serves_a_subset_view(native, shape):
    """A p = 0.5 subset of each shape under every form-forcing setting: the view, a fresh handle given the filtered lists and the
    reference return the same bytes, and the two handles name the same form (get_stats()).  The settings are applied to the view itself."""
    t0 = time.time()
    seed, n, d, kc, m, ksub, K0, w = SHAPES[shape]
    u16 = shape == "u16"
    if u16:
        ref = u16_ref.make_index(seed, n, d, kc, m, ksub, perm_labels=True, ndistinct=5000)
    else:
        ref, _ = helpers.build_index(seed, n, d, kc, m, ksub, label_perm=(shape == "m10"), mode="random")
    qs = np.random.default_rng(seed + 5).random((64, d), dtype=np.float32)
    mask = random_mask(ref, 0.5, seed + 6)
    model = sb.filtered_lists(ref.offsets, ref.codes, ref.ids, mask)
    fref = with_lists(ref, model)
    g = wp.gpu_handle(native, ref)
    v = g.subset(mask=mask)
    fresh = wp.gpu_handle(native, fref)
    assert len(v) == len(fresh) == int(model[0][-1]) and 0.45 * n < len(v) < 0.55 * n
    cache = {}
    for f in forms_of(shape):
        K, nq = f["K"] or K0, f["nq"] or (32 if u16 else 64)
        if (K, nq) not in cache:
            cache[(K, nq)] = u16_ref.knn(fref, qs[:nq], K, w) if u16 else fref.knn_search(qs[:nq], K, w, nthreads=ora.max_threads())
        what = "%s / %s" % (shape, f["name"])
        res, stats = [], []
        for h in (v, fresh):
            apply_form(h, f)
            res.append(h.search_raw(qs[:nq], K, w))
            stats.append(h.get_stats())
        check_form(stats[0], f, what + " (subset view)")
        check_form(stats[1], f, what + " (fresh handle)")
        assert all(stats[0][k] == stats[1][k] for k in NAMING), "%s: the view ran %s, the fresh handle %s" % (
            what, {k: stats[0][k] for k in NAMING}, {k: stats[1][k] for k in NAMING})
        same(res[0], cache[(K, nq)], what + ": subset view against the reference", u16)
        same(res[0], res[1], what + ": subset view against the fresh handle", u16)
    # the index's own settings were never touched, and it still answers for ALL its points
    assert g.get_stats()["queries"] == 0
    exp = u16_ref.knn(ref, qs[:8], K0, w) if u16 else ref.knn_search(qs[:8], K0, w)
    same(g.search_raw(qs[:8], K0, w), exp, shape + ": the index after its subset was searched", u16)
    print("subset forms %s: %d forms, %.2f s" % (shape, len(forms_of(shape)), time.time() - t0))


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (10, 64, 100))
def test_ties_come_out_in_the_filtered_visit_order(native, K):
    """Four distinct code rows: thousands of exact ties per list, so the ids returned ARE the order of the kept entries."""
    ref, _ = helpers.build_index(7711, 30000, 64, 16, 8, 256, mode="random", ndistinct=4)
    qs = np.random.default_rng(7712).random((32, 64), dtype=np.float32)
    mask = random_mask(ref, 0.5, 7713)
    fref = with_lists(ref, sb.filtered_lists(ref.offsets, ref.codes, ref.ids, mask))
    v = wp.gpu_handle(native, ref).subset(mask=mask)
    exp = fref.knn_search(qs, K, 4, nthreads=ora.max_threads())
    assert all(len(set(exp[1][r, :K].tolist())) < K for r in range(4)), "the shape must produce ties inside the top K"
    for plan in (0, -1, 4, -2):
        v.set_tuning(plan, 0)
        same(v.search_raw(qs, K, 4), exp, "ties, K = %d, plan %d" % (K, plan))
    assert all(mask[exp[0][r, :exp[2][r]]].all() for r in range(32)), "only selected ids come back"


# ---- 4. synthetic lists: the parent itself is the second oracle --------------------------------------------------------------------------
def test_subset_of_device_synthesised_lists(native):
    """The index has no host mirror and no id array (the id is the position).  Its own exhaustive read-back with the unselected rows
    removed, in order, is what the subset's read-back must be: no model of the lists is involved."""
    C_ = sb.chunk()
    cent, cbs, labels = helpers.make_quantizers(6100, 32, 16, 8, 256)
    sizes = np.array([0, 1, 63, 65, 257, C_ - 1, C_, C_ + 1, 2 * C_ + 1, 300, 5, 0, 777, 1500, 64, 256], np.int64)
    offsets = np.zeros(17, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    n = int(offsets[-1])
    g = native.IVFADCIndex.from_arrays(cent, cbs, labels)
    g.synth_lists(offsets, 99)
    qs = np.random.default_rng(6101).random((2, 32), dtype=np.float32)
    all_i, all_d, all_c = g.search_raw(qs, n, 16)
    assert (all_c == n).all() and sorted(all_i[0].tolist()) == list(range(n))
    for p, seed in ((0.5, 1), (0.01, 2), (1.0, 3)):
        mask = np.random.default_rng(seed).random(n) < p
        v = g.subset(mask=mask)
        kept = int(mask.sum())
        assert len(v) == kept and np.array_equal(v.list_sizes(), [int(mask[offsets[l]:offsets[l + 1]].sum()) for l in range(16)])
        got = v.search_raw(qs, kept + 7, 16)
        assert (got[2] == kept).all()
        for r in range(2):
            sel = mask[all_i[r]]
            assert np.array_equal(got[0][r, :kept], all_i[r][sel]), "p = %s, query %d: ids" % (p, r)
            assert np.array_equal(got[1][r, :kept].view(np.uint32), all_d[r][sel].view(np.uint32)), "p = %s, query %d: distance bits" % (p, r)
    refuses(lambda: g.subset(mask=mask)._lists())


# ---- 5. life cycle ------------------------------------------------------------------------------------------------------------------------
def test_life_cycle(native, tmp_path):
    import ivfadc_jl_amd as pkg
    from ivfadc_jl_amd import _native as nat
    ref, data = helpers.build_index(3300, 6000, 32, 12, 8, 256, mode="encode")
    qs = np.random.default_rng(3301).random((40, 32), dtype=np.float32)
    mask = random_mask(ref, 0.5, 3302)
    exp = with_lists(ref, sb.filtered_lists(ref.offsets, ref.codes, ref.ids, mask)).knn_search(qs, 10, 4)

    def pair():
        g = wp.gpu_handle(native, ref)
        v = g.subset(mask=mask)
        same(v.search_raw(qs, 10, 4), exp, "fresh subset")
        return g, v

    # every mutator of the index makes the view refuse
    mutators = {
        "append": lambda g: g._append(data[:3], np.arange(3, dtype=np.uint32) + 900000),
        "delete_ids": lambda g: g._delete_ids(np.array([int(ref.ids[0])], np.uint32)),
        "shift_ids": lambda g: g._shift_ids(1),
        "set_lists": lambda g: g.set_lists(ref.offsets, ref.codes, ref.ids),
    }
    for name, mutate in mutators.items():
        g, v = pair()
        mutate(g)
        refuses(lambda: v.search_raw(qs[:4], 10, 4), match="changed since this view")
        refuses(lambda: v.coarse_search_raw(qs[:4], 2), match="changed since this view")
        if name == "set_lists":          # (the same lists again: a new subset is the old one)
            same(g.subset(mask=mask).search_raw(qs, 10, 4), exp, "a new subset after set_lists")
    # a mutator call that changes nothing leaves it valid
    g, v = pair()
    assert g._delete_ids(np.array([4_000_000], np.uint32)) == 0
    same(v.search_raw(qs, 10, 4), exp, "after a delete of an unknown id")
    # read-only: no mutator, no mirror, no save; no subset or view of a view
    blocked = {
        "append": lambda: v._append(data[:3], np.arange(3, dtype=np.uint32) + 900000),
        "delete_ids": lambda: v._delete_ids(np.array([1], np.uint32)),
        "shift_ids": lambda: v._shift_ids(1),
        "set_lists": lambda: v.set_lists(ref.offsets, ref.codes, ref.ids),
        "get_lists": lambda: v._lists(),
        "save": lambda: pkg.save_ivfadc_index(str(tmp_path / "subset.ivfadc"), v),
        "subset of a subset": lambda: v.subset(mask=mask),
        "view of a subset": lambda: v.clone_view(),
        "subset of a view": lambda: g.clone_view().subset(mask=mask),
    }
    for name, call in blocked.items():
        refuses(call)
    same(v.search_raw(qs, 10, 4), exp, "after the refused calls")
    # a handle that was never given lists is an empty index (ivfadc_create leaves it so), and so is any subset of it
    none = wp.gpu_handle(native, ref, with_lists=False).subset(mask=mask)
    assert len(none) == 0 and not none.search_raw(qs[:5], 10, 4)[2].any()
    # the other entries a view serves: coarse search, preassigned probes, a run of batches; a list partition comes along
    lists, dists = v.coarse_search_raw(qs, 4)
    same(v.search_preassigned_raw(qs, 10, lists, dists), exp, "preassigned probes on a subset view")
    parts = v.search_batches_raw([qs[:7], qs[7:30], qs[30:]], 10, 4)
    same(tuple(np.concatenate([p[i] for p in parts]) for i in range(3)), exp, "a run of batches on a subset view")
    # a plain view and a subset view of one index, searched alternately, return what each returns alone
    pv = g.clone_view()
    full = ref.knn_search(qs, 10, 4)
    for _ in range(3):
        same(pv.search_raw(qs, 10, 4), full, "plain view, alternating")
        same(v.search_raw(qs, 10, 4), exp, "subset view, alternating")
        same(g.search_raw(qs, 10, 4), full, "the index, alternating")
    # the empty subset is a valid index
    for empty in (g.subset(ids=np.zeros(0, np.int64)), g.subset(mask=np.zeros(5000, bool)), g.subset(ids=[4_000_000])):
        assert len(empty) == 0 and not empty.list_sizes().any()
        assert not empty.search_raw(qs, 10, 4)[2].any() and not empty.search_raw(qs[:3], 70, 12)[2].any()
    # destroying the index first makes the view refuse; the view is destroyed afterwards
    g.__del__()
    refuses(lambda: v.search_raw(qs[:4], 10, 4), match="destroyed")
    refuses(lambda: pv.search_raw(qs[:4], 10, 4), match="destroyed")
    del v, pv


def test_subset_carries_the_list_partition(native):
    """A list partition set on the index is copied to its subset, like every setting: the partial keys of each part are numpy's over the
    filtered lists."""
    import torch
    ref, _ = helpers.build_index(3400, 20000, 128, 14, 8, 256, mode="random")
    qs = np.random.default_rng(3401).random((12, 128), dtype=np.float32)
    mask = random_mask(ref, 0.5, 3402)
    fref = with_lists(ref, sb.filtered_lists(ref.offsets, ref.codes, ref.ids, mask))
    g = wp.gpu_handle(native, ref)
    dev = torch.device("cuda:0")
    qd = torch.from_numpy(qs).to(dev)
    for part in range(2):
        g.set_list_partition(2, part)
        v = g.subset(mask=mask)
        keys = torch.zeros((12, 10), dtype=torch.int64, device=dev)
        cnts = torch.zeros(12, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        v.search_device_partial(12, qd.data_ptr(), 10, 3, keys.data_ptr(), cnts.data_ptr())
        v.sync()
        rk, rc, _ = helpers.numpy_partial_keys(fref, qs, 10, 3, 2, part)
        gk, gc = keys.cpu().numpy().view(np.uint64), cnts.cpu().numpy()
        assert np.array_equal(gc, rc) and all(np.array_equal(gk[r, :rc[r]], rk[r, :rc[r]]) for r in range(12)), "part %d" % part


# ---- 6. no leak ---------------------------------------------------------------------------------------------------------------------------
def test_create_search_destroy_leaks_nothing(native):
    """50 create / search / destroy cycles of a p = 0.5 subset of a 40 000-point index: the device's free memory does not fall by more
    than ONE subset's own allocation -- the bound is what ivfadc_clone_subset allocates for the view, not a measurement:
    codes (every list's kept * cs rounded up to 256 B, plus the 64 KB CODE_SLACK tail) + ids (4 B each) + the three list tables
    (kc * (8 + 4 + 8) B, grown by a quarter as every table is)."""
    import torch
    seed, n, d, kc, m, ksub, K, w = helpers.BITWISE_SHAPES["m8"]
    ref, _ = helpers.build_index(seed, n, d, kc, m, ksub, mode="random")
    qs = np.random.default_rng(1).random((64, d), dtype=np.float32)
    mask = random_mask(ref, 0.5, 2)
    model = sb.filtered_lists(ref.offsets, ref.codes, ref.ids, mask)
    cs = 8
    one_subset = int(sum(-(-int(k) * cs // 256) * 256 for k in np.diff(model[0]))) + (64 << 10) + 4 * int(model[0][-1]) + (kc * 20 * 5) // 4
    g = wp.gpu_handle(native, ref)
    exp = with_lists(ref, model).knn_search(qs, K, w)

    def cycle():
        v = g.subset(mask=mask)
        same(v.search_raw(qs, K, w), exp, "cycle")
        v.__del__()

    for _ in range(2):                   # what the first creation and the first search set up once per process stays: not a leak
        cycle()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(50):
        cycle()
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    print("free memory before %d, after %d (fell by %d); one subset allocates %d" % (before, after, before - after, one_subset))
    assert before - after <= one_subset, "free device memory fell by %d B over 50 cycles; one subset is %d B" % (before - after, one_subset)


# ---- 7. two in flight -----------------------------------------------------------------------------------------------------------------------
def test_index_and_subset_search_from_two_threads(native):
    seed, n, d, kc, m, ksub, K, w = helpers.BITWISE_SHAPES["m8"]
    ref, _ = helpers.build_index(seed, n, d, kc, m, ksub, mode="random")
    rng = np.random.default_rng(11)
    qa, qb = rng.random((700, d), dtype=np.float32), rng.random((900, d), dtype=np.float32)
    mask = random_mask(ref, 0.5, 12)
    g = wp.gpu_handle(native, ref)
    v = g.subset(mask=mask)
    serial = (g.search_raw(qa, K, w), v.search_raw(qb, K, w))
    same(serial[0], ref.knn_search(qa, K, w, nthreads=ora.max_threads()), "the index, serial")
    same(serial[1], with_lists(ref, sb.filtered_lists(ref.offsets, ref.codes, ref.ids, mask)).knn_search(qb, K, w, nthreads=ora.max_threads()),
         "the subset view, serial")
    out, err = {}, []

    def run(name, h, q):
        try:
            out[name] = [h.search_raw(q, K, w) for _ in range(4)]
        except Exception as e:          # noqa: BLE001 -- reported by the main thread
            err.append((name, e))

    ts = [threading.Thread(target=run, args=("index", g, qa)), threading.Thread(target=run, args=("subset", v, qb))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not err, err
    for r in out["index"]:
        same(r, serial[0], "the index beside its subset view")
    for r in out["subset"]:
        same(r, serial[1], "the subset view beside its index")
