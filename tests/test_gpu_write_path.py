"""The device write path at its edges: ivfadc_encode, ivfadc_append, ivfadc_delete_ids, ivfadc_shift_ids (encode_kernel,
argmin_rows_kernel, append_scatter_kernel, delete_compact_kernel, shift_ids_kernel) against the CPU oracle and a model of the lists.

Every comparison is exact.  The expected lists come from the oracle's encoder and from the restatements of utils.jl in
tests/write_path.py (shown equal to the literal _RefModel in tests/test_write_path_model.py), never from the library's host mirror;
the device copy is observed whole, through write_path.assert_device_equals (w = kc, K = len(index): every stored point comes back
with its id and its distance bits).  The mirror (g._lists()) is compared with the model as well."""
import time

import numpy as np
import pytest

import helpers
import write_path as wp
from oracle import oracle as ora

pytestmark = pytest.mark.gpu
f32 = np.float32

PAIRS = ((3, 200), (63, 64), (0, 255), (127, 128))      # same wave, across a wave boundary, first and last wave, middle boundary


def _empty_oracle(cent, cbs, labels):
    kc, m = cent.shape[0], cbs.shape[0]
    return ora.OracleIndex(cent, cbs, labels, np.zeros(kc + 1, np.int64), np.zeros((0, m), np.uint8), np.zeros(0, np.uint32))


def _same_lists(got, exp, what):
    for name, a, b in zip(("offsets", "codes", "ids"), got, exp):
        assert np.array_equal(a, b), "%s: %s of the host mirror differ from the model" % (what, name)


def _encode_case(native, cent, cbs, labels, pts, qs, what, plans=(-2, 0), seed=0):
    """encode == the oracle's encode; then _append, and the device copy == np_append of the ORACLE's codes.  Returns the handle, the
    oracle's (lists, codes) and the reference index over the model lists."""
    empty = _empty_oracle(cent, cbs, labels)
    g = wp.gpu_handle(native, empty, with_lists=False)
    pts = np.ascontiguousarray(pts, f32)
    n = pts.shape[0]
    gl, gc = g.encode(pts)
    ol, oc = empty.encode(pts) if n else (np.zeros(0, np.int32), np.zeros((0, empty.m), np.uint8))
    assert np.array_equal(gl, ol), "%s: lists differ at points %s: %s vs %s" % (what, np.nonzero(gl != ol)[0][:8], gl[gl != ol][:8], ol[gl != ol][:8])
    assert np.array_equal(gc, oc), "%s: codes differ at (point, sub-space) %s" % (what, np.argwhere(gc != oc)[:8].tolist())
    ids = (np.random.default_rng(seed).permutation(n) + 11).astype(np.uint32)
    g._append(pts, ids)
    model = wp.np_append(*wp.lists_of(empty), ol, oc, ids)
    ref = wp.ref_with_lists(empty, *model)
    wp.assert_device_equals(g, ref, qs, what=what, plans=plans)
    _same_lists(g._lists(), model, what)
    return g, ol, oc, ref


def _tie_geometry(seed):
    """d = 32, m = 4, ksub = 256, kc = 16 on a grid of 2^-10 (centroid + codeword and point - centroid are exact), permuted labels."""
    cent, cbs, labels = helpers.make_quantizers(seed, 32, 16, 4, 256, label_perm=True)
    cent = (np.round(cent * 1024) / 1024).astype(f32)
    cbs = (np.round(cbs * 1024) / 1024).astype(f32)
    return cent, cbs, labels


def test_encode_codeword_ties(native):
    """Duplicate codewords at PAIRS in every sub-space; half of the points lie exactly on duplicated codewords of a centroid (distance
    +0 to both copies).  The wave min and the LDS atomicMin of encode_kernel order (distance bits, codeword): the first index wins,
    and only then the (permuted) label map applies."""
    cent, cbs, labels = _tie_geometry(501)
    for lo, hi in PAIRS:
        cbs[:, hi] = cbs[:, lo]
    rng = np.random.default_rng(501)
    n = 256
    pts = rng.random((n, 32), dtype=f32)
    cell = rng.integers(0, 16, n // 2)
    pick = np.array(PAIRS)[rng.integers(0, 4, (n // 2, 4)), rng.integers(0, 2, (n // 2, 4))]     # either copy, per sub-space
    pts[: n // 2] = cent[cell] + cbs[np.arange(4), pick].reshape(n // 2, 32)
    empty = _empty_oracle(cent, cbs, labels)
    ol, oc = empty.encode(pts)
    on_lo = sum(int(np.count_nonzero(oc[: n // 2, i] == labels[i, lo])) for i in range(4) for lo, _ in PAIRS)
    on_hi = sum(int(np.count_nonzero(oc[:, i] == labels[i, hi])) for i in range(4) for _, hi in PAIRS)
    assert on_hi == 0 and on_lo >= n, (on_lo, on_hi)        # the oracle: first index; most of the 4 * n / 2 slices are such ties
    exact = [r for r in range(n // 2) if np.array_equal(pts[r] - cent[ol[r]], cbs[np.arange(4), pick[r]].reshape(32))]
    assert len(exact) >= n // 4                              # ... at distance +0
    qs = (pts[[3, n - 2]] + f32(0.01)).astype(f32)
    _encode_case(native, cent, cbs, labels, pts, qs, "codeword_ties")


def _table(cbs_i, r, how):
    """Distances of one residual slice to every codeword of a sub-space: the reference's order in f32 ("ref"), exact in float64
    ("f64"), one fused multiply-add per step ("fma": the f32 product is exact in float64, one rounding after the add), the
    reference's operations in descending dimension ("rev")."""
    dsub = cbs_i.shape[1]
    if how == "f64":
        return ((cbs_i.astype(np.float64) - r.astype(np.float64)[None, :]) ** 2).sum(1)
    s = np.zeros(cbs_i.shape[0], f32)
    for t in (range(dsub - 1, -1, -1) if how == "rev" else range(dsub)):
        df = cbs_i[:, t] - r[t]
        if how == "fma":
            s = (df.astype(np.float64) * df.astype(np.float64) + s.astype(np.float64)).astype(f32)
        else:
            s = s + df * df
    return s


def test_encode_one_ulp_apart(native):
    """Codeword pairs one ulp apart in two coordinates, and points -- chosen on the CPU out of 6000 candidates -- for which the two
    f32 sums in the reference's order differ by exactly one ulp IN FAVOUR OF THE HIGHER INDEX.  An encoder that contracts
    sum + df * df into a fused multiply-add, or adds the dimensions in another order, or is simply more exact, picks the lower index
    for many of them: counted here against an fma-emulating, a reversed and a float64 restatement, at least 20 points each."""
    cent, cbs, labels = helpers.make_quantizers(502, 32, 16, 4, 256, label_perm=True)
    rng = np.random.default_rng(502)
    for i in range(4):
        for lo, hi in PAIRS:
            cbs[i, hi] = cbs[i, lo]
            for t in rng.choice(8, 2, replace=False):      # two coordinates, one ulp each way: which copy is nearer is a matter of rounding
                cbs[i, hi, t] = np.nextafter(cbs[i, hi, t], f32(rng.choice([-2.0, 2.0])))
    ncand = 6000
    cell = rng.integers(0, 16, ncand)
    pick = np.array(PAIRS)[rng.integers(0, 4, (ncand, 4)), 0]
    cand = (cent[cell] + cbs[np.arange(4), pick].reshape(ncand, 32) + f32(0.04) * rng.standard_normal((ncand, 32))).astype(f32)
    empty = _empty_oracle(cent, cbs, labels)
    ol, oc = empty.encode(cand)
    chosen, votes = [], {"f64": 0, "fma": 0, "rev": 0}
    for r in range(ncand):
        res = cand[r] - cent[ol[r]]
        hit = False
        for i in range(4):
            lo, hi = next(p for p in PAIRS if p[0] == pick[r, i])
            sl = res[i * 8:(i + 1) * 8]
            two = _table(cbs[i, [lo, hi]], sl, "ref")
            if int(two[0].view(np.uint32)) - int(two[1].view(np.uint32)) != 1 or oc[r, i] != labels[i, hi]:
                continue                                     # not one ulp in favour of hi, or another codeword is nearer still
            full = _table(cbs[i], sl, "ref")
            assert int(np.argmin(full)) == hi
            hit = True
            for how in votes:
                votes[how] += int(np.argmin(_table(cbs[i], sl, how))) != hi
        if hit:
            chosen.append(r)
    assert len(chosen) >= 40 and min(votes.values()) >= 20, (len(chosen), votes)
    pts = np.concatenate([cand[chosen[:300]], rng.random((20, 32), dtype=f32)])
    _encode_case(native, cent, cbs, labels, pts, (pts[[0, 7]] + f32(0.01)).astype(f32), "one_ulp_apart")


@pytest.mark.parametrize("d,m,ksub,kc,n", [(6, 2, 2, 1, 150), (50, 10, 16, 13, 150), (12, 4, 255, 130, 300), (8, 8, 256, 1, 150),
                                           (768, 48, 256, 13, 60), (4088, 1, 256, 130, 40)])
def test_encode_small_and_odd(native, d, m, ksub, kc, n):
    """The c < ksub mask at ksub = 2 / 16 / 255, dsub = 1 / 5 / 16 / 4088 (a 16 KB residual in LDS), one wave's worth and 48 waves'
    worth of sub-spaces, kc = 1 (argmin over one column), 13 and 130 (lanes with 2 and 3 strides)."""
    cent, cbs, labels = helpers.make_quantizers(510 + m, d, kc, m, ksub, label_perm=True)
    rng = np.random.default_rng(d)
    pts = rng.random((n, d), dtype=f32)
    cw = rng.integers(0, ksub, (n // 2, m))
    pts[: n // 2] = cent[rng.integers(0, kc, n // 2)] + cbs[np.arange(m), cw].reshape(n // 2, d)      # half next to a codeword
    _, ol, oc, _ = _encode_case(native, cent, cbs, labels, pts, rng.random((2, d), dtype=f32), "small_and_odd d=%d m=%d ksub=%d kc=%d" % (d, m, ksub, kc))
    assert all(np.isin(oc[:, i], labels[i]).all() for i in range(m))


def test_encode_centroid_ties(native):
    """Identical centroid rows at (1, 65) -- the same lane on two strides of argmin_rows_kernel --, (3, 64), (0, 129), (63, 128);
    points lie on and next to them.  The lower cell wins, in the encoder and in the coarse search of the read-back."""
    kc, d = 130, 8
    cent, cbs, labels = helpers.make_quantizers(503, d, kc, 4, 256, label_perm=True)
    dup = ((1, 65), (3, 64), (0, 129), (63, 128))
    for lo, hi in dup:
        cent[hi] = cent[lo]
    rng = np.random.default_rng(503)
    n = 320
    pts = rng.random((n, d), dtype=f32)
    lo_cells = np.array([lo for lo, _ in dup])
    pts[:40] = cent[lo_cells[np.arange(40) % 4]]                                                        # exactly on them: distance +0 twice
    pts[40:160] = cent[lo_cells[np.arange(120) % 4]] + f32(0.01) * rng.standard_normal((120, d)).astype(f32)
    _, ol, _, _ = _encode_case(native, cent, cbs, labels, pts, pts[[0, 41]].copy(), "centroid_ties")
    assert not np.isin(ol, [hi for _, hi in dup]).any()
    assert all(np.count_nonzero(ol[:160] == lo) >= 30 for lo in lo_cells)


def sum_sq(a, b):
    """sum_t (a_t - b_t)^2 over the last axis in the reference's order: ascending t, f32, one rounding per operation."""
    s = np.zeros(np.broadcast_shapes(a.shape, b.shape)[:-1], f32)
    for t in range(a.shape[-1]):
        df = a[..., t] - b[..., t]
        s = s + df * df
    return s


def _nearest_cell(cent, pts):
    """First minimum of the reference's f32 coarse sums (ascending dimension, one rounding per operation) for every point, eight
    points at a time so that the kc-wide rows stay in cache."""
    ct = np.ascontiguousarray(cent.T)
    out = np.zeros(pts.shape[0], np.int32)
    for s0 in range(0, pts.shape[0], 8):
        p = pts[s0:s0 + 8]
        acc = np.zeros((p.shape[0], cent.shape[0]), f32)
        df = np.empty_like(acc)
        for t in range(cent.shape[1]):
            np.subtract(ct[t][None, :], p[:, t][:, None], out=df)
            np.multiply(df, df, out=df)
            np.add(acc, df, out=acc)
        out[s0:s0 + 8] = np.argmin(acc, axis=1)
    return out


def test_encode_large_kc_batch_cut(native):
    """kc = 65536: encode_dev cuts the batch at 2^30 / (4 kc) = 4096 points, so 4100 points are two batches of 4096 and 4, and the b0
    offsets of the points, the lists and the codes all matter.  The coarse distances must be the exact kernel's (a search on this
    handle would use the matrix-core filter): 48 centroids have a twin one ulp away in one coordinate, and points sit on either."""
    kc, d, m, ksub, n = 65536, 4, 2, 16, 4100
    assert (1 << 30) // (4 * kc) == 4096
    cent, cbs, labels = helpers.make_quantizers(504, d, kc, m, ksub, label_perm=True, scale=0.01)
    rng = np.random.default_rng(504)
    twins = rng.choice(kc, 96, replace=False).reshape(48, 2)
    for a, b in twins:
        cent[b] = cent[a]
        t = int(rng.integers(0, d))
        cent[b, t] = np.nextafter(cent[a, t], f32(2.0))
    pts = rng.random((n, d), dtype=f32)
    where = np.concatenate([rng.choice(4096, 188, replace=False), np.arange(4096, 4100)])            # the second batch is all twins
    pts[where] = cent[twins[np.arange(192) % 48, (np.arange(192) // 48) % 2]]
    pts[where[96:]] += (f32(1e-6) * rng.standard_normal((96, d))).astype(f32)
    # the oracle's encoder sorts all kc distances for every point (minutes at this kc): the expected lists and codes are its sums
    # restated in numpy -- ascending dimension, one rounding per operation, first minimum -- and the oracle itself confirms a sample
    ol = _nearest_cell(cent, pts)
    res = pts - cent[ol]
    oc = np.stack([labels[i][np.argmin(sum_sq(cbs[i][None, :, :], res[:, None, i * 2:(i + 1) * 2]), axis=1)] for i in range(m)], 1)
    sample = np.concatenate([where[:12], where[-12:], np.arange(8)])
    sl, sc = _empty_oracle(cent, cbs, labels).encode(pts[sample])
    assert np.array_equal(sl, ol[sample]) and np.array_equal(sc, oc[sample])
    assert np.isin(ol[where], twins).all() and len(np.unique(ol[where])) > 60
    empty = _empty_oracle(cent, cbs, labels)
    g = wp.gpu_handle(native, empty, with_lists=False)
    gl, gc = g.encode(pts)
    assert np.array_equal(gl, ol), "lists differ at points %s" % np.nonzero(gl != ol)[0][:8]
    assert np.array_equal(gc, oc), "codes differ at %s" % np.argwhere(gc != oc)[:8].tolist()
    tl, tc = g.encode(pts[4096:])
    assert np.array_equal(tl, ol[4096:]) and np.array_equal(tc, oc[4096:])                            # as when encoded alone
    ids = (rng.permutation(n) + 11).astype(np.uint32)
    g._append(pts, ids)
    model = wp.np_append(*wp.lists_of(empty), ol, oc, ids)
    wp.assert_device_equals(g, wp.ref_with_lists(empty, *model), pts[[4097, 5]].copy(), what="large_kc_batch_cut", plans=(-2,))
    _same_lists(g._lists(), model, "large_kc_batch_cut")


def test_encode_offset_300(native):
    """A common offset of 300, three ways.  (a) data, centroids and codebooks all + 300, literally: the residuals are of ordinary size
    and every codeword distance is a sum of squares near 300^2 whose last bits decide the minimum.  (b) data and centroids + 300,
    codebooks as they are: point - centroid cancels catastrophically and the codes spread over the codebook.  (c) data + 600,
    centroids and codebooks + 300: the residuals are near 300 as well and cancel against the codewords."""
    cent, cbs, labels = helpers.make_quantizers(505, 32, 16, 4, 256, label_perm=True)
    rng = np.random.default_rng(505)
    base = rng.random((300, 32), dtype=f32)
    q = rng.random((2, 32), dtype=f32)
    off = f32(300.0)
    for name, dp, dc, db in (("a", off, off, off), ("b", off, off, f32(0.0)), ("c", f32(600.0), off, off)):
        _, ol, oc, _ = _encode_case(native, (cent + dc).astype(f32), (cbs + db).astype(f32), labels, (base + dp).astype(f32),
                                    (q + dp).astype(f32), "offset_300 (%s)" % name)
        assert name == "a" or min(len(np.unique(oc[:, i])) for i in range(4)) > 20, name      # (a) and (c) fill few cells, (a) few codes
        assert name != "b" or len(np.unique(ol)) > 8


@pytest.mark.parametrize("n", [0, 1])
def test_encode_n0_n1(native, n):
    cent, cbs, labels = helpers.make_quantizers(506, 12, 5, 3, 64, label_perm=True)
    rng = np.random.default_rng(506)
    pts = rng.random((n, 12), dtype=f32)
    g, _, _, ref = _encode_case(native, cent, cbs, labels, pts, rng.random((2, 12), dtype=f32), "n=%d" % n)
    assert len(g) == n and g.get_stats()["inplace_appends"] == 0
    more = rng.random((3, 12), dtype=f32)                         # ... and the handle goes on from there, in place this time
    ml, mc = ref.encode(more)
    g._append(more, np.array([100, 101, 102], np.uint32))
    assert g.get_stats()["inplace_appends"] == 1
    wp.assert_device_equals(g, wp.ref_with_lists(ref, *wp.np_append(*wp.lists_of(ref), ml, mc, [100, 101, 102])), more[:2], what="n=%d + 3" % n)


def test_encode_non_finite_points_are_contained(native):
    """Containment only: rows with NaN / +Inf / -Inf coordinates get SOME list in [0, kc) and SOME label of each sub-space, the call
    returns OK, the finite rows of the batch encode exactly as without the others, and the handle works normally afterwards.

    Why no index can leave its array (read off the kernels, not tried out): the coarse kernel and both encoder kernels index
    memory by thread, block and loop counters only -- never by a value computed from the data.  argmin_rows_kernel folds keys
    (distance bits << 32) | c with c < kc; whatever the distance bits are (NaN and Inf included) a key's low word is a valid
    cell, and every key is below KEY_MAX because its low word is below 2^32 - 1, so lane 0's first key always replaces the
    initial KEY_MAX (kc >= 1) and out[r] = low word of a real key, in [0, kc).  encode_kernel reads centroids[assign[p]] with that
    cell; its keys are (sum bits << 32) | c for c < ksub, KEY_MAX for the masked lanes c >= ksub; codeword 0 exists in every
    sub-space (ksub >= 1) and its key is below KEY_MAX, so after the wave min and the LDS atomicMin best[i]'s low word is a
    codeword index below ksub, and labels[i * ksub + that] is inside the label table.  Non-finite sums only change WHICH valid key
    is the minimum (NaN bit patterns order above +Inf as integers), which is unspecified here."""
    cent, cbs, labels = helpers.make_quantizers(507, 32, 16, 4, 200, label_perm=True)
    rng = np.random.default_rng(507)
    clean = rng.random((64, 32), dtype=f32)
    pts = clean.copy()
    pts[5] = np.nan
    pts[17, 3] = np.inf
    pts[23, 30] = -np.inf
    pts[41, 8] = np.nan
    bad = np.array([5, 17, 23, 41])
    fine = np.setdiff1d(np.arange(64), bad)
    empty = _empty_oracle(cent, cbs, labels)
    g = wp.gpu_handle(native, empty, with_lists=False)
    gl, gc = g.encode(pts)                                                      # returns OK (a failure raises)
    assert ((gl >= 0) & (gl < 16)).all(), gl[bad]
    assert all(np.isin(gc[:, i], labels[i]).all() for i in range(4)), gc[bad]
    ol, oc = empty.encode(clean)
    assert np.array_equal(gl[fine], ol[fine]) and np.array_equal(gc[fine], oc[fine])
    al, ac = g.encode(pts[fine])
    assert np.array_equal(al, ol[fine]) and np.array_equal(ac, oc[fine])
    # afterwards: encode, append and search as if nothing had happened
    cl, cc = g.encode(clean)
    assert np.array_equal(cl, ol) and np.array_equal(cc, oc)
    ids = np.arange(64, dtype=np.uint32)
    g._append(clean, ids)
    ref = wp.ref_with_lists(empty, *wp.np_append(*wp.lists_of(empty), ol, oc, ids))
    wp.assert_device_equals(g, ref, clean[:2] + f32(0.01), what="after non-finite points")


# ---- delete, append and shift observed exhaustively -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunk_cases():
    """The `chunks` geometry per stride, built once and never changed: name -> (reference index, two queries)."""
    return {s: wp.chunks_case(s) for s in wp.STRIDES}


@pytest.mark.parametrize("pattern", wp.PATTERNS)
@pytest.mark.parametrize("stride", list(wp.STRIDES))
def test_delete_patterns_read_back(native, chunk_cases, stride, pattern):
    """delete_compact_kernel over several chunks per list, with the write cursor lagging the read cursor by up to a whole chunk and
    more, at every code stride (cb == cs, padded cs > cb, one dword, twelve dwords, UInt16 codes): the device copy equals np_delete's
    lists after the deletion, the removed count is the model's."""
    ref, qs = chunk_cases[stride]
    g = wp.gpu_handle(native, ref)
    wp.assert_device_equals(g, ref, qs, what="%s before" % stride)              # a search: the device layout is current from here on
    n = int(ref.offsets[-1])
    if pattern == "absent_and_duplicates":
        view = g.clone_view()
        assert g._delete_ids(wp.absent_ids(n)) == 0                             # nothing stored under these ids: nothing changes,
        helpers.assert_same_results(view.search_raw(qs, 10, 3), wp.ref_knn(ref, qs, 10, 3), what="view after a no-op delete")   # views stay valid
        wp.assert_device_equals(g, ref, qs, what="%s after a no-op delete" % stride)
    dele = wp.pattern_ids(pattern, ref.offsets, ref.ids)
    *model, removed = wp.np_delete(*wp.lists_of(ref), dele)
    assert removed == {"everything": n, "absent_and_duplicates": 3, "whole_list": 1000, "every_other": 1289}.get(pattern, removed)
    assert g._delete_ids(dele) == removed
    wp.assert_device_equals(g, wp.ref_with_lists(ref, *model), qs, what="%s %s" % (stride, pattern))
    _same_lists(g._lists(), model, "%s %s" % (stride, pattern))
    if pattern == "everything":
        assert len(g) == 0


@pytest.mark.parametrize("stride", list(wp.STRIDES))
def test_chained_mutations_read_back(native, chunk_cases, stride):
    """One handle through delete, delete, append into the freed room, append up to exactly the capacity of a list (in place), one
    point more (re-layout), pushfirst! and popfirst!; the whole device copy is read back after every step.  Capacities follow the
    library's rule (write_path.capacity) from the lengths at the last re-layout; the test checks its own preconditions from the model."""
    ref, qs = chunk_cases[stride]
    g = wp.gpu_handle(native, ref)
    state = wp.lists_of(ref)
    short = wp.SHORT_LIST

    def check(what):
        wp.assert_device_equals(g, wp.ref_with_lists(ref, *state), qs, what="%s: %s" % (stride, what))
        _same_lists(g._lists(), state, "%s: %s" % (stride, what))

    def append(pts, ids, inplace, what):
        nonlocal state
        lst, codes = wp.ref_encode(ref, pts)
        before = g.get_stats()["inplace_appends"]
        g._append(pts, np.asarray(ids, np.uint32))
        assert g.get_stats()["inplace_appends"] == before + (1 if inplace else 0), what
        state = wp.np_append(*state, lst, codes, ids)
        check(what)
        return lst

    def points_of_cell(cell, count, seed):
        rng = np.random.default_rng(seed)
        pts = (ref.centroids[cell] + f32(1e-3) * rng.standard_normal((4 * count, ref.d))).astype(f32)
        pts = pts[wp.ref_encode(ref, pts)[0] == cell][:count]
        assert pts.shape[0] == count
        return pts

    check("before")
    cap = wp.capacity(np.diff(state[0]))                                       # laid out by that first search
    assert cap[short] == 33
    for step, pattern in enumerate(("every_other", "boundary_pairs")):       # the second in the numbering the first left
        dele = wp.pattern_ids(pattern, state[0], state[2])
        *state, removed = wp.np_delete(*state, dele)
        assert g._delete_ids(dele) == removed == len(dele)
        check("delete %s" % pattern)
    # into the freed room
    pts, lst, _ = wp.append_batch(ref, 77, 40)
    n = int(state[0][-1])
    assert (np.diff(state[0]) + np.bincount(lst, minlength=ref.kc) <= cap).all()
    append(pts, np.arange(n, n + 40), True, "append into the freed room")
    # exactly to the capacity of the list that began with one point: still in place; one more: a re-layout
    room = int(cap[short] - np.diff(state[0])[short])
    assert 0 < room <= 33
    n = int(state[0][-1])
    append(points_of_cell(short, room, 78), np.arange(n, n + room), True, "fill a list to its capacity")
    assert np.diff(state[0])[short] == cap[short] == 33
    append(points_of_cell(short, 1, 79), [n + room], False, "one point past the capacity")
    assert np.diff(state[0])[short] == 34
    # pushfirst!: every id up by one, then id 0 (the read-back above has laid the lists out again: both edits are in place)
    before = g.get_stats()["inplace_appends"]
    g._shift_ids(1)
    state = wp.np_shift(*state, 1)
    check("shift +1")
    append(points_of_cell(2, 1, 80), [0], True, "append id 0")
    assert g.get_stats()["inplace_appends"] == before + 1
    # popfirst!
    *state, removed = wp.np_delete(*state, [0])
    assert g._delete_ids(np.array([0], np.uint32)) == removed == 1
    check("delete id 0")
    assert sorted(state[2].tolist()) == list(range(len(g)))


def test_grid_stride_shift(native):
    """shift_ids_kernel launches at most 4096 x 256 threads: above 2^20 id slots its grid-stride loop takes a second trip.  950 000
    points in 64 lists are 1 068 7xx slots by the capacity rule.  shift +1, read back whole (one query, K = n) against np_shift's lists;
    then about half of the ids deleted at random (58 chunks per list, the write cursor thousands of slots behind) and read back
    again.  The reference here is helpers.numpy_knn_batch, the sort-based restatement of the oracle: the C oracle's bounded insertion
    is quadratic in K.  Measured on an MI355X: 0.4 s wall for the whole test (printed below, pytest -s)."""
    t0 = time.time()
    kc, d, m, n = 64, 4, 2, 950_000
    oidx, _ = helpers.build_index(520, n, d, kc, m, 256, label_perm=True, mode="random")
    slots = int(wp.capacity(np.diff(oidx.offsets)).sum())
    assert slots > 4096 * 256 and slots - n > kc * 32
    rng = np.random.default_rng(520)
    q = rng.random((1, d), dtype=f32)
    g = wp.gpu_handle(native, oidx)
    assert g.search_raw(q, 10, 4)[2][0] == 10                                   # the device layout is current
    g._shift_ids(1)
    state = wp.np_shift(*wp.lists_of(oidx), 1)
    wp.assert_device_equals(g, wp.ref_with_lists(oidx, *state), q, what="shift across 2^20 slots", plans=(-2,), knn=wp.numpy_exhaustive)
    dele = rng.permutation(n + 1)[: n // 2].astype(np.uint32)                   # id 0 is not stored any more; n is
    *state, removed = wp.np_delete(*state, dele)
    assert g._delete_ids(dele) == removed and n // 2 - 1 <= removed <= n // 2
    wp.assert_device_equals(g, wp.ref_with_lists(oidx, *state), q, what="half deleted", plans=(-2,), knn=wp.numpy_exhaustive)
    print("grid_stride_shift: %.1f s wall, %d slots" % (time.time() - t0, slots))


# ---- both code widths through one chain ---------------------------------------------------------------------------------------------
OK, ERR_STATE = 0, 4
# ivfadc_encode / ivfadc_encode_u16 on a handle of the other width, n = 0 and n = 1 (valid pointers), as the entries have always
# answered: the 8-bit entry returns on n == 0 before it looks at the width, the _u16 entry looks at the width first
CROSS_WIDTH_ENCODE = {("encode", 16, 0): OK, ("encode", 16, 1): ERR_STATE, ("encode_u16", 8, 0): ERR_STATE, ("encode_u16", 8, 1): ERR_STATE}


def test_both_widths_one_chain(native, tmp_path):
    """d = 16, m = 4, ksub = 256, kc = 5, 600 points, list 2 empty.  An 8-bit handle and its 16-bit re-expression (same codewords,
    permuted uint16 labels out of 0 .. 65535) go through set lists, search, append 3 in place, append past a list's capacity, delete
    across three lists with an absent id, shift by 1, save and load.  After every step the two mirrors agree through the label maps
    and equal the numpy model, inplace_appends agree, and a K = 5, w = kc search returns identical bytes from both."""
    import ctypes as C
    from ivfadc_jl_amd import _native as nat
    d, m, kc, n = 16, 4, 5, 600
    cent, cbs, lab8 = helpers.make_quantizers(530, d, kc, m, 256, label_perm=True)
    rng = np.random.default_rng(530)
    lab16 = np.stack([rng.permutation(65536)[:256].astype(np.uint16) for _ in range(m)])
    inv8 = np.zeros((m, 256), np.int64)
    for i in range(m):
        inv8[i, lab8[i]] = np.arange(256)

    def widen(codes8):                                    # 8-bit labels -> codeword indices -> 16-bit labels
        return np.stack([lab16[i][inv8[i][codes8[:, i]]] for i in range(m)], 1).astype(np.uint16).reshape(-1, m)

    sizes = np.array([200, 150, 0, 130, 120])
    offsets = np.zeros(kc + 1, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    codes = np.stack([lab8[i][rng.integers(0, 256, n)] for i in range(m)], 1).astype(np.uint8)
    ref = ora.OracleIndex(cent, cbs, lab8, offsets, codes, rng.permutation(n).astype(np.uint32))
    g8 = native.IVFADCIndex.from_arrays(cent, cbs, lab8)
    g16 = native.IVFADCIndex.from_arrays(cent, cbs, lab16)
    assert g8.code_type == np.uint8 and g16.code_type == np.uint16
    qs = rng.random((6, d), dtype=f32)
    state = wp.lists_of(ref)
    inplace = 0

    def check(what):
        l8, l16 = g8._lists(), g16._lists()
        _same_lists(l8, state, "%s (8-bit)" % what)
        _same_lists(l16, (state[0], widen(state[1]), state[2]), "%s (16-bit)" % what)
        r8, r16 = g8.search_raw(qs, 5, kc), g16.search_raw(qs, 5, kc)
        for a, b in zip(r8, r16):
            assert a.tobytes() == b.tobytes(), what
        helpers.assert_same_results(r8, wp.ref_knn(wp.ref_with_lists(ref, *state), qs, 5, kc), what=what)
        assert g8.get_stats()["inplace_appends"] == g16.get_stats()["inplace_appends"] == inplace, what
        assert len(g8) == len(g16) == int(state[0][-1])

    def append(pts, ids, what):
        nonlocal state
        lst, new = ref.encode(pts)
        g8._append(pts, np.asarray(ids, np.uint32))
        g16._append(pts, np.asarray(ids, np.uint32))
        state = wp.np_append(*state, lst, new, ids)
        check(what)
        return lst

    g8.set_lists(*state)
    g16.set_lists(state[0], widen(state[1]), state[2])
    check("set lists")                                                          # (its search lays the capacity out)
    cap = wp.capacity(np.diff(state[0]))
    pts, lst, _ = wp.append_batch(ref, 531, 3)
    assert (np.diff(state[0]) + np.bincount(lst, minlength=kc) <= cap).all()
    inplace += 1
    append(pts, [n, n + 1, n + 2], "append 3 in place")
    cell2 = (cent[2] + f32(1e-3) * rng.standard_normal((200, d))).astype(f32)
    past = int(cap[2] - np.diff(state[0])[2]) + 1                               # one more than the room the layout left behind list 2
    cell2 = cell2[ref.encode(cell2)[0] == 2][:past]
    assert cap[2] == 32 and 30 <= cell2.shape[0] == past <= 33
    append(cell2, np.arange(n + 3, n + 3 + past), "append past the capacity of the list that was empty")      # no in-place append: a re-layout
    dele = np.concatenate([state[2][[0, 1, int(state[0][1]) + 5, int(state[0][3]) + 7]], [0x7FFFFFF0]]).astype(np.uint32)[::-1]
    *state, removed = wp.np_delete(*state, dele)
    assert removed == 4 and g8._delete_ids(dele) == 4 and g16._delete_ids(dele) == 4
    check("delete across three lists, one id absent")
    g8._shift_ids(1)
    g16._shift_ids(1)
    state = wp.np_shift(*state, 1)
    check("shift by 1")
    f8, f16 = str(tmp_path / "w8.bin"), str(tmp_path / "w16.bin")
    native.save_ivfadc_index(f8, g8)
    native.save_ivfadc_index(f16, g16)
    keep = (g8, g16)
    g8, g16 = native.load_ivfadc_index(f8), native.load_ivfadc_index(f16)
    assert g8.code_type == np.uint8 and g16.code_type == np.uint16
    inplace = 0
    check("save, then load")
    # the entries of the other width
    lib = nat.lib()
    for (entry, bits, npts), want in CROSS_WIDTH_ENCODE.items():
        h = (keep[1] if bits == 16 else keep[0])._h
        p = np.ascontiguousarray(qs[:1])
        out_list, out_codes = np.zeros(1, np.int32), np.zeros(2 * m, np.uint8)
        rc = getattr(lib, "ivfadc_" + entry)(h, npts, nat.ptr(p, C.c_float), nat.ptr(out_list, C.c_int32),
                                              out_codes.ctypes.data_as(C.c_void_p if entry.endswith("_u16") else C.POINTER(C.c_uint8)))
        print("cross-width %s on a %d-bit handle, n = %d: %d" % (entry, bits, npts, rc))
        assert rc == want, (entry, bits, npts, rc)
