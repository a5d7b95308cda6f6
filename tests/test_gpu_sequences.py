"""Search SEQUENCES on one handle: every scan form behind every other, and steered random sequences.

A handle keeps state from one search to the next (the probe histogram, the work-queue heads, the per-query bounds, the
arrival counters, grow-only buffers under changing layouts, raised LDS attributes, the settings views copy), and every form is one tenant
of it.  The per-kernel files build a handle per combination; here ONE handle per index walks all ordered pairs of forms
(sequences.transition_walk), and a fuzz deals settings, entries, views and mutations to one handle per draw.  Every search names the form
it must run BEFORE it is issued and asserts it through get_stats(); every result is compared exactly (counts, ids, distance bits over the
first `count` slots) with the CPU oracle, with tests/u16_ref.py or numpy, or -- UInt16 handles -- with a fresh handle's generic path that
numpy has checked.  A failure names the step, the form before it and the form itself."""
import os

import numpy as np
import pytest

import helpers
import sequences as sq
import u16_ref
from oracle import oracle as ora
from test_gpu_u16_edges import generic_of, u16_index

pytestmark = pytest.mark.gpu
f32 = np.float32
W = 3


def gpu_index(native, oidx):
    return native.IVFADCIndex.from_arrays(oidx.centroids, oidx.codebooks, oidx.labels, oidx.offsets, oidx.codes, oidx.ids)


def _form(name, qg, chunk=0, table=0, K=10, w=W, nq=None, prune=1, parts=0, ws=sq.WS_DEFAULT, **expect):
    """set_tuning(qg, chunk), set_table_mode(table), set_pruning(prune); nq: the first nq queries (None: all); parts: a list partition of
    that many parts, rehearsed on the one handle; ws: set_workspace_limit; expect: get_stats() fields the search must show ("lds_max": an upper bound of last_scan_lds)."""
    return dict(name=name, qg=qg, chunk=chunk, table=table, K=K, w=w, nq=nq, prune=prune, parts=parts, ws=ws, expect=expect)


def forms_8bit(m, dsub):
    """The forms of an 8-bit handle with lists of ~2 100 points (14 lists, 30 000 points): DESIGN.md 4.4 / 4.10 / 4.11."""
    filt = sq.filt_shape(m, dsub)
    wave8 = dict(lds_max=80 * 1024, last_nf=0)
    out = [
        _form("query-major", -1, last_qg=0, last_lb=0),
        _form("query-major, stand-alone top-w", -3, last_qg=0, last_lb=0),
        _form("small-batch single launch", 0, nq=9, last_qg=-3),
        _form("generic (forced)", -2, last_qg=-2),
        _form("generic by K", 0, K=2500, nq=8, last_qg=-2),
    ]
    for qg in (1, 2, 4):
        out.append(_form("list-major qg=%d reference tables" % qg, qg, 1024, table=1, last_qg=qg, last_striped=0, last_nf=0, last_chunk=1024))
    if m == 8:
        out += [
            _form("list-major qg=4 automatic tables", 4, 0, table=0, last_qg=4, last_striped=1 if filt else 0, last_nf=0),
            _form("eight-wave q4", 4, 0, table=6, last_qg=4, last_striped=2, **wave8),
            _form("eight-wave q8", 4, 0, table=7, last_qg=8, last_striped=3, **wave8),
            _form("eight-wave q4 K=64, several chunks", 4, 2048, table=6, K=64, last_qg=4, last_striped=2, last_chunk=2048, **wave8),
            _form("wide pool q4 K=100", 4, 0, table=8, K=100, last_qg=4, last_striped=4, last_nf=0),
            _form("wide pool q8 K=100", 4, 0, table=9, K=100, last_qg=8, last_striped=5, last_nf=0),
            _form("four-wave LDS selectors K=100", 4, 0, table=6, K=100, last_qg=4, last_striped=1 if filt else 0, last_nf=0,
                  last_scan_lds=sq.scan_lds_bytes(m, dsub, 256, 4, sq.cap_of(100), False, True, True)),
            _form("eight-wave q4 pruning off", 4, 0, table=6, prune=0, last_qg=4, last_striped=2, pruned_points=0, **wave8),
            _form("list partition on eight-wave q4", 4, 0, table=6, parts=2, last_qg=4, last_striped=2, **wave8),
            _form("list partition on wide pool q4", 4, 0, table=8, K=100, parts=2, last_qg=4, last_striped=4, last_nf=0),
        ]
        if sq.nf_shape(m, dsub):
            out.append(_form("narrow-field", 8, 0, table=0, last_qg=8, last_nf=1))
    else:
        out += [
            _form("m16 q4", 4, 0, table=6, last_qg=4, last_striped=2, **wave8),
            _form("m16 q8", 4, 0, table=7, last_qg=8, last_striped=3, **wave8),
            _form("m16 q4 K=64, several chunks", 4, 1024, table=6, K=64, last_qg=4, last_striped=2, last_chunk=1024, **wave8),
            _form("m16 q8 K=64, several chunks", 4, 1024, table=7, K=64, last_qg=8, last_striped=3, last_chunk=1024, **wave8),
            _form("striped four-wave", 4, 0, table=0, last_qg=4, last_striped=1, last_nf=0),
            # K = 65 under table mode 8: the wide pool is m = 8 only -- what mode 6 plans, the striped four-wave kernel on LDS selectors
            _form("K=65 under mode 8 leaves the kernel", 4, 0, table=8, K=65, last_qg=4, last_striped=1, last_nf=0,
                  last_scan_lds=sq.scan_lds_bytes(m, dsub, 256, 4, sq.cap_of(65), False, True, True)),
            _form("list partition on m16 q4", 4, 0, table=6, parts=2, last_qg=4, last_striped=2, **wave8),
        ]
    return out


def forms_u16(m, dsub, nq, kc):
    """K <= 64 on the register-selector kernel at every forced width and the plan's own, chunks of 4096 and the plan's, K = 1 / 10 / 64
    (table mode 10 where the chunk is the plan's: it must not matter there); mode 10 above 64 at both sides of two capacities; the
    generic path by table mode, by K and by request."""
    auto = sq.expected_form(dict(m=m, dsub=dsub, ksub=1024, kc=kc, n=0, u16=True), dict(table=0, qg=0), 10, W, nq)["last_qg"]
    out = []
    for qg in (1, 2, 4, 8, 0):
        for chunk in (4096, 0):
            for K in (1, 10, 64):
                exp = dict(last_qg=qg or auto, last_scan_lds=sq.u16_small_lds(m, dsub))
                if chunk:
                    exp["last_chunk"] = chunk
                out.append(_form("u16 K=%d qg=%d chunk=%d" % (K, qg, chunk), qg, chunk, table=0 if chunk else 10, K=K, **exp))
    for K, qg, chunk in ((65, 8, 0), (192, 4, 4096), (193, 0, 0), (1000, 8, 4096)):
        g = qg or auto
        cap = sq.cap_of(K)
        while g > 1 and sq.u16_wide_lds(m, dsub, g, cap) > sq.LDS_MAX:        # planned_qg of test_gpu_u16_wide.py
            g >>= 1
        assert sq.u16_wide_lds(m, dsub, g, cap) <= sq.LDS_MAX
        out.append(_form("u16 wide K=%d qg=%d chunk=%d" % (K, qg, chunk), qg, chunk, table=10, K=K, last_qg=g,
                         last_scan_lds=sq.u16_wide_lds(m, dsub, g, cap)))
    # the smallest workspace limit: 96 queries in two sub-batches (ten chunks of 1024 per list: per_q >= 16 132 B, 65 queries at the most),
    # so the merge re-arms the histogram, the queue head and the bounds in the middle of a search
    sub = dict(m=m, dsub=dsub, ksub=1024, kc=kc, n=40000, u16=True)
    for K, qg, table in ((64, 8, 0), (200, 4, 10)):
        st = dict(K=K, w=W, chunk=1024, ws=sq.WS_SMALL, table=table, qg=qg)
        assert sq.sub_batch_upper_bound(sub, st) < nq
        e = sq.expected_form(sub, st, K, W, nq)
        out.append(_form("u16 K=%d qg=%d in two sub-batches" % (K, qg), qg, 1024, table=table, K=K, ws=sq.WS_SMALL, last_chunk=1024,
                         last_qg=e["last_qg"], last_scan_lds=e["last_scan_lds"]))
    out += [
        _form("u16 mode 0 K=100 (generic)", 4, 0, table=0, K=100, last_qg=-2),
        _form("u16 mode 10 K=2500 (generic)", 0, 0, table=10, K=2500, nq=8, last_qg=-2),
        _form("u16 generic (forced)", -2, 0, table=10, K=10, last_qg=-2),
    ]
    return out


# ---- one index per handle kind, built once and left unchanged -----------------------------------------------------------------------------
class Kind:
    """An index, its queries, the exact reference per (K, w, nq) and -- 8-bit -- the partial keys of a list partition, computed once."""

    def __init__(self, name):
        self.name = name
        self.u16 = name == "u16"
        self.cache, self.pcache = {}, {}
        if self.u16:
            self.ix = u16_ref.make_index(4242, 40000, 32, 4, 4, 1024, perm_labels=True, ndistinct=5000)     # test_gpu_u16_wide.py: long_lists
            self.qs = np.random.default_rng(9).random((96, 32), dtype=f32)
            self.m, self.dsub, self.kc = 4, 8, 4
        else:
            m, d = {"m8_d128": (8, 128), "m8_d32": (8, 32), "m16_d128": (16, 128)}[name]
            if m == 16:
                from test_gpu_wg8_m16 import fixture
                self.ix, self.qs, _ = fixture(128, "random")
            else:
                self.ix, _ = helpers.build_index(2500 + d, 30000, d, 14, 8, 256, mode="random")
                self.qs = np.random.default_rng(177 + d).random((61, d), dtype=f32)
            self.m, self.dsub, self.kc = m, d // m, 14
            sizes = np.diff(self.ix.offsets)
            assert sizes.min() >= 2000 and sizes.max() > 2048, sizes      # several 1024-point chunks, one to two eight-wave steps

    def make(self, native):
        return u16_index(native, self.ix) if self.u16 else gpu_index(native, self.ix)

    def forms(self):
        return forms_u16(self.m, self.dsub, self.qs.shape[0], self.kc) if self.u16 else forms_8bit(self.m, self.dsub)

    def prepare(self, native, forms):
        """UInt16: the reference of every (K, w, nq) the forms use, from the generic path of a FRESH handle (never the handle under
        test), which numpy has checked on the first 8 queries."""
        if not self.u16:
            return
        g = u16_index(native, self.ix)
        for f in forms:
            key = (f["K"], f["w"], f["nq"])
            if key not in self.cache:
                q = self.qs[:f["nq"]]
                gen = generic_of(g, q, f["K"], f["w"])
                u16_ref.assert_exact(tuple(a[:8] for a in gen), u16_ref.knn(self.ix, q[:8], f["K"], f["w"]), "generic path vs numpy %s" % (key,))
                self.cache[key] = gen

    def expected(self, f):
        key = (f["K"], f["w"], f["nq"])
        if key not in self.cache:
            self.cache[key] = self.ix.knn_search(self.qs[:f["nq"]], f["K"], f["w"], nthreads=ora.max_threads())
        return self.cache[key]

    def partial(self, f, part):
        key = (f["K"], f["w"], f["parts"], part)
        if key not in self.pcache:
            self.pcache[key] = helpers.numpy_partial_keys(self.ix, self.qs[:12], f["K"], f["w"], f["parts"], part)
        return self.pcache[key]

    def same(self, got, f, what):
        if self.u16:
            u16_ref.assert_exact(got, self.expected(f), what)
        else:
            helpers.assert_same_results(got, self.expected(f), what=what)


_KINDS = {}


def kind_of(name):
    if name not in _KINDS:
        _KINDS[name] = Kind(name)
    return _KINDS[name]


def apply(g, f, u16=False):
    if not u16:
        g.set_list_partition(1, 0)
    g.set_tuning(f["qg"], f["chunk"])
    g.set_table_mode(f["table"])
    g.set_pruning(f["prune"])
    g.set_workspace_limit(f["ws"])


def ran(g, expect, what):
    st = g.get_stats()
    for key, val in expect.items():
        if key == "lds_max":
            assert st["last_scan_lds"] <= val, "%s did not run as the form it names: last_scan_lds = %s > %s (%s)" % (what, st["last_scan_lds"], val, st)
        else:
            assert st[key] == val, "%s did not run as the form it names: %s = %s, expected %s (%s)" % (what, key, st[key], val, st)


class DeviceIO:
    """Device-pointer searches: queries on the device once, fresh outputs per search."""

    def __init__(self, qs):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.qd = torch.from_numpy(np.ascontiguousarray(qs)).to(self.dev)
        self.other = torch.from_numpy(np.ascontiguousarray(qs[::-1] * f32(0.5))).to(self.dev)      # other queries: what a wrong hint names

    def outputs(self, nq, K):
        t = self.torch
        return (t.zeros(nq * K, dtype=t.int32, device=self.dev), t.zeros(nq * K, dtype=t.float32, device=self.dev), t.zeros(nq, dtype=t.int32, device=self.dev))

    def sync(self):
        self.torch.cuda.synchronize()

    def search(self, lanes, nq, K, w):
        """The same search on every lane, all in flight at once; the caller synchronises."""
        outs = [self.outputs(nq, K) for _ in lanes]
        self.sync()       # (torch fills the outputs on ITS stream: finished before the library's streams write into them)
        for g, o in zip(lanes, outs):
            g.search_device(nq, self.qd.data_ptr(), K, w, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
        return outs

    @staticmethod
    def host(o, nq, K):
        return o[0].cpu().numpy().view(np.uint32).reshape(nq, K), o[1].cpu().numpy().reshape(nq, K), o[2].cpu().numpy()


def run_form(kind, lanes, f, what, io=None):
    """One step on every lane (one lane: the host entry; several: the device-pointer entry, all lanes in flight, ONE synchronisation per
    search): settings, search, stats, exact comparison.  A partition form plays every part in turn on each lane (partial keys against numpy
    on 12 queries, the merge against the oracle), then switches the partition off and searches as the same form unpartitioned."""
    nq = f["nq"] or kind.qs.shape[0]
    K, w = f["K"], f["w"]
    for g in lanes:
        apply(g, f, kind.u16)
        if "pruned_points" in f["expect"]:
            g.reset_stats()
    if f["parts"]:
        t = io.torch
        keys = [t.zeros((f["parts"], nq, K), dtype=t.int64, device=io.dev) for _ in lanes]
        cnts = [t.zeros((f["parts"], nq), dtype=t.int32, device=io.dev) for _ in lanes]
        io.sync()
        for part in range(f["parts"]):
            for g, k, c in zip(lanes, keys, cnts):
                g.set_list_partition(f["parts"], part)
                g.search_device_partial(nq, io.qd.data_ptr(), K, w, k[part].data_ptr(), c[part].data_ptr())
            io.sync()
            rk, rc, _ = kind.partial(f, part)
            for li, (g, k, c) in enumerate(zip(lanes, keys, cnts)):
                ran(g, f["expect"], "%s, lane %d, part %d" % (what, li, part))
                gk, gc = k[part].cpu().numpy().view(np.uint64)[:12], c[part].cpu().numpy()[:12]
                assert np.array_equal(gc, rc) and all(np.array_equal(gk[r, :rc[r]], rk[r, :rc[r]]) for r in range(12)), \
                    "%s, lane %d: partial keys of part %d" % (what, li, part)
        outs = [io.outputs(nq, K) for _ in lanes]
        io.sync()
        for g, k, c, o in zip(lanes, keys, cnts, outs):
            g.merge_partials_device(nq, K, f["parts"], k.data_ptr(), c.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
        io.sync()
        for li, o in enumerate(outs):
            kind.same(io.host(o, nq, K), f, "%s, lane %d: merged parts" % (what, li))
        for g in lanes:
            g.set_list_partition(1, 0)
        what += ", partition off again"
    if len(lanes) == 1:
        got = [lanes[0].search_raw(kind.qs[:nq], K, w)]
    else:
        outs = io.search(lanes, nq, K, w)
        io.sync()
        got = [io.host(o, nq, K) for o in outs]
    for li, (g, r) in enumerate(zip(lanes, got)):
        ran(g, f["expect"], "%s, lane %d" % (what, li))
        kind.same(r, f, "%s, lane %d" % (what, li))


@pytest.mark.parametrize("name", ["m8_d128", "m8_d32", "m16_d128", "u16"])
def test_every_ordered_pair_of_forms_on_one_handle(native, name):
    """ONE handle, n forms, n * n + 1 searches: every form directly behind every form, itself included (sequences.transition_walk).  Then
    a view of the handle -- the last form's settings copied, its own fresh probe histogram -- walks the first n steps side by side with
    the index: two lanes, device-pointer entry, one synchronisation per step."""
    kind = kind_of(name)
    forms = kind.forms()
    kind.prepare(native, forms)
    g = kind.make(native)
    io = DeviceIO(kind.qs)
    if kind.u16:      # the list-partitioned mode serves UInt8 codes only: refused once, no partition forms on this kind
        from ivfadc_jl_amd import _native as nat
        with pytest.raises(nat.IVFADCError, match="UInt8 codes only"):
            g.set_list_partition(2, 0)
        g.set_list_partition(1, 0)
    walk = sq.transition_walk(len(forms))
    assert len(walk) == len(forms) ** 2 + 1
    prev = "a new handle"
    for step, fi in enumerate(walk):
        f = forms[fi]
        run_form(kind, [g], f, "%s step %d: [%s] behind [%s]" % (name, step, f["name"], prev), io)
        prev = f["name"]
    v = g.clone_view()
    for step, fi in enumerate(walk[:len(forms) + 1]):
        f = forms[fi]
        run_form(kind, [g, v], f, "%s view step %d: [%s] behind [%s]" % (name, step, f["name"], prev), io)
        prev = f["name"]


# ---- steered random sequences --------------------------------------------------------------------------------------------------------------
def _fuzz_index(shape):
    m, dsub, ksub, kc, n = (shape[k] for k in ("m", "dsub", "ksub", "kc", "n"))
    if shape["u16"]:
        return u16_ref.make_index(shape["seed"], n, m * dsub, kc, m, ksub, perm_labels=shape["label_perm"], ndistinct=shape["ndistinct"] or 0)
    return helpers.build_index(shape["seed"], n, m * dsub, kc, m, ksub, label_perm=shape["label_perm"], mode="random", ndistinct=shape["ndistinct"])[0]


def _rebuild(shape, ref, g):
    off, codes, ids = g._lists()
    if shape["u16"]:
        return u16_ref.U16Index(ref.centroids, ref.codebooks, ref.labels, off, codes, ids)
    return ora.OracleIndex(ref.centroids, ref.codebooks, ref.labels, off, codes, ids)


def _reference(shape, ref, gen, q, K, w):
    """8-bit: the C oracle.  UInt16: the generic path of a second handle that is never the one under test (kept in step with its lists),
    checked by numpy on three queries."""
    if not shape["u16"]:
        return ref.knn_search(q, K, w, nthreads=ora.max_threads())
    r = generic_of(gen, q, K, w)
    u16_ref.assert_exact(tuple(a[:3] for a in r), u16_ref.knn(ref, q[:3], K, w), "generic path vs numpy")
    return r


def test_fuzz_sequences_on_one_handle(native):
    """Seeded (sequences.draw_all; IVFADC_FUZZ_SEED / IVFADC_FUZZ_DRAWS widen it): per handle a shape -- m = 8 / 16 at the eight-wave
    widths, UInt16, or one no on-request kernel exists for --, then steps that draw table mode, tuning, chunk, K, w, batch, pruning,
    coarse mode, workspace limit and the entry (host, device pointers with a next-batch hint that is right, wrong or absent, a run of
    ragged batches whose odd ones use the internal view, a view searched while the index searches), one step in six a push or a delete
    (old views refuse, the reference is rebuilt from the handle's lists).  sequences.expected_form says before each search which form
    it must run, or that the automatic plan decides; on a shape without on-request kernels a table mode of 5 or more must plan what
    mode 0 plans."""
    seed = int(os.environ.get("IVFADC_FUZZ_SEED", str(sq.FUZZ_SEED)))
    handles = int(os.environ.get("IVFADC_FUZZ_DRAWS", str(sq.FUZZ_HANDLES)))
    keys = ("last_qg", "last_chunk", "last_scan_lds", "last_striped", "last_nf")
    for hi, (shape, steps) in enumerate(sq.draw_all(seed, handles)):
        shape = dict(shape)
        d = shape["m"] * shape["dsub"]
        ref = _fuzz_index(shape)
        g = u16_index(native, ref) if shape["u16"] else gpu_index(native, ref)
        gen = u16_index(native, ref) if shape["u16"] else None
        view = g.clone_view()
        rng = np.random.default_rng(shape["seed"] + 1)
        qs = rng.random((max(sq.NQS), d), dtype=f32)
        io = DeviceIO(qs)
        next_id = 10_000_000
        prev = "a new handle"
        for si, st in enumerate(steps):
            what = "sequence fuzz seed %d handle %d step %d: %s %s behind [%s]" % (seed, hi, si, {k: shape[k] for k in ("m", "dsub", "ksub", "kc", "n", "u16")}, st, prev)
            if st["op"] != "search":
                if st["op"] == "append":
                    pts = rng.random((st["count"], d), dtype=f32)
                    g._append(pts, np.arange(next_id, next_id + st["count"], dtype=np.uint32))
                    next_id += st["count"]
                else:
                    g._delete_ids(rng.integers(0, shape["n"], st["count"]).astype(np.uint32))
                ref = _rebuild(shape, ref, g)
                if gen is not None:
                    gen.set_lists(*g._lists())
                shape["n"] = len(g)
                with pytest.raises(Exception, match="changed since this view"):
                    view.search_raw(qs[:1], 3, 1)
                view = g.clone_view()
                prev = st["op"]
                continue
            K, w, nq = st["K"], st["w"], st["nq"]
            lanes = [g, view] if st["entry"] == "view" else [g]
            for ln in lanes:
                ln.set_tuning(st["qg"], st["chunk"])
                ln.set_table_mode(st["table"])
                ln.set_pruning(st["prune"])
                ln.set_coarse_mode(st["coarse"])
                ln.set_workspace_limit(st["ws"])
            q = qs[:nq]
            exp = _reference(shape, ref, gen, q, K, w)
            stats_nq = nq
            if st["entry"] == "search_raw":
                got = [g.search_raw(q, K, w)]
            elif st["entry"] == "search_batches":
                sizes = sq.batch_sizes(nq, st["nbatches"])
                cuts = np.concatenate([[0], np.cumsum(sizes)])
                parts = g.search_batches_raw([q[cuts[i]:cuts[i + 1]] for i in range(len(sizes))], K, w)
                got = [tuple(np.concatenate([p[i] for p in parts]) for i in range(3))]
                stats_nq = sq.index_lane_batch(sizes)           # the index's own lane searched the even batches
            else:
                hinted = st["entry"] == "search_device" and st["hint"] != "absent"
                if hinted:      # right: the follow-up search's own queries; wrong: as many OTHER queries in another buffer, same token
                    g.set_next_queries(nq, (io.qd if st["hint"] == "right" else io.other).data_ptr(), 7)
                outs = io.search(lanes, nq, K, w)
                io.sync()
                got = [io.host(o, nq, K) for o in outs]
                if hinted:      # the follow-up declares the hinted generation: it may start from rows that rode along only if they are ITS rows
                    g.set_query_token(7)
                    o = io.search([g], nq, K, w)[0]
                    io.sync()
                    got.append(io.host(o, nq, K))
                    lanes = [g, g]
            want = sq.expected_form(shape, st, K, w, stats_nq)
            for li, (ln, r) in enumerate(zip(lanes, got)):
                if want is not None:
                    ran(ln, want, "%s, lane %d" % (what, li))
                if shape["u16"]:
                    u16_ref.assert_exact(r, exp, "%s, lane %d" % (what, li))
                else:
                    helpers.assert_same_results(r, exp, what="%s, lane %d" % (what, li))
            if not shape["qualifies"] and st["table"] >= 5:
                # no on-request kernel for this shape: the mode quietly plans what mode 0 plans, and returns the same bytes
                # (query-major: last_scan_lds follows the probes per round, which the pruning feedback may move between two searches)
                mine = tuple(g.get_stats()[k] for k in keys)
                assert mine[3] not in (2, 3, 4, 5), (what, mine)
                g.set_table_mode(0)
                r0 = g.search_raw(q[:stats_nq], K, w)
                base = tuple(g.get_stats()[k] for k in keys)
                if mine[0] == 0:
                    mine, base = mine[:2] + mine[3:], base[:2] + base[3:]
                assert mine == base, "%s: table mode %d planned %s, mode 0 plans %s" % (what, st["table"], mine, base)
                part = tuple(a[:stats_nq] for a in exp)
                helpers.assert_same_results(r0, part, what=what + ", mode 0 again")
            form = sq.form_name(shape, want)
            prev = form or ("specified: %s" % (want,) if want is not None else "unspecified")
