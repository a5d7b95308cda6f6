"""What tests/test_gpu_sequences.py needs and a CPU can check (tests/test_sequences_walk.py): the walk that puts every scan form behind
every other on one handle, the draws of the sequence fuzz, and a restatement of the plan's rules -- which form a search with given
settings must run -- from make_plan / make_plan_u16 (csrc/plan.h) and search_dev (csrc/ivfadc_hip.hip).  Nothing here touches the library."""
import numpy as np

LDS_MAX = 160 << 10
MAX_K = 2048          # IVFADC_MAX_K / IVFADC_MAX_W
WS_DEFAULT = 8 << 30  # the handle's workspace budget when nothing is set
WS_SMALL = 1 << 20    # the smallest budget ivfadc_set_workspace_limit admits: sub-batches of 64 wherever per_q reaches 16 KB


def transition_walk(n):
    """A closed walk over the forms 0 .. n-1 that takes every ordered pair (a, b), a == b included, exactly once: an Eulerian circuit of
    the complete digraph with loops (every vertex has n edges in and n out, and the graph is strongly connected), by Hierholzer's
    algorithm.  n * n + 1 vertices; walk[0] == walk[-1]; step i goes from walk[i] to walk[i + 1]."""
    if n < 1:
        return []
    used = [0] * n                 # out-edges of v are taken in the order v, v + 1, ... (mod n)
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if used[v] < n:
            stack.append((v + used[v]) % n)
            used[v] += 1
        else:
            out.append(stack.pop())
    return out[::-1]


# ---- the plan's rules, restated ---------------------------------------------------------------------------------------------------------
def pow2ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def cap_of(K):
    """make_plan: the selector capacity of K > 64."""
    return 64 if K <= 64 else max(128, pow2ceil(K + 64))


def filt_shape(m, dsub):
    return (m == 8 and dsub == 16) or (m == 16 and dsub in (6, 8))


def nf_shape(m, dsub):
    return m == 8 and dsub == 16


def w8_shape(m, dsub, on_request):
    """Shapes the eight-wave kernel is instantiated for; m = 16 on request only (table modes 6 .. 9)."""
    return (m == 8 and dsub in (4, 8, 12, 16)) or (m == 16 and dsub in (4, 8) and on_request)


def scan_lds_bytes(m, dsub, ksub, qg, cap, small, list_major, allow_filt):
    """scan_lds_bytes of the four-wave kernels (csrc/scan_layouts.h; restates carve_lds in kernels.hip.h)."""
    d = m * dsub
    b = max(m, 2) * 256 * qg * 4
    b += ((d * qg + 3) & ~3) * 4
    if not small:
        b += 4 * (qg if list_major else 1) * cap * 8
    b += 4 * qg * 4 + 16
    b = ((b + 7) & ~7) + qg * 40
    b += 3 * 256
    if list_major and qg == 4 and m in (8, 16):
        b += 4 * 16 * 5 * 4
    if list_major and qg == 4 and m == 8 and dsub == 16 and allow_filt and ksub == 256:
        b += 256 * 64
    return b


def u16_small_lds(m, dsub):
    return 8 * m * ((dsub + 3) & ~3) * 4 + 32768 + 4 * 8 * 4 + 16


def u16_wide_lds(m, dsub, qg, cap):
    return u16_small_lds(m, dsub) + 4 * qg * cap * 8


GENERIC = {"last_qg": -2}


def expected_form(shape, settings, K, w, nq):
    """The stats (get_stats() fields -> values) a search must show, or None where the automatic plan decides (tuning 0 on an 8-bit handle
    beyond the small-batch path: query-major against list-major, group widths from probes per list).
    shape: dict(m, dsub, ksub, kc, n, u16); settings: dict(table, qg, chunk, prune, part_n) -- what set_table_mode, set_tuning,
    set_pruning and set_list_partition were given.
    Conditions of make_plan that hold for every shape draw_shape and the pair tests use, and are therefore NOT restated: every list is
    shorter than the eight-wave kernels' position fields (maxlen < 2^27); the narrow-field tables exist wherever nf_shape holds (allow_nf,
    nf_n2: built at creation for m = 8, dsub = 16, ksub = 256); the small-batch path is not switched off (allow_sq, no IVFADC_NO_SMALLQ)
    and IVFADC_EXACT_TABLES is unset; kc stays below the two-level coarse search; K <= 2048 keeps every four-wave plan within a CU's LDS
    at one query per stream.  w is clamped to kc as check_search_args does.  A seed that draws outside these (a new shape list) has to
    extend the restatement first."""
    m, dsub, ksub, kc, n, u16 = (shape[k] for k in ("m", "dsub", "ksub", "kc", "n", "u16"))
    table, qg = settings["table"], settings["qg"]
    parted = settings.get("part_n", 1) > 1
    d = m * dsub
    w = min(w, kc)
    small_k = K <= 64
    # search_dev: the small-batch single launch first, then what only the generic path reaches
    if (not parted and not u16 and qg == 0 and K <= 64 and w <= 64 and nq <= 64 and nq * w <= 512 and d % 4 == 0 and
            scan_lds_bytes(m, dsub, ksub, 1, 64, True, False, table != 1) + 64 <= LDS_MAX):
        return {"last_qg": -3}
    if K > MAX_K or w > MAX_K or qg == -2 or (u16 and K > 64 and table != 10):
        return dict(GENERIC)
    ppl = float(nq) * w / max(1, kc)
    if u16:
        g = 8 if ppl >= 6.0 else (4 if ppl >= 2.5 else (2 if ppl >= 1.25 else 1))
        if qg in (1, 2, 4, 8):
            g = qg
        if small_k:
            return {"last_qg": g, "last_scan_lds": u16_small_lds(m, dsub), "last_striped": 0}
        cap = cap_of(K)
        while g > 1 and u16_wide_lds(m, dsub, g, cap) > LDS_MAX:
            g >>= 1
        if u16_wide_lds(m, dsub, g, cap) > LDS_MAX:
            return dict(GENERIC)
        return {"last_qg": g, "last_scan_lds": u16_wide_lds(m, dsub, g, cap), "last_striped": 0}
    forced = qg in (1, 2, 4, 8)
    if qg in (-1, -3) and not parted:
        return {"last_qg": 0}
    if not forced:
        return None
    # list-major at a forced width
    allow_filt = table != 1
    wg8_mode = -1 if table == 5 else (1 if table in (6, 8) else (2 if table in (7, 9) else 0))
    wg8_wide = table in (8, 9)
    avg_len = float(n) / max(1, kc)
    cap = cap_of(K)
    g = qg
    nf_ok = allow_filt and nf_shape(m, dsub) and ksub == 256 and small_k
    if qg == 8 and not nf_ok:
        g = 4
    if nf_ok and qg == 8:
        return {"last_qg": 8, "last_nf": 1}
    wide_k = (not small_k) and wg8_wide and wg8_mode > 0 and m == 8 and K <= 128
    w8_k = small_k or wide_k
    w8_md = w8_shape(m, dsub, wg8_mode > 0)
    m16_ok = small_k and allow_filt and m == 16 and w8_md and ksub == 256
    wide_ok = (wide_k and allow_filt and m == 8 and dsub in (4, 8, 12, 16) and ksub == 256) or m16_ok
    while g > 1 and not (g == 4 and wide_ok) and scan_lds_bytes(m, dsub, ksub, g, cap, small_k, True, allow_filt) > LDS_MAX:
        g >>= 1
    if not (g == 4 and wide_ok) and scan_lds_bytes(m, dsub, ksub, g, cap, small_k, True, allow_filt) > LDS_MAX:
        return dict(GENERIC)
    wg8 = (g == 4 and w8_k and allow_filt and wg8_mode >= 0 and w8_md and ksub == 256 and
           (wg8_mode > 0 or (m == 8 and dsub == 16 and not parted and avg_len >= 8192.0)))
    if wg8:
        q8 = wg8_mode == 2
        return {"last_qg": 8 if q8 else 4, "last_striped": (4 if not small_k else 2) + (1 if q8 else 0), "last_nf": 0}
    stripe = allow_filt and filt_shape(m, dsub) and g == 4 and ksub == 256
    return {"last_qg": g, "last_striped": 1 if stripe else 0, "last_nf": 0,
            "last_scan_lds": scan_lds_bytes(m, dsub, ksub, g, cap, small_k, True, allow_filt)}


# the on-request forms the fuzz must reach, by the stats that name them
def form_name(shape, exp):
    """eight-wave q4 / q8, wide q4 / q8, m16 q4 / q8, u16 K<=64, u16 wide -- or None for every other form."""
    if exp is None:
        return None
    if shape["u16"]:
        if exp.get("last_qg", 0) >= 1:
            return "u16 K<=64" if exp["last_scan_lds"] == u16_small_lds(shape["m"], shape["dsub"]) else "u16 wide"
        return None
    s = exp.get("last_striped")
    if s in (2, 3, 4, 5):
        if shape["m"] == 16:
            return {2: "m16 q4", 3: "m16 q8"}[s]
        return {2: "eight-wave q4", 3: "eight-wave q8", 4: "wide q4", 5: "wide q8"}[s]
    return None


ON_REQUEST = ("eight-wave q4", "eight-wave q8", "wide q4", "wide q8", "m16 q4", "m16 q8", "u16 K<=64", "u16 wide")

# ---- the draws of test_fuzz_sequences_on_one_handle ---------------------------------------------------------------------------------------
# The default seed.  It has to give every on-request form at least three times, each at least once directly behind a different one of
# them, and each at least once in a search that certainly takes several sub-batches (tests/test_sequences_walk.py asserts all three on
# the draws alone).  2026, the year the other fuzzes took theirs from, does not (no UInt16 handle, no eight-query wide pool); 14 is
# the first of 1, 2, 3, ... that does.
FUZZ_SEED = 14
FUZZ_HANDLES = 12
FUZZ_STEPS = 12
TABLES = tuple(range(11))
TUNINGS = (-3, -1, 0, 1, 2, 4, 8)
CHUNKS = (0, 1024, 4096)
KS = (1, 10, 63, 64, 65, 100, 128, 129, 200, 2500)
WS = (1, 3, 8, 70)
NQS = (1, 9, 61, 130, 257)
ENTRIES = ("search_raw", "search_device", "search_batches", "view")


def draw_shape(rng):
    """One handle's shape: m = 8 at the four eight-wave widths, m = 16 at its two, a UInt16 shape, and one draw in four a shape no on-request
    kernel is instantiated for (m = 4; ksub = 255; m = 16 at dsub = 6)."""
    if rng.random() < 0.25:
        m, dsub, ksub = [(4, 8, 256), (8, 16, 255), (16, 6, 256)][int(rng.integers(0, 3))]
        u16, qualifies = False, False
    else:
        kind = int(rng.integers(0, 3))
        qualifies = True
        if kind == 0:
            m, dsub, ksub, u16 = 8, int(rng.choice([4, 8, 12, 16])), 256, False
        elif kind == 1:
            m, dsub, ksub, u16 = 16, int(rng.choice([4, 8])), 256, False
        else:
            m, dsub, ksub, u16 = int(rng.choice([2, 4])), int(rng.choice([4, 8])), int(rng.choice([300, 1024])), True
    kc = int(rng.choice([3, 14, 300]))
    n = int(rng.choice([3000, 30000]))
    return dict(m=m, dsub=dsub, ksub=ksub, u16=u16, qualifies=qualifies, kc=kc, n=n, label_perm=bool(rng.random() < 0.5),
                ndistinct=4 if rng.random() < 0.2 else None, seed=int(rng.integers(0, 1 << 30)))


def draw_step(rng, shape, steer):
    """One step: either a mutation (one in six) or a search with every setting drawn.  `steer` (0 .. 1): the share of steps whose table
    mode, tuning and K are drawn from the on-request combinations of the handle's shape instead of from the full lists -- the full lists
    alone reach a given on-request form about once in a hundred steps."""
    if rng.random() < 1.0 / 6.0:
        if rng.random() < 0.6:
            return dict(op="append", count=int(rng.integers(1, 41)))
        return dict(op="delete", count=int(rng.integers(1, 6)))
    st = dict(op="search", table=int(rng.choice(TABLES)), qg=int(rng.choice(TUNINGS)), chunk=int(rng.choice(CHUNKS)), K=int(rng.choice(KS)),
              w=int(rng.choice(WS)), nq=int(rng.choice(NQS)), prune=int(rng.integers(0, 2)), coarse=int(rng.integers(0, 2)),
              ws=WS_SMALL if rng.random() < 0.5 else WS_DEFAULT, entry=str(rng.choice(ENTRIES)), hint=str(rng.choice(["right", "wrong", "absent"])),
              nbatches=int(rng.integers(1, 5)))
    if rng.random() < steer and shape["qualifies"]:
        # with the small workspace limit the steered step is also made HEAVY: a forced chunk of 1024 points, 130 or 257 queries through one
        # entry, 8 or 70 probes and the upper half of the form's K -- w maxch (8 K + 4) bytes per query are then what pushes the sub-batch
        # below the batch (sub_batch_upper_bound), so that the chain of kernels re-arms the handle's state inside one search
        heavy = st["ws"] == WS_SMALL
        if shape["u16"]:
            st["table"] = int(rng.choice([0, 10, 10]))
            st["qg"] = int(rng.choice([0, 1, 2, 4, 8]))
            if st["table"] == 0:
                st["K"] = int(rng.choice([63, 64] if heavy else [1, 10, 63, 64]))
            else:
                st["K"] = int(rng.choice([100, 128, 129, 200] if heavy else KS[:-1]))
        else:
            st["table"] = int(rng.choice([6, 7, 8, 9]))
            st["qg"] = 4
            if shape["m"] == 8:
                st["K"] = int(rng.choice(([100, 128] if st["table"] >= 8 else [63, 64]) if heavy else KS[:7]))
            else:
                st["K"] = int(rng.choice([63, 64] if heavy else KS[:4]))
        if heavy:
            st["chunk"] = 1024
            st["nq"] = int(rng.choice([130, 257]))
            st["w"] = int(rng.choice([8, 70]))
            st["entry"] = str(rng.choice(["search_raw", "search_device", "view"]))
    return st


def sub_batch_upper_bound(shape, st):
    """An upper bound of the sub-batch size nb that make_plan / make_plan_u16 give a list-major search with a FORCED chunk under the
    step's workspace limit: nb = max(64, budget / per_q), per_q = 4 kc + w maxch (8 K + 4) + 20 w + 8 K + 64 with
    maxch = ceil(longest list / chunk).  The longest list is not known here; it is at least the average one, taken 60 points short
    (what the deletes of one handle's steps can remove at most), so per_q is a lower bound and nb an upper one.  (The shapes drawn keep
    kc below the two-level coarse search and every list below 64 chunks, where the plan would widen the chunk.)"""
    assert st["chunk"] > 0 and st["chunk"] % 1024 == 0
    kc, w, K = shape["kc"], min(st["w"], shape["kc"]), st["K"]
    shortest_longest = -(-max(0, shape["n"] - 60) // kc)
    maxch = max(1, -(-shortest_longest // st["chunk"]))
    per_q = 4 * kc + w * maxch * (8 * K + 4) + 20 * w + 8 * K + 64
    return max(64, max(st["ws"], 1 << 20) // per_q)


def draw_all(seed=FUZZ_SEED, handles=FUZZ_HANDLES, steps=FUZZ_STEPS, steer=0.5):
    """[(shape, [step, ...]), ...] of a seed: what the GPU test runs and what the CPU test counts."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(handles):
        shape = draw_shape(rng)
        out.append((shape, [draw_step(rng, shape, steer) for _ in range(steps)]))
    return out


def batch_sizes(nq, nbatches):
    """nq queries as nbatches ragged batches (sizes differ by position; none is empty)."""
    nb = max(1, min(nbatches, nq))
    cuts = [nq * (i * (i + 1)) // (nb * (nb + 1)) for i in range(nb + 1)]       # growing sizes: 1 : 2 : 3 : ...
    sizes = [max(1, cuts[i + 1] - cuts[i]) for i in range(nb)]
    sizes[-1] += nq - sum(sizes)
    if sizes[-1] < 1:
        return [nq]
    return sizes


def index_lane_batch(sizes):
    """ivfadc_search_batches deals the even batches to the index's own lane and the odd ones to its internal view: the size of the last
    batch the index itself searched, which is what its get_stats() describes afterwards."""
    last = len(sizes) - 1
    return sizes[last if last % 2 == 0 else last - 1]


def sub_batched_forms(seed=FUZZ_SEED, handles=FUZZ_HANDLES, steps=FUZZ_STEPS):
    """The on-request forms that at least one step of a seed's draws runs in SEVERAL sub-batches for certain (sub_batch_upper_bound
    below the batch): {name: number of such steps}."""
    out = {}
    for shape, sts in draw_all(seed, handles, steps):
        for st in sts:
            if st["op"] != "search" or st["entry"] == "search_batches" or st["chunk"] == 0:
                continue
            name = form_name(shape, expected_form(shape, st, st["K"], st["w"], st["nq"]))
            if name is not None and sub_batch_upper_bound(shape, st) < st["nq"]:
                out[name] = out.get(name, 0) + 1
    return out


def specified_forms(seed=FUZZ_SEED, handles=FUZZ_HANDLES, steps=FUZZ_STEPS):
    """The on-request form of every search step of a seed's draws, in order and per handle: [[name or None, ...], ...] -- None for a
    mutation, for an unspecified step and for every other form.  n is taken as drawn (a mutation moves it by at most 40 points, far from
    the one rule that reads it: 8192 points per list)."""
    out = []
    for shape, sts in draw_all(seed, handles, steps):
        row = []
        for st in sts:
            if st["op"] != "search":
                row.append(None)
                continue
            nq = index_lane_batch(batch_sizes(st["nq"], st["nbatches"])) if st["entry"] == "search_batches" else st["nq"]
            row.append(form_name(shape, expected_form(shape, st, st["K"], st["w"], nq)))
        out.append(row)
    return out
