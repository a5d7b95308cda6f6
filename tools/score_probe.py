"""What scoring caller-supplied candidate ids costs (ivfadc_score_ids_device) against the only bit-identical route there
was before it, on one GPU.

SIFT1M bench shape (d = 128, m = 8, n = 1e6, kc = 1024, random quantizers and codes), device-resident queries (a centroid plus noise).
Per-query candidate lists of C = 100 and C = 1000 distinct ids: the query's own top results (w = 8; 50 of them at C = 100, 100 at
C = 1000) padded with random stored ids.

  score          ivfadc_score_ids_device on NQ = 1024 queries (and on the baseline's 64, for the same-batch comparison)
  locate         ivfadc_locate_device on the same NQ x C flattened ids: the locate pass of the path above, alone.  The pair kernel's
                 share is the difference (score - locate), and is named so.
  masked         the baseline: ONE mask set with one mask per query holding the same ids, ivfadc_search_device_masked with w = kc and
                 K = C -- every stored entry of every list is read for every query.  NQ_MASKED = 64 queries, as many as one mask set of
                 64 masks over 1e6 ids (8 MB of bitmaps) takes; timed with the mask-set build (host bitmaps -> ivfadc_maskset_create)
                 included and excluded.

Before anything is timed the distance bits of `score` and `masked` are ASSERTED equal for every (query, id) of the 64 queries.
One child process under `timeout`; the legs alternate in every window, after a warm-up, a host clock around work that ends with a
synchronise.  The parent writes the medians of the windows, their fastest and slowest window, and says "not measured" if the child did
not finish.

    python tools/score_probe.py [--reps 3] [--windows 5] [--seconds 0.5] [--limit 500] [--out profiles/score_probe.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, M, N, KC, NQ, W = 128, 8, 1_000_000, 1024, 1024, 8
NQ_MASKED = 64
SIZES = ((100, 50), (1000, 100))          # (C, how many of the query's own top results)


def build():
    import ivfadc_jl_amd as pkg
    rng = np.random.default_rng(0)
    cent = rng.random((KC, D), dtype=np.float32)
    cbs = ((rng.random((M, 256, D // M), dtype=np.float32) - 0.5) * 0.5).astype(np.float32)
    labels = np.tile(np.arange(256, dtype=np.uint8), (M, 1))
    lst = rng.integers(0, KC, N)
    offsets = np.zeros(KC + 1, np.int64)
    np.cumsum(np.bincount(lst, minlength=KC), out=offsets[1:])
    codes = rng.integers(0, 256, (N, M)).astype(np.uint8)
    g = pkg.IVFADCIndex.from_arrays(cent, cbs, labels, offsets, codes, np.arange(N, dtype=np.uint32))
    q = (cent[rng.integers(0, KC, NQ)] + rng.normal(0, 0.05, (NQ, D))).astype(np.float32)
    return g, q, rng


def candidate_rows(g, q, ncand, ntop, rng):
    """(NQ, ncand) distinct ids per row: the query's top `ntop`, then random stored ids, in a shuffled order"""
    top, _, cnt = g.search_raw(q, ntop, W)
    assert (cnt == ntop).all()
    rows = np.zeros((len(q), ncand), np.uint32)
    for i in range(len(q)):
        pool = np.concatenate([top[i], rng.integers(0, N, 2 * ncand).astype(np.uint32)])
        _, first = np.unique(pool, return_index=True)
        rows[i] = rng.permutation(pool[np.sort(first)][:ncand])
    return rows


def run_legs(g, legs, reps, windows, seconds):
    for _, f in legs:             # warm-up: code objects, workspace
        for _ in range(2):
            f()
    nrep = {}
    for name, f in legs:          # a window holds at least `reps` batches and about `seconds` of work
        g.sync()
        t0 = time.perf_counter()
        f()
        g.sync()
        nrep[name] = max(reps, int(np.ceil(seconds / max(time.perf_counter() - t0, 1e-6))))
    wins = {name: [] for name, _ in legs}
    for _ in range(windows):
        for name, f in legs:      # the legs alternate inside every window
            g.sync()
            t0 = time.perf_counter()
            for _ in range(nrep[name]):
                f()
            g.sync()
            wins[name].append((time.perf_counter() - t0) / nrep[name] * 1e3)
    return {name: {"ms_median": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v)), "batches_per_window": nrep[name]}
            for name, v in wins.items()}


def child(reps, windows, seconds):
    import torch
    g, q, rng = build()
    dev = torch.device("cuda:0")
    dq = torch.from_numpy(q).to(dev)
    out = {"sizes": {}}
    for ncand, ntop in SIZES:
        rows = candidate_rows(g, q, ncand, ntop, rng)
        drows = torch.from_numpy(rows.view(np.int32)).to(dev)
        dd = torch.zeros((NQ, ncand), dtype=torch.float32, device=dev)
        dl = torch.zeros(NQ * ncand, dtype=torch.int32, device=dev)
        dp = torch.zeros(NQ * ncand, dtype=torch.int64, device=dev)
        mi = torch.zeros((NQ_MASKED, ncand), dtype=torch.int32, device=dev)
        md = torch.zeros((NQ_MASKED, ncand), dtype=torch.float32, device=dev)
        mc = torch.zeros(NQ_MASKED, dtype=torch.int32, device=dev)
        moq = torch.arange(NQ_MASKED, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        held = {}

        def score_all():
            g.score_device(NQ, dq.data_ptr(), ncand, ncand, drows.data_ptr(), None, dd.data_ptr(), None)
            g.sync()

        def score_64():
            g.score_device(NQ_MASKED, dq.data_ptr(), ncand, ncand, drows.data_ptr(), None, dd.data_ptr(), None)
            g.sync()

        def locate_all():
            g.locate_device(NQ * ncand, drows.data_ptr(), dl.data_ptr(), dp.data_ptr())
            g.sync()

        def masked_search():
            g.search_device_masked(held["ms"], NQ_MASKED, dq.data_ptr(), ncand, KC, moq.data_ptr(), mi.data_ptr(), md.data_ptr(), mc.data_ptr())
            g.sync()

        def masked_with_build():
            held["ms"] = g.maskset(ids=[rows[i] for i in range(NQ_MASKED)])
            masked_search()

        # the same bits, before anything is timed
        masked_with_build()
        score_all()
        assert (mc.cpu().numpy() == ncand).all(), "a masked search did not return all of its mask's ids"
        m_ids = mi.cpu().numpy().view(np.uint32)
        m_bits = md.cpu().numpy().view(np.uint32)
        s_bits = dd.cpu().numpy().view(np.uint32)[:NQ_MASKED]
        for i in range(NQ_MASKED):
            a, b = np.argsort(m_ids[i]), np.argsort(rows[i])
            assert np.array_equal(m_ids[i][a], rows[i][b]) and np.array_equal(m_bits[i][a], s_bits[i][b]), "query %d: the routes differ" % i
        legs = (("score_%d_queries" % NQ, score_all), ("locate_%d_queries" % NQ, locate_all), ("score_%d_queries" % NQ_MASKED, score_64),
                ("masked_%d_queries_search_only" % NQ_MASKED, masked_search), ("masked_%d_queries_with_set_build" % NQ_MASKED, masked_with_build))
        out["sizes"][str(ncand)] = run_legs(g, legs, reps, windows, seconds)
        held.clear()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5, help="work a window holds, at least (and at least --reps batches)")
    ap.add_argument("--limit", type=int, default=500, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_probe.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.reps, args.windows, args.seconds)
    lines = ["scoring candidate ids against a masked search over the same ids: tools/score_probe.py --reps %d --windows %d --seconds %g"
             % (args.reps, args.windows, args.seconds),
             "SIFT1M bench shape (d = 128, m = 8, n = 1e6, kc = 1024, random quantizers and codes), device-resident queries; per-query rows of C",
             "distinct ids (the query's own top results padded with random stored ids); baseline: one mask per query, w = kc, K = C; one MI355X,",
             "one bounded process, legs alternating inside every window; milliseconds per batch, median of the windows (fastest .. slowest)", ""]
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps),
           "--windows", str(args.windows), "--seconds", str(args.seconds)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    status = r.returncode
    if status != 0:
        lines += ["NOT MEASURED (the measuring process ended with status %d)" % status, ""]
    else:
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        for ncand, legs in rec["sizes"].items():
            lines.append("C = %s" % ncand)
            for name, v in legs.items():
                lines.append("  %-40s %10.3f ms  (windows %.3f .. %.3f, %d batches a window)"
                             % (name, v["ms_median"], v["ms_min"], v["ms_max"], v["batches_per_window"]))
            sc, lo = legs["score_%d_queries" % NQ]["ms_median"], legs["locate_%d_queries" % NQ]["ms_median"]
            s64 = legs["score_%d_queries" % NQ_MASKED]["ms_median"]
            ms, mb = legs["masked_%d_queries_search_only" % NQ_MASKED]["ms_median"], legs["masked_%d_queries_with_set_build" % NQ_MASKED]["ms_median"]
            lines += ["  split of score at %d queries: locate pass %.3f ms (%.0f %%), pair kernel and the rest, by difference, %.3f ms"
                      % (NQ, lo, 100.0 * lo / sc, sc - lo),
                      "  per query: score %.2f us at %d queries, %.2f us at %d; masked %.1f us (search only), %.1f us (with the set's build)"
                      % (1e3 * sc / NQ, NQ, 1e3 * s64 / NQ_MASKED, NQ_MASKED, 1e3 * ms / NQ_MASKED, 1e3 * mb / NQ_MASKED),
                      "  same %d queries: masked / score = %.1f x (search only), %.1f x (with the set's build)" % (NQ_MASKED, ms / s64, mb / s64), ""]
        lines += ["same distance bits for every (query, id) of the %d queries asserted before timing: True" % NQ_MASKED, json.dumps(rec), ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return status


if __name__ == "__main__":
    sys.exit(main())
