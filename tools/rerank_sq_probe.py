"""What re-ranking against an 8-bit scalar-quantised vector store (ivfadc_vectors_create_sq) costs, takes and buys, beside
the Float16 store and the PQ store.

TIMING.  tools/rerank_probe.py's setting: SIFT1M bench shape, 1024 device-resident queries a call, K = 10, C in 100 and 1000, every leg
rotating through 8 query batches with their own candidate sets, HIP events on the handle's stream, a warm-up of every batch, windows of at
least 0.25 s of work, the median of the windows (fastest .. slowest).  Legs: ivfadc_rerank_device against the Float16 store (the
yardstick), against a PQ store of m2 = 16 (k2 = 256, trained on the first 100 000 rows, codeword pieces through the L2) and against the
SQ8 store with a trained range; the same candidates, the same process.  The legs ALTERNATE: every round of windows times each leg once, so
drift falls on all of them alike.
MEMORY.  Bytes per row and device bytes of the Float32, Float16, PQ and SQ8 stores.
RECALL.  bench.py's lowrank dataset and trained SIFT1M-shape index, 1024 queries, k = 10, w = 8, recall@1 in the top 10: plain, refined
against the SQ8 store, the Float16 store and a PQ store of m2 = 16 (trained on all rows), Kc in 100 and 1000.

    python tools/rerank_sq_probe.py [--windows 7] [--seconds 0.25] [--limit 500] [--out profiles/rerank_sq_probe.txt]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rerank_probe as base  # noqa: E402

from rerank_probe import CS, D, K, N, NQ, ROT, W, block, ptrs  # noqa: E402

LEGS = ("f16", "pq m2=16", "sq8")
STORES = ("f32",) + LEGS


def time_child(windows, seconds):
    import torch
    g, q = base.build()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    g.set_stream(stream.cuda_stream)
    rec = {}
    with torch.cuda.stream(stream):
        dq = torch.from_numpy(q).to(dev)
        dv = torch.rand((N, D), device=dev)
        stream.synchronize()
        st = {"f32": g.vectors_device(dv.data_ptr(), N, np.float32), "f16": g.vectors_device(dv.data_ptr(), N, np.float16),
              "pq m2=16": g.vectors_pq_device(dv.data_ptr(), N, 16, ntrain=100000), "sq8": g.vectors_sq_device(dv.data_ptr(), N)}
        rec["memory"] = {name: {"bytes_per_row": s.bytes_per_row, "nbytes": s.nbytes} for name, s in st.items()}
        del st["f32"]
        out = block(torch, dev, K)
        for C in CS:
            cand = [block(torch, dev, C) for _ in range(ROT)]
            for r in range(ROT):
                g.search_device(NQ, dq[r].data_ptr(), C, W, *ptrs(cand[r]))
            stream.synchronize()

            def window(store, reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for i in range(reps):
                    r = i % ROT
                    g.rerank_device(st[store], NQ, dq[r].data_ptr(), C, cand[r][0].data_ptr(), cand[r][2].data_ptr(), K, *ptrs(out))
                b.record(stream)
                b.synchronize()
                return a.elapsed_time(b) / reps * 1e3

            reps = {}
            for name in LEGS:
                window(name, 2 * ROT)
                reps[name] = max(2 * ROT, int(np.ceil(seconds * 1e6 / window(name, 2 * ROT) / ROT)) * ROT)
            wins = {name: [] for name in LEGS}
            for _ in range(windows):
                for name in LEGS:
                    wins[name].append(window(name, reps[name]))
            for name, w in wins.items():
                rec["%d|%s" % (C, name)] = {"us_median": float(np.median(w)), "us_min": float(min(w)), "us_max": float(max(w)), "calls_per_window": reps[name]}
    print(json.dumps(rec))


def recall_child():
    import torch
    import bench
    import ivfadc_jl_amd as pkg
    dev = torch.device("cuda:0")
    cfg = bench.CONFIGS["sift1m"]
    idx, x = bench.build_trained(pkg, cfg, dev, 0, None, "lowrank")
    q = bench.global_queries(cfg, NQ, dev, "lowrank")
    out = block(torch, dev, K)
    torch.cuda.synchronize()
    rec = {}
    idx.search_device(NQ, q.data_ptr(), K, W, *ptrs(out))
    idx.sync()
    rec["plain"] = bench.recall_at_1(x, q, out[0], out[2])
    for name, store in (("sq8", lambda: idx.vectors_sq_device(x.data_ptr(), cfg["n"])), ("f16", lambda: idx.vectors_device(x.data_ptr(), cfg["n"], np.float16)),
                        ("pq m2=16", lambda: idx.vectors_pq_device(x.data_ptr(), cfg["n"], 16))):
        s = store()
        for C in CS:
            idx.search_device_refined(s, NQ, q.data_ptr(), K, C, W, *ptrs(out))
            idx.sync()
            rec["refined %s Kc=%d" % (name, C)] = bench.recall_at_1(x, q, out[0], out[2])
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.25, help="work a window holds, at least")
    ap.add_argument("--limit", type=int, default=500, help="seconds each measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank_sq_probe.txt"))
    ap.add_argument("--time-child", action="store_true")
    ap.add_argument("--recall-child", action="store_true")
    args = ap.parse_args()
    if args.time_child:
        return time_child(args.windows, args.seconds)
    if args.recall_child:
        return recall_child()
    base.__file__ = os.path.abspath(__file__)                 # run_child starts this file's children
    lines = ["re-ranking against an SQ8 vector store beside the Float16 and PQ stores: tools/rerank_sq_probe.py --windows %d --seconds %g" % (args.windows, args.seconds),
             "TIMING: SIFT1M bench shape (d = %d, m = 8, n = 1e6, kc = 1024, random quantizers, codes and originals), %d device-resident queries a call, K = %d;" % (D, NQ, K),
             "every leg rotates through %d query batches with their own candidates; one MI355X, HIP events on the handle's stream, warm-up," % ROT,
             "legs alternating window by window; microseconds per call of ivfadc_rerank_device: median of the windows (fastest .. slowest).", ""]
    status, last = base.run_child(["--time-child", "--windows", str(args.windows), "--seconds", str(args.seconds)], args.limit)
    rec = json.loads(last) if status == 0 else None
    if rec is None:
        lines += ["TIMING AND MEMORY NOT MEASURED (the measuring process ended with status %d)" % status, ""]
    else:
        for C in CS:
            lines.append("C = %d" % C)
            for name in LEGS:
                v = rec["%d|%s" % (C, name)]
                lines.append("  %-10s %9.1f (%.1f .. %.1f), %d calls a window   this / f16 = %.2f" % (
                    name, v["us_median"], v["us_min"], v["us_max"], v["calls_per_window"], v["us_median"] / rec["%d|f16" % C]["us_median"]))
        lines += ["", "MEMORY (n = 1e6, d = %d)" % D]
        lines += ["  %-10s %4d bytes a row, %.1f MB on the device" % (name, rec["memory"][name]["bytes_per_row"], rec["memory"][name]["nbytes"] / 1e6) for name in STORES]
    lines += ["", "RECALL@1 in the top 10 (bench.py's lowrank dataset and trained sift1m index, %d queries, w = %d, exact neighbour by torch brute force)" % (NQ, W)]
    rstatus, rlast = base.run_child(["--recall-child"], args.limit) if status == 0 else (-1, "")   # nothing more on the GPU after a process that failed there
    if rstatus != 0:
        lines.append("  unmeasured (%s)" % ("the measuring process ended with status %d" % rstatus if status == 0 else "not run: the timing process failed"))
    else:
        rrec = json.loads(rlast)
        lines += ["  %-24s %.4f" % (k, v) for k, v in rrec.items()] + [json.dumps(rrec)]
    if rec:
        lines += ["", json.dumps(rec)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return status or (rstatus if rstatus > 0 else 0)


if __name__ == "__main__":
    sys.exit(main())
