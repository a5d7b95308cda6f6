"""What exact re-ranking (ivfadc_rerank_device, ivfadc_search_device_refined) costs and what it buys, on one GPU.

TIMING.  SIFT1M bench shape (d = 128, m = 8, n = 1e6, kc = 1024, random quantizers and codes; the originals are uniform random rows
generated on the device: 512 MB as Float32), 1024 device-resident queries a call, K = 10, w = 8, C = Kc in 100 and 1000, both store types.
Every leg ROTATES through 8 query batches with their own candidate sets (the ids and counts a plain search with K = C left in device
memory), so consecutive calls do not re-read the same rows out of the 256 MB cache in front of HBM.  HIP events on the handle's stream,
a warm-up of every batch, windows of at least 0.25 s of work, the median of the windows (fastest .. slowest):
  rerank f32 / f16   ivfadc_rerank_device
  refined f32        ivfadc_search_device_refined, the whole fused call
  plain              ivfadc_search_device with K = 10: what a step costs without the re-rank
  torch              the only route before: gather the rows, subtract, square, sum, topk in torch on the same GPU and stream.  Its
                     distances are NOT bit-comparable (another summation order), only its cost is.
KERNELS.  A run of its own per C under `rocprofv3 --kernel-trace --stats` (tracing slows the host, so no call time is taken from it):
the average time of rerank_dist_kernel per store type and of rerank_select_kernel, and the distance kernel's fraction of 8 TB/s counting
C x d x 4 (or x 2) row bytes per query.
RECALL.  bench.py's lowrank dataset and trained SIFT1M-shape index, its 1024 queries, the exact nearest neighbour from bench.py's torch
brute force: recall@1 in the top 10 of the plain search and of the refined search at Kc in 100 and 1000, the same w, both store types.

    python tools/rerank_probe.py [--windows 7] [--seconds 0.25] [--limit 300] [--out profiles/rerank_probe.txt]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, M, N, KC, K, W, NQ, ROT = 128, 8, 1_000_000, 1024, 10, 8, 1024, 8
CS = (100, 1000)
LEGS = ("rerank f32", "rerank f16", "refined f32", "plain", "torch")


def build():
    import ivfadc_jl_amd as pkg
    rng = np.random.default_rng(0)
    cent = rng.random((KC, D), dtype=np.float32)
    cbs = ((rng.random((M, 256, D // M), dtype=np.float32) - 0.5) * 0.5).astype(np.float32)
    labels = np.tile(np.arange(256, dtype=np.uint8), (M, 1))
    lst = np.sort(rng.integers(0, KC, N))
    offsets = np.zeros(KC + 1, np.int64)
    np.cumsum(np.bincount(lst, minlength=KC), out=offsets[1:])
    codes = rng.integers(0, 256, (N, M)).astype(np.uint8)
    g = pkg.IVFADCIndex.from_arrays(cent, cbs, labels, offsets, codes, np.arange(N, dtype=np.uint32))
    q = (cent[rng.integers(0, KC, ROT * NQ)] + rng.normal(0, 0.05, (ROT * NQ, D))).astype(np.float32)
    return g, q.reshape(ROT, NQ, D)


def block(torch, dev, width):
    return (torch.zeros((NQ, width), dtype=torch.int32, device=dev), torch.zeros((NQ, width), dtype=torch.float32, device=dev),
            torch.zeros(NQ, dtype=torch.int32, device=dev))


def ptrs(b):
    return [t.data_ptr() for t in b]


def setup(torch, cs):
    """the index on a torch stream, both stores, and per C the ROT candidate sets with one callable per leg taking the batch number"""
    g, q = build()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    g.set_stream(stream.cuda_stream)
    legs = {}
    with torch.cuda.stream(stream):
        dq = torch.from_numpy(q).to(dev)
        dv = torch.rand((N, D), device=dev)
        stream.synchronize()
        st = {"f32": g.vectors_device(dv.data_ptr(), N, np.float32), "f16": g.vectors_device(dv.data_ptr(), N, np.float16)}
        out = block(torch, dev, K)
        for C in cs:
            cand = [block(torch, dev, C) for _ in range(ROT)]
            for r in range(ROT):
                g.search_device(NQ, dq[r].data_ptr(), C, W, *ptrs(cand[r]))
            stream.synchronize()
            assert min(int(c[2].min()) for c in cand) == C, "every query has C candidates on this index"
            rows = [c[0].long() for c in cand]

            def rerank(r, store, C=C, cand=cand):
                g.rerank_device(st[store], NQ, dq[r].data_ptr(), C, cand[r][0].data_ptr(), cand[r][2].data_ptr(), K, *ptrs(out))

            legs[C] = {"rerank f32": lambda r, f=rerank: f(r, "f32"), "rerank f16": lambda r, f=rerank: f(r, "f16"),
                       "refined f32": lambda r, C=C: g.search_device_refined(st["f32"], NQ, dq[r].data_ptr(), K, C, W, *ptrs(out)),
                       "plain": lambda r: g.search_device(NQ, dq[r].data_ptr(), K, W, *ptrs(out)),
                       "torch": lambda r, rows=rows: torch.topk(((dv[rows[r]] - dq[r][:, None, :]) ** 2).sum(2), K, dim=1, largest=False)}
    return g, stream, legs, (st, dv, dq)


def time_child(windows, seconds):
    import torch
    g, stream, legs, keep = setup(torch, CS)
    rec = {}
    with torch.cuda.stream(stream):
        for C in CS:
            for name in LEGS:
                f = legs[C][name]

                def window(reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    for i in range(reps):
                        f(i % ROT)
                    b.record(stream)
                    b.synchronize()
                    return a.elapsed_time(b) / reps * 1e3

                window(2 * ROT)                                               # warm-up: every batch twice
                reps = max(2 * ROT, int(np.ceil(seconds * 1e6 / window(2 * ROT) / ROT)) * ROT)
                wins = [window(reps) for _ in range(windows)]
                rec["%d|%s" % (C, name)] = {"us_median": float(np.median(wins)), "us_min": float(min(wins)), "us_max": float(max(wins)), "calls_per_window": reps}
    print(json.dumps(rec))


def trace_child(C):
    """what the tracer watches: 5 rounds over the batches of both re-rank legs at one C"""
    import torch
    g, stream, legs, keep = setup(torch, (C,))
    with torch.cuda.stream(stream):
        for i in range(5 * ROT):
            legs[C]["rerank f32"](i % ROT)
            legs[C]["rerank f16"](i % ROT)
        stream.synchronize()


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
    for name, dtype in (("f32", np.float32), ("f16", np.float16)):
        store = idx.vectors_device(x.data_ptr(), cfg["n"], dtype)
        for C in CS:
            idx.search_device_refined(store, NQ, q.data_ptr(), K, C, W, *ptrs(out))
            idx.sync()
            rec["refined %s Kc=%d" % (name, C)] = bench.recall_at_1(x, q, out[0], out[2])
    print(json.dumps(rec))


def run_child(args, limit, prefix=()):
    cmd = ["timeout", "-k", "10", str(limit)] + list(prefix) + [sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    return r.returncode, last


def kernel_times(C, limit):
    """{kernel: average us} from a kernel-trace run of trace_child(C), or the reason there is none"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return "rocprofv3 is not installed"
    tmp = tempfile.mkdtemp(prefix="rerank_trace_")
    try:
        status, _ = run_child(["--trace-child", str(C)], limit, [rocprof, "--kernel-trace", "--stats", "-f", "csv", "-d", tmp, "--"])
        if status != 0:
            return "the traced process ended with status %d" % status
        found = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "").replace(" ", "")
                avg = float(row.get("AverageNs", "nan")) / 1e3
                if "rerank_dist_kernel" in name:
                    found["dist f16" if ("<true" in name or "ILb1E" in name) else "dist f32"] = avg
                elif "rerank_select_kernel" in name:
                    found["select"] = avg
        return found if len(found) == 3 else "the trace names %s of the three kernels" % (sorted(found) or "none")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.25, help="work a window holds, at least")
    ap.add_argument("--limit", type=int, default=300, help="seconds each measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank_probe.txt"))
    ap.add_argument("--time-child", action="store_true")
    ap.add_argument("--trace-child", type=int, default=0)
    ap.add_argument("--recall-child", action="store_true")
    args = ap.parse_args()
    if args.time_child:
        return time_child(args.windows, args.seconds)
    if args.trace_child:
        return trace_child(args.trace_child)
    if args.recall_child:
        return recall_child()
    lines = ["exact re-ranking: its cost against the plain search and the torch route, its kernels, and recall: tools/rerank_probe.py "
             "--windows %d --seconds %g" % (args.windows, args.seconds),
             "TIMING: SIFT1M bench shape (d = %d, m = %d, n = 1e6, kc = %d, random quantizers, codes and originals), %d device-resident queries a call," % (
                 D, M, KC, NQ),
             "K = %d, w = %d; every leg rotates through %d query batches with their own candidates; one MI355X, HIP events on the handle's stream," % (K, W, ROT),
             "warm-up, microseconds per call: median of the windows (fastest .. slowest).  The torch route's distances are not bit-comparable.", ""]
    status, last = run_child(["--time-child", "--windows", str(args.windows), "--seconds", str(args.seconds)], args.limit)
    if status != 0:
        lines += ["TIMING NOT MEASURED (the measuring process ended with status %d)" % status, ""]
        rec = None
    else:
        rec = json.loads(last)
        for C in CS:
            lines.append("C = Kc = %d" % C)
            for name in LEGS:
                v = rec["%d|%s" % (C, name)]
                note = "   torch / this = %.1f" % (rec["%d|torch" % C]["us_median"] / v["us_median"]) if name.startswith("rerank") else ""
                lines.append("  %-12s %9.1f (%.1f .. %.1f), %d calls a window%s" % (name, v["us_median"], v["us_min"], v["us_max"], v["calls_per_window"], note))
            lines.append("  the refined call costs %.1f us more than the plain K = %d step" % (
                rec["%d|refined f32" % C]["us_median"] - rec["%d|plain" % C]["us_median"], K))
            slower = [n for n in ("rerank f32", "rerank f16") if rec["%d|%s" % (C, n)]["us_median"] > rec["%d|torch" % C]["us_median"]]
            lines.append("  slower than the torch route: %s" % (", ".join(slower) if slower else "none"))
        lines.append("")
    lines.append("KERNELS (rocprofv3 --kernel-trace --stats, a run of its own per C; average microseconds per launch over %d launches)" % (5 * ROT))
    alive = status == 0                                   # nothing more is started on the GPU after a process that failed there
    for C in CS:
        kt = kernel_times(C, args.limit) if alive else "not run: an earlier measuring process failed"
        if isinstance(kt, str):
            lines.append("  C = %d: not separated (%s)" % (C, kt))
            alive = alive and not kt.startswith("the traced process")
            continue
        for kind, width in (("f32", 4), ("f16", 2)):
            us = kt["dist " + kind]
            gbs = NQ * C * D * width / (us * 1e-6) / 1e9
            lines.append("  C = %-5d rerank_dist_kernel %s %8.1f us: %.0f GB/s of row bytes = %.3f of 8 TB/s" % (C, kind, us, gbs, gbs / 8000))
        lines.append("  C = %-5d rerank_select_kernel   %8.1f us" % (C, kt["select"]))
    lines += ["", "RECALL@1 in the top 10 (bench.py's lowrank dataset and trained sift1m index, %d queries, w = %d, exact neighbour by torch brute force)" % (NQ, W)]
    rstatus, rlast = run_child(["--recall-child"], args.limit) if alive else (-1, "")
    if rstatus != 0:
        lines.append("  unmeasured (%s)" % ("the measuring process ended with status %d" % rstatus if alive else "not run: an earlier measuring process failed"))
    else:
        rrec = json.loads(rlast)
        lines += ["  %-22s %.4f" % (k, v) for k, v in rrec.items()]
        lines.append(json.dumps(rrec))
    if rec:
        lines += ["", json.dumps(rec)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return status or (rstatus if rstatus > 0 else 0)


if __name__ == "__main__":
    sys.exit(main())
