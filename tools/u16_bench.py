"""Throughput of the UInt16-code scan (csrc/u16scan.hip.h) on one GPU: one JSON line.

Shapes: SIFT1M (d = 128, m = 8, n = 1e6, kc = 1024, 1024 queries, K = 10, w = 8) at k = 256 stored as UInt16, 1024 and 4096; Deep1B-like
d = 96, m = 16, k = 1024 on a shortened index (n = 1e6, kc = 4096) at 10 000 queries x w = 32; k = 65536 at small n.  Quantizers and codes
are random (the scan's cost does not depend on training); queries are data points plus noise.  Per shape: knn_search q/s of a
device-resident batch, scan time from events, pruned fraction, table-build element operations (3 d ksub per (query, probe)) per
second of scan time against the 78.6 T/s no-FMA vector-ALU peak, and codebook bytes read per table.

    python tools/u16_bench.py [--reps 10] [--only sift1m_k1024,...] [--K 100] [--table-mode 10] [--windows 5] [--u16-tables 1]
                              [--sweep-len 128,256,512,1024,2048]

--K overrides the shapes' K; --table-mode is passed to set_table_mode (10: K > 64 on the scan kernel's LDS-selector form instead of the
generic path, whose scan_ms covers its own kernels).  --windows N times N windows of --reps searches and reports the median window and
the spread (max - min) next to the mean; get_stats()["last_qg"] (pairs_per_item; -2 = generic path) tells which path ran.
--u16-tables is passed to set_u16_tables (1: the table-free scan, 2: where its rule expects it to win; 0 makes no call at all, so the
tool also runs against a library that lacks the entry); get_stats()["last_striped"] (6 / 7: table-free) is reported as "form".
--sweep-len adds the crossover sweep: the SIFT1M-shape quantizers at k = 1024 (d = 128, m = 8, kc = 1024, 1024 queries, K = 10, w = 8)
with n = L x kc points for every L given, named sift_k1024_len<L>: the list length at which tables and table-free sums cost the same
is what U16_DIRECT_COST (csrc/u16scan.hip.h) records.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ivfadc_jl_amd as pkg  # noqa: E402

SHAPES = [  # name, d, m, ksub, n, kc, nq, K, w
    ("sift1m_k256_u16", 128, 8, 256, 1_000_000, 1024, 1024, 10, 8),
    ("sift1m_k1024", 128, 8, 1024, 1_000_000, 1024, 1024, 10, 8),
    ("sift1m_k4096", 128, 8, 4096, 1_000_000, 1024, 1024, 10, 8),
    ("deep_d96_m16_k1024", 96, 16, 1024, 1_000_000, 4096, 10_000, 10, 32),
    ("k65536_small", 64, 4, 65536, 100_000, 256, 256, 10, 4),
]


def build(d, m, ksub, n, kc, seed=0):
    rng = np.random.default_rng(seed)
    cent = rng.random((kc, d), dtype=np.float32)
    cbs = ((rng.random((m, ksub, d // m), dtype=np.float32) - 0.5) * 0.5).astype(np.float32)
    labels = np.tile(np.arange(ksub, dtype=np.uint16), (m, 1))
    lst = rng.integers(0, kc, n)
    offsets = np.zeros(kc + 1, np.int64)
    np.cumsum(np.bincount(lst, minlength=kc), out=offsets[1:])
    codes = rng.integers(0, ksub, (n, m)).astype(np.uint16)
    g = pkg.IVFADCIndex.from_arrays(cent, cbs, labels, offsets, codes, np.arange(n, dtype=np.uint32))
    return g, cent, lst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma-separated shape names (default: all)")
    ap.add_argument("--K", type=int, default=0, help="K for every shape (default: the shape's own, 10)")
    ap.add_argument("--table-mode", type=int, default=0, help="ivfadc_set_table_mode (10: UInt16 scan kernel also for 64 < K)")
    ap.add_argument("--windows", type=int, default=1, help="timed windows of --reps searches each (median and spread are reported)")
    ap.add_argument("--u16-tables", type=int, default=0, choices=[0, 1, 2], help="ivfadc_set_u16_tables (1: table-free scan, 2: by its rule)")
    ap.add_argument("--sweep-len", default="", help="comma-separated average list lengths of the k = 1024 crossover sweep")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    shapes = SHAPES + [("sift_k1024_len%d" % L, 128, 8, 1024, L * 1024, 1024, 1024, 10, 8) for L in map(int, filter(None, args.sweep_len.split(",")))]
    import torch
    out = {"tool": "u16_bench", "shapes": {}}
    for name, d, m, ksub, n, kc, nq, K, w in shapes:
        if only and name not in only:
            continue
        K = args.K or K
        g, cent, lst = build(d, m, ksub, n, kc)
        if args.table_mode:
            g.set_table_mode(args.table_mode)
        if args.u16_tables:
            g.set_u16_tables(args.u16_tables)
        rng = np.random.default_rng(1)
        q = (cent[rng.integers(0, kc, nq)] + rng.normal(0, 0.05, (nq, d))).astype(np.float32)
        dq = torch.from_numpy(q).cuda()
        di = torch.zeros((nq, K), dtype=torch.int32, device="cuda")
        dd = torch.zeros((nq, K), dtype=torch.float32, device="cuda")
        dc = torch.zeros(nq, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        run = lambda: g.search_device(nq, dq.data_ptr(), K, w, di.data_ptr(), dd.data_ptr(), dc.data_ptr())  # noqa: E731
        for _ in range(3):
            run()
        g.sync()
        wins = []
        for _ in range(max(1, args.windows)):
            t0 = time.perf_counter()
            for _ in range(args.reps):
                run()
            g.sync()
            wins.append((time.perf_counter() - t0) / args.reps)
        dt = sum(wins) / len(wins)
        g.set_profiling(1)
        g.reset_stats()
        for _ in range(args.reps):
            run()
        g.sync()
        st = g.get_stats()
        g.set_profiling(0)
        scan_s = st["scan_ms"] / 1e3 / args.reps
        tables = nq * w
        pruned = st["pruned_points"] / max(1, st["scanned_points"])
        ops = 3.0 * d * ksub * tables * (1.0 - pruned)   # (an item that prunes builds no table: approximate by the point fraction)
        out["shapes"][name] = {
            "d": d, "m": m, "k": ksub, "n": n, "kc": kc, "nq": nq, "K": K, "w": w,
            "table_mode": args.table_mode, "u16_tables": args.u16_tables, "form": st["last_striped"],
            "qps": nq / dt, "ms_per_batch": dt * 1e3, "ms_per_batch_median": float(np.median(wins)) * 1e3,
            "ms_per_batch_spread": (max(wins) - min(wins)) * 1e3, "windows": len(wins), "reps": args.reps,
            "scan_ms": scan_s * 1e3, "pruned_fraction": pruned,
            "table_ops_per_s": ops / scan_s if scan_s > 0 else None,
            "table_ops_fraction_of_78.6T": (ops / scan_s) / 78.6e12 if scan_s > 0 else None,
            "codebook_bytes_per_table": 4 * d * ksub, "pairs_per_item": st["last_qg"], "chunk": st["last_chunk"],
            "scan_lds": st["last_scan_lds"],
        }
        print("[u16_bench] %s: %.0f q/s, scan %.3f ms, pruned %.2f" % (name, nq / dt, scan_s * 1e3, pruned), file=sys.stderr)
        del g
    print(json.dumps(out))


if __name__ == "__main__":
    main()
