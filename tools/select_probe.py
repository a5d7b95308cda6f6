"""What the large-K search (ivfadc_set_tuning(h, -4, cap_keys): sel_scan_kernel, csrc/selscan.hip.h) costs against the
default plan and the generic path, on one GPU.

SIFT1M bench shape (d = 128, m = 8, n = 1e6, kc = 1024, random quantizers and codes), 1024 device-resident queries a call, w = 8.  Every
leg ROTATES through 8 query batches.  HIP events on the handle's stream, a warm-up of every batch, windows of at least 0.25 s of work,
the median of the windows (fastest .. slowest):
  plain     ivfadc_search_device at K = 65 / 100 / 256 / 1000 / 2048 under qg = 0 (the default plan, whose code this path does not touch:
            the parent commit's time), qg = -4 (this path) and qg = -2 (the generic dump-and-sort path)
  refined   ivfadc_search_device_refined, K = 10, at Kc = 100 / 1000 on a Float16 store under qg = 0 and qg = -4

    python tools/select_probe.py [--windows 7] [--seconds 0.25] [--limit 500] [--out profiles/select_probe.txt]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, M, N, KC, W, NQ, ROT = 128, 8, 1_000_000, 1024, 8, 1024, 8
KS = (65, 100, 256, 1000, 2048)
KCS = (100, 1000)
QGS = (0, -4, -2)
NAMES = {0: "default", -4: "select", -2: "generic"}


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


def time_child(windows, seconds):
    import torch
    g, q = build()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    g.set_stream(stream.cuda_stream)
    rec = {}
    with torch.cuda.stream(stream):
        dq = torch.from_numpy(q).to(dev)
        dv = torch.rand((N, D), device=dev)
        stream.synchronize()
        store = g.vectors_device(dv.data_ptr(), N, np.float16)
        out = [torch.zeros((NQ, max(KS)), dtype=torch.int32, device=dev), torch.zeros((NQ, max(KS)), dtype=torch.float32, device=dev),
               torch.zeros(NQ, dtype=torch.int32, device=dev)]
        ptrs = [t.data_ptr() for t in out]
        legs = [("plain K=%d" % K, qg, lambda r, K=K: g.search_device(NQ, dq[r].data_ptr(), K, W, *ptrs)) for K in KS for qg in QGS]
        legs += [("refined Kc=%d" % C, qg, lambda r, C=C: g.search_device_refined(store, NQ, dq[r].data_ptr(), 10, C, W, *ptrs))
                 for C in KCS for qg in QGS[:2]]
        for name, qg, f in legs:
            g.set_tuning(qg, 0)

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
            st = g.get_stats()
            rec["%s|%s" % (name, NAMES[qg])] = {"us_median": float(np.median(wins)), "us_min": float(min(wins)), "us_max": float(max(wins)),
                                               "calls_per_window": reps, "last_qg": st["last_qg"], "last_chunk": st["last_chunk"],
                                               "last_scan_lds": st["last_scan_lds"]}
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.25, help="work a window holds, at least")
    ap.add_argument("--limit", type=int, default=500, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_probe.txt"))
    ap.add_argument("--time-child", action="store_true")
    args = ap.parse_args()
    if args.time_child:
        return time_child(args.windows, args.seconds)
    lines = ["large-K search (ivfadc_set_tuning(h, -4, 0)) against the default plan (qg = 0) and the generic path (qg = -2): tools/select_probe.py "
             "--windows %d --seconds %g" % (args.windows, args.seconds),
             "SIFT1M bench shape (d = %d, m = %d, n = 1e6, kc = %d, random quantizers and codes), %d device-resident queries a call, w = %d;" % (
                 D, M, KC, NQ, W),
             "every leg rotates through %d query batches; one MI355X, HIP events on the handle's stream, warm-up, microseconds per call:" % ROT,
             "median of the windows (fastest .. slowest).  The default plan's code is untouched: its leg is the parent commit's time.", ""]
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--time-child", "--windows", str(args.windows),
           "--seconds", str(args.seconds)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    if r.returncode != 0:
        lines.append("NOT MEASURED (the measuring process ended with status %d)" % r.returncode)
    else:
        rec = json.loads(last)
        for leg in ["plain K=%d" % K for K in KS] + ["refined Kc=%d" % C for C in KCS]:
            lines.append(leg)
            base = rec[leg + "|default"]["us_median"]
            for qg in QGS:
                v = rec.get("%s|%s" % (leg, NAMES[qg]))
                if v is None:
                    continue
                lines.append("  %-8s %9.1f (%.1f .. %.1f), %d calls a window, last_qg %d, default / this = %.2f" % (
                    NAMES[qg], v["us_median"], v["us_min"], v["us_max"], v["calls_per_window"], v["last_qg"], base / v["us_median"]))
        slower = [k.split("|")[0] for k, v in rec.items() if k.endswith("|select") and v["us_median"] > rec[k.split("|")[0] + "|default"]["us_median"]]
        lines += ["", "the select path is slower than the default plan at: %s" % (", ".join(slower) if slower else "none"), "", json.dumps(rec)]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
