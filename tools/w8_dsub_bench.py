"""Eight-wave against four-wave list-major scan (csrc/wg8scan.hip.h against scan_kernel) per sub-space width on one GPU: JSON lines.

A synthetic long-list index per d = 32 / 64 / 96 / 128 at m = 8 (random quantizers and codes, as tools/u16_bench.py builds its own:
the scan's cost does not depend on training): 512 lists of 65 536 points.  Batches of 4096 queries at w = 1 and 2 (8 and 16 probes
per list: the eight-query form's regime) and 1024 queries at w = 1 (2 probes per list: the four-query form's).  Per batch and table
mode -- 5: never the eight-wave kernel (what the plan ran before the kernel knew the width), 6 / 7: its four- / eight-query form, 0: the
plan's own choice -- the scan time from events: the median of `--windows` windows of `--reps` launches each, and the windows' spread.
With --partition N every search is rank 0's share of an N-way list partition (ivfadc_search_device_partial).
--k sets K (default 10).  Above 64 the eight-wave kernel runs through table modes 8 / 9 only (its wide-pool form, K <= 128); mode 6 is the
four-wave kernel with LDS selectors there, which is what the A/B of the wide pool compares with.
--m 16 builds the index with sixteen sub-quantizers (d = 128 and 64: wg8_m16_scan_kernel<NQ, DS>, on request only -- modes 6 / 7; modes 5
and 0 are the four-wave kernel with bank-striped f32 tables there, K <= 64):

    python tools/w8_dsub_bench.py [--d 32,64,96,128] [--windows 5] [--reps 8] [--partition 8]
    python tools/w8_dsub_bench.py --d 128 --k 100,128 --modes 6,8,9 --out profiles/wg8_wide.json
    python tools/w8_dsub_bench.py --m 16 --d 128,64 --modes 5,6,7,0 --out profiles/wg8_m16.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ivfadc_jl_amd as pkg  # noqa: E402

KC, LIST = 512, 65536
BATCHES = ((4096, 2), (4096, 1), (1024, 1))
KERNEL = {0: "reference-order", 1: "four-wave", 2: "eight-wave q4", 3: "eight-wave q8", 4: "eight-wave wide q4", 5: "eight-wave wide q8"}


def kernel_symbol(m, dsub, striped):
    """The instantiation behind stats.last_striped 2 ... 5 (csrc/wg8scan.hip.h); None for the four-wave kernels."""
    if striped not in (2, 3, 4, 5):
        return None
    nq = 8 if striped in (3, 5) else 4
    if m == 16:
        return "wg8_m16_scan_kernel<%d, %d>" % (nq, dsub)
    if striped >= 4:
        return "wg8_wide_scan_kernel<%d, %d>" % (nq, dsub)
    return "wg8_scan_kernel<%d>" % nq if dsub == 16 else "wg8_scan_kernel<%d, %d>" % (nq, dsub)


def build(d, seed=0, M=8):
    rng = np.random.default_rng(seed)
    n = KC * LIST
    cent = rng.random((KC, d), dtype=np.float32)
    cbs = ((rng.random((M, 256, d // M), dtype=np.float32) - 0.5) * 0.5).astype(np.float32)
    labels = np.tile(np.arange(256, dtype=np.uint8), (M, 1))
    offsets = np.arange(KC + 1, dtype=np.int64) * LIST
    codes = rng.integers(0, 256, (n, M), dtype=np.uint8)
    return pkg.IVFADCIndex.from_arrays(cent, cbs, labels, offsets, codes, np.arange(n, dtype=np.uint32)), cent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", default="32,64,96,128")
    ap.add_argument("--m", type=int, default=8, choices=(8, 16), help="sub-quantizers (16: d = 128 and 64)")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--modes", default="5,6,7,0")
    ap.add_argument("--partition", type=int, default=0)
    ap.add_argument("--k", default="10", help="K, or several separated by commas")
    ap.add_argument("--out", default="", help="also write the runs to this JSON file")
    args = ap.parse_args()
    import torch
    M = args.m
    runs = []
    for d in (int(x) for x in args.d.split(",")):
        g, cent = build(d, M=M)
        if args.partition > 1:
            g.set_list_partition(args.partition, 0)
        for K, (nq, w) in ((int(k), b) for k in args.k.split(",") for b in BATCHES):
            rng = np.random.default_rng(1)
            q = (cent[rng.integers(0, KC, nq)] + rng.normal(0, 0.05, (nq, d))).astype(np.float32)
            dq = torch.from_numpy(q).cuda()
            di = torch.zeros((nq, K), dtype=torch.int32, device="cuda")
            dd = torch.zeros((nq, K), dtype=torch.float32, device="cuda")
            dc = torch.zeros(nq, dtype=torch.int32, device="cuda")
            dk = torch.zeros((nq, K), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            if args.partition > 1:
                run = lambda: g.search_device_partial(nq, dq.data_ptr(), K, w, dk.data_ptr(), dc.data_ptr())  # noqa: E731
            else:
                run = lambda: g.search_device(nq, dq.data_ptr(), K, w, di.data_ptr(), dd.data_ptr(), dc.data_ptr())  # noqa: E731
            for mode in (int(x) for x in args.modes.split(",")):
                g.set_table_mode(mode)
                for _ in range(3):
                    run()
                g.sync()
                g.set_profiling(1)
                win = []
                for _ in range(args.windows):
                    g.reset_stats()
                    for _ in range(args.reps):
                        run()
                    g.sync()
                    win.append(g.get_stats()["scan_ms"] / args.reps)
                st = g.get_stats()
                g.set_profiling(0)
                runs.append({"tool": "w8_dsub_bench", "m": M, "d": d, "dsub": d // M, "kc": KC, "list_len": LIST, "K": K, "nq": nq, "w": w,
                             "probes_per_list": nq * w / KC, "partition": args.partition, "table_mode": mode,
                             "last_striped": st["last_striped"], "kernel": KERNEL.get(st["last_striped"], "?"),
                             "kernel_symbol": kernel_symbol(M, d // M, st["last_striped"]), "qg": st["last_qg"],
                             "chunk": st["last_chunk"], "scan_lds": st["last_scan_lds"], "scan_grid": st["last_scan_grid"],
                             "scan_ms_median": float(np.median(win)), "scan_ms_spread": float(max(win) - min(win)),
                             "scan_ms_windows": [round(x, 4) for x in win]})
                print(json.dumps(runs[-1]), flush=True)
        del g
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/w8_dsub_bench.py", "args": vars(args), "runs": runs}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
