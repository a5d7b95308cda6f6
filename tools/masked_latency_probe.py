"""What the latency path of the masked search (ivfadc_set_masked_latency(h, 1)) costs a call against the path it
leaves alone and against the plain search of the same queries, on one GPU.

SIFT1M bench shape (d = 128, m = 8, n = 1e6, kc = 1024, random quantizers and codes), device-resident queries (a centroid plus noise),
the device entries, K = 10, w = 8.  nq in 1, 8, 64; one mask set of four masks: uniform at selectivity 1.0, 0.1 and 0.01, and one that
selects the entries of 8 cells only (0.8 % of the index, clustered).  Every query of a batch carries the same mask.

  off      ivfadc_search_device_masked with the setting off: coarse, top-w, masked_scan_kernel, merge -- the yardstick
  on       the same call with the setting on: sq_masked_kernel behind the coarse launch
  plain    ivfadc_search_device of the same queries, no mask: the plain latency path, the floor of the launch chain

Before anything is timed `on` and `off` are ASSERTED to return the same bytes at every point of the grid.  One child process under
`timeout`; after a warm-up the legs alternate inside every window, a host clock around calls that end with a synchronise on both
sides; a call is enqueue + synchronise, as an online caller sees it.  The parent writes the medians of the windows with their fastest
and slowest, and says "not measured" if the child did not finish.

    python tools/masked_latency_probe.py [--reps 20] [--windows 7] [--seconds 0.25] [--limit 400] [--out profiles/masked_latency_probe.txt]
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

D, M, N, KC, K, W = 128, 8, 1_000_000, 1024, 10, 8
NQS = (1, 8, 64)
MASKS = ("uniform 1.0", "uniform 0.1", "uniform 0.01", "8 cells")


def build():
    import ivfadc_jl_amd as pkg
    rng = np.random.default_rng(0)
    cent = rng.random((KC, D), dtype=np.float32)
    cbs = ((rng.random((M, 256, D // M), dtype=np.float32) - 0.5) * 0.5).astype(np.float32)
    labels = np.tile(np.arange(256, dtype=np.uint8), (M, 1))
    lst = np.sort(rng.integers(0, KC, N))                   # ids in list order: id i lies in cell lst[i]
    offsets = np.zeros(KC + 1, np.int64)
    np.cumsum(np.bincount(lst, minlength=KC), out=offsets[1:])
    codes = rng.integers(0, 256, (N, M)).astype(np.uint8)
    g = pkg.IVFADCIndex.from_arrays(cent, cbs, labels, offsets, codes, np.arange(N, dtype=np.uint32))
    cells = rng.integers(0, KC, max(NQS))
    q = (cent[cells] + rng.normal(0, 0.05, (max(NQS), D))).astype(np.float32)
    masks = [np.ones(N, bool), rng.random(N) < 0.1, rng.random(N) < 0.01, np.isin(lst, cells[:8])]
    return g, q, g.maskset(masks=masks)


def windows_of(g, legs, reps, windows, seconds):
    for _, f in legs:
        for _ in range(3):
            f()
    nrep = {}
    for name, f in legs:
        g.sync()
        t0 = time.perf_counter()
        f()
        nrep[name] = max(reps, int(np.ceil(seconds / max(time.perf_counter() - t0, 1e-6))))
    wins = {name: [] for name, _ in legs}
    for _ in range(windows):
        for name, f in legs:
            g.sync()
            t0 = time.perf_counter()
            for _ in range(nrep[name]):
                f()
            wins[name].append((time.perf_counter() - t0) / nrep[name] * 1e6)
    return {name: {"us_median": float(np.median(v)), "us_min": float(min(v)), "us_max": float(max(v)), "calls_per_window": nrep[name]}
            for name, v in wins.items()}


def child(reps, windows, seconds):
    import torch
    g, q, ms = build()
    dev = torch.device("cuda:0")
    dq = torch.from_numpy(q).to(dev)
    nqm = max(NQS)
    outs = {n: (torch.zeros((nqm, K), dtype=torch.int32, device=dev), torch.zeros((nqm, K), dtype=torch.float32, device=dev),
                torch.zeros(nqm, dtype=torch.int32, device=dev)) for n in ("off", "on", "plain")}
    torch.cuda.synchronize()
    rec = {}
    for r, mname in enumerate(MASKS):
        moq = torch.full((nqm,), r, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for nq in NQS:
            def masked(which, nq=nq, moq=moq):
                o = outs[which]
                g.set_masked_latency(1 if which == "on" else 0)
                g.search_device_masked(ms, nq, dq.data_ptr(), K, W, moq.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
                g.sync()

            def plain(nq=nq):
                o = outs["plain"]
                g.search_device(nq, dq.data_ptr(), K, W, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
                g.sync()

            masked("off")
            qg_off = g.get_stats()["last_qg"]
            masked("on")
            assert g.get_stats()["last_qg"] == -3 and qg_off != -3
            a, b = ([t[:nq].cpu().numpy() for t in outs[n]] for n in ("off", "on"))
            assert np.array_equal(a[2], b[2]), "counts differ"
            for i in range(nq):
                c = int(a[2][i])
                assert np.array_equal(a[0][i, :c], b[0][i, :c]) and np.array_equal(a[1][i, :c].view(np.uint32), b[1][i, :c].view(np.uint32)), (mname, nq, i)
            legs = (("off", lambda: masked("off")), ("on", lambda: masked("on")), ("plain", plain))
            rec["%s|%d" % (mname, nq)] = windows_of(g, legs, reps, windows, seconds)
    g.set_masked_latency(0)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--seconds", type=float, default=0.25, help="work a window holds, at least (and at least --reps calls)")
    ap.add_argument("--limit", type=int, default=400, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_latency_probe.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.reps, args.windows, args.seconds)
    lines = ["masked search of a handful of queries, the latency path off / on, and the plain search: tools/masked_latency_probe.py --reps %d "
             "--windows %d --seconds %g" % (args.reps, args.windows, args.seconds),
             "SIFT1M bench shape (d = 128, m = 8, n = 1e6, kc = 1024, random quantizers and codes), device entries, K = %d, w = %d; one MI355X, one" % (K, W),
             "bounded process, legs alternating inside every window; microseconds per call (enqueue + synchronise), median of the windows",
             "(fastest .. slowest)", ""]
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps),
           "--windows", str(args.windows), "--seconds", str(args.seconds)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    status = r.returncode
    if status != 0:
        lines += ["NOT MEASURED (the measuring process ended with status %d)" % status, ""]
    else:
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        lines.append("%-14s %3s  %-28s %-28s %-28s %s" % ("mask", "nq", "off", "on", "plain", "on / off"))
        for key, legs in rec.items():
            mname, nq = key.split("|")
            cell = lambda v: "%8.1f (%.1f .. %.1f)" % (v["us_median"], v["us_min"], v["us_max"])
            lines.append("%-14s %3s  %-28s %-28s %-28s %.2f" % (mname, nq, cell(legs["off"]), cell(legs["on"]), cell(legs["plain"]),
                                                             legs["on"]["us_median"] / legs["off"]["us_median"]))
        lines += ["", "same bytes from `on` and `off` asserted at every point before timing: True", json.dumps(rec), ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return status


if __name__ == "__main__":
    sys.exit(main())
