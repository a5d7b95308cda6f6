"""What the seam costs: a search with caller-supplied probes against the plain search, on one GPU.

SIFT1M bench shape (d = 128, m = 8, n = 1e6, kc = 1024, random quantizers and codes -- the scan's cost does not depend on training),
1024 device-resident queries (data-like: a centroid plus noise), K = 10, w = 8.  Three legs, each a whole call sequence per batch,
alternating inside every window, `--reps` batches per leg and window, a host clock around work that ends in a device synchronise:

  (a) ivfadc_search_device                                       the plain search: its plan fuses the top-w selection into the scan
  (b) ivfadc_coarse_search_device + ivfadc_search_device_preassigned   the seam crossed on the device
  (c) ivfadc_search_device_preassigned alone                     the probes are there already (a cached assignment, a router)

What matters is (c) against (a) at the same commit.  The measuring process is ONE child under `timeout`; the parent writes
profiles/preassigned.json (medians of the windows, their spread, and that the three legs returned the same bytes).

    python tools/preassigned_probe.py [--reps 50] [--windows 5] [--limit 300] [--out profiles/preassigned.json]
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

D, M, N, KC, NQ, K, W = 128, 8, 1_000_000, 1024, 1024, 10, 8


def child(reps, windows):
    import torch
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
    dev = torch.device("cuda:0")
    dq = torch.from_numpy(q).to(dev)
    outs = [(torch.zeros(NQ * K, dtype=torch.int32, device=dev), torch.zeros(NQ * K, dtype=torch.float32, device=dev),
             torch.zeros(NQ, dtype=torch.int32, device=dev)) for _ in range(3)]
    cl, cd = torch.zeros(NQ * W, dtype=torch.int32, device=dev), torch.zeros(NQ * W, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    p = lambda o: (o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())  # noqa: E731

    def leg_a():
        g.search_device(NQ, dq.data_ptr(), K, W, *p(outs[0]))

    def leg_b():
        g.coarse_search_device(NQ, dq.data_ptr(), W, cl.data_ptr(), cd.data_ptr())
        g.search_device_preassigned(NQ, dq.data_ptr(), K, W, cl.data_ptr(), cd.data_ptr(), *p(outs[1]))

    def leg_c():
        g.search_device_preassigned(NQ, dq.data_ptr(), K, W, cl.data_ptr(), cd.data_ptr(), *p(outs[2]))

    legs = (("a_search_device", leg_a), ("b_coarse_then_preassigned", leg_b), ("c_preassigned_alone", leg_c))
    forms = {}
    for name, f in legs:          # warm-up: code objects, workspace, LDS attributes
        for _ in range(5):
            f()
        g.sync()
        st = g.get_stats()
        forms[name] = {"last_qg": st["last_qg"], "last_lb": st["last_lb"], "last_scan_lds": st["last_scan_lds"]}
    host = [tuple(t.cpu().numpy() for t in o) for o in outs]
    same = all(np.array_equal(host[0][i], host[j][i]) for j in (1, 2) for i in range(3))
    wins = {name: [] for name, _ in legs}
    for _ in range(windows):
        for name, f in legs:
            g.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            g.sync()
            wins[name].append((time.perf_counter() - t0) / reps * 1e6)
    res = {name: {"us_per_batch_median": float(np.median(v)), "us_per_batch_spread": float(max(v) - min(v)), "form": forms[name]}
           for name, v in wins.items()}
    print(json.dumps({"measurements": res, "same_bytes": bool(same), "reps": reps, "windows": windows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preassigned.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.reps, args.windows)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps),
           "--windows", str(args.windows)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print("[preassigned_probe] the measuring process ended with status %d: nothing written" % r.returncode, file=sys.stderr)
        return r.returncode
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    out = {
        "what": "search with caller-supplied probes against the plain search: tools/preassigned_probe.py --reps %d --windows %d, one bounded "
                "process, the three legs alternating inside every window" % (args.reps, args.windows),
        "shape": "SIFT1M bench shape (d = 128, m = 8, n = 1e6, kc = 1024, random quantizers and codes), 1024 device-resident queries, K = 10, "
                 "w = 8; whole call sequence per batch in microseconds, medians of the windows and their spread (max - min)",
        "status": "measured on one MI355X",
    }
    out.update(rec)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
