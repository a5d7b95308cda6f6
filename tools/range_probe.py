"""What a range search costs against the only way to the same answer that existed before it, on one GPU.

SIFT1M bench shape (d = 128, m = 8, n = 1e6, kc = 1024, random quantizers and codes -- the scan's cost does not depend on training),
1024 device-resident queries (data-like: a centroid plus noise), w = 8, every query's radius its own 10th-neighbour distance (from a
plain K = 10 search).  Two legs, each a whole call sequence per batch, alternating inside every window, at least `--reps` batches and `--seconds` of work per leg and
window after a warm-up, a host clock around work that ends with the answer in host arrays:

  (a) ivfadc_range_search_device + ivfadc_range_result_copy + _destroy      count, scan, fill, sort the survivors, emit; CSR rows to the host
  (b) ivfadc_search_device with K = the largest probed total, through       dump and sort a key for EVERY probed point, K-strided rows
      ivfadc_set_tuning(h, -2, 0), rows to the host, cut at d <= r there    to the host, the cut in numpy

(b) is the yardstick: there is no earlier number for a new entry.  The device-only parts of both legs (no copy to the host, no cut) are
timed as well.  The measuring process is ONE child under `timeout`; the parent writes the medians of the windows and their spread.

    python tools/range_probe.py [--reps 5] [--windows 5] [--seconds 0.5] [--limit 400] [--out profiles/range_probe.txt]
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


def child(reps, windows, seconds):
    import torch
    import ivfadc_jl_amd as pkg
    from ivfadc_jl_amd import index as ix
    rng = np.random.default_rng(0)
    cent = rng.random((KC, D), dtype=np.float32)
    cbs = ((rng.random((M, 256, D // M), dtype=np.float32) - 0.5) * 0.5).astype(np.float32)
    labels = np.tile(np.arange(256, dtype=np.uint8), (M, 1))
    lst = rng.integers(0, KC, N)
    sizes = np.bincount(lst, minlength=KC)
    offsets = np.zeros(KC + 1, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    codes = rng.integers(0, 256, (N, M)).astype(np.uint8)
    g = pkg.IVFADCIndex.from_arrays(cent, cbs, labels, offsets, codes, np.arange(N, dtype=np.uint32))
    q = (cent[rng.integers(0, KC, NQ)] + rng.normal(0, 0.05, (NQ, D))).astype(np.float32)
    _, d10, c10 = g.search_raw(q, 10, W)
    assert (c10 == 10).all()
    radii = np.ascontiguousarray(d10[:, 9])
    lists, _ = g.coarse_search_raw(q, W)
    K = int(sizes[lists].sum(1).max())                      # the largest probed total: every query's probed points fit K
    dev = torch.device("cuda:0")
    dq, dr = torch.from_numpy(q).to(dev), torch.from_numpy(radii).to(dev)
    oi = torch.zeros(NQ * K, dtype=torch.int32, device=dev)
    od = torch.zeros(NQ * K, dtype=torch.float32, device=dev)
    oc = torch.zeros(NQ, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    last = {}

    def a_device():
        res = g.range_search_device(NQ, dq.data_ptr(), dr.data_ptr(), W)
        ix.range_result_destroy(res)

    def a_full():
        res = g.range_search_device(NQ, dq.data_ptr(), dr.data_ptr(), W)
        last["a"] = ix.range_result_copy(res)
        ix.range_result_destroy(res)

    def b_device():
        g.set_tuning(-2, 0)
        g.search_device(NQ, dq.data_ptr(), K, W, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        g.sync()
        g.set_tuning(0, 0)

    def b_full():
        b_device()
        ids = oi.cpu().numpy().reshape(NQ, K).view(np.uint32)
        dd = od.cpu().numpy().reshape(NQ, K)
        cnt = oc.cpu().numpy()
        keep = (dd <= radii[:, None]) & (np.arange(K)[None, :] < cnt[:, None])
        n = keep.sum(1)
        lims = np.zeros(NQ + 1, np.int64)
        np.cumsum(n, out=lims[1:])
        last["b"] = (lims, ids[keep], dd[keep])             # (rows are sorted: the kept entries of a row are its prefix)

    legs = (("a_range_search_to_host", a_full), ("b_generic_search_all_probed_and_host_cut", b_full),
            ("a_device_only", a_device), ("b_device_only", b_device))
    for _, f in legs:             # warm-up: code objects, workspace, LDS attributes
        for _ in range(2):
            f()
    same = all(np.array_equal(last["a"][i], last["b"][i]) for i in range(3))
    nrep = {}
    for name, f in legs:          # a window holds at least `reps` batches and about `seconds` of work
        g.sync()
        t0 = time.perf_counter()
        f()
        g.sync()
        nrep[name] = max(reps, int(np.ceil(seconds / max(time.perf_counter() - t0, 1e-6))))
    wins = {name: [] for name, _ in legs}
    for _ in range(windows):
        for name, f in legs:
            g.sync()
            t0 = time.perf_counter()
            for _ in range(nrep[name]):
                f()
            g.sync()
            wins[name].append((time.perf_counter() - t0) / nrep[name] * 1e3)
    res = {name: {"ms_per_batch_median": float(np.median(v)), "ms_per_batch_spread": float(max(v) - min(v)), "batches_per_window": nrep[name]} for name, v in wins.items()}
    print(json.dumps({"measurements": res, "same_answer": bool(same), "results_per_batch": int(last["a"][0][-1]), "K_of_leg_b": K,
                      "keys_written_by_leg_b": int(sizes[lists].sum()), "reps": reps, "windows": windows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5, help="work a window holds, at least (and at least --reps batches)")
    ap.add_argument("--limit", type=int, default=400, help="seconds the measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_probe.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.reps, args.windows, args.seconds)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps),
           "--windows", str(args.windows), "--seconds", str(args.seconds)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print("[range_probe] the measuring process ended with status %d: nothing written" % r.returncode, file=sys.stderr)
        return r.returncode
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    lines = ["range search against the generic search over every probed point: tools/range_probe.py --reps %d --windows %d --seconds %g" % (args.reps, args.windows, args.seconds),
             "SIFT1M bench shape (d = 128, m = 8, n = 1e6, kc = 1024, random quantizers and codes), 1024 device-resident queries, w = 8,",
             "radius of a query = its own 10th-neighbour distance; one MI355X, one bounded process, legs alternating inside every window;",
             "milliseconds per batch, median of the windows (spread = max - min)", ""]
    for name, v in rec["measurements"].items():
        lines.append("%-44s %9.3f ms  (spread %.3f, %d batches a window)" % (name, v["ms_per_batch_median"], v["ms_per_batch_spread"], v["batches_per_window"]))
    lines += ["", "same answer (lims, ids, distance bits): %s" % rec["same_answer"],
              "results per batch: %d; keys leg (b) writes and sorts: %d (K = %d)" % (rec["results_per_batch"], rec["keys_written_by_leg_b"], rec["K_of_leg_b"]),
              json.dumps(rec)]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
