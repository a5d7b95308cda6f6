"""What a masked range search costs against the only earlier way to the same bytes, on one GPU.

8-bit legs: SIFT1M bench shape (d = 128, m = 8, n = 1e6, kc = 1024, random quantizers and codes), 1024 device-resident queries (a
centroid plus noise), w = 8, ONE set of 16 masks at selectivities 1.0, 0.5 and 0.01 (mask r has selectivity SEL[r % 3]; query q carries
mask q % 16), every query's radius its own 10th MASKED neighbour's distance (from a K = 10 masked search).

  (1) ivfadc_range_search_device_masked + ivfadc_range_result_copy + _destroy
  (2) ivfadc_search_device_masked with K = the largest probed total (the masked generic path), rows to the host, cut at d <= r there:
      the only way to the same bytes before this entry.  lims, ids and distance bits of (1) and (2) are ASSERTED equal before timing.
  (3) every query on a selectivity-1.0 mask, against the plain ivfadc_range_search_device on the same radii: the price of the mask words.

UInt16 legs: tools/u16_bench.py's SIFT1M k = 1024 shape, no mask set, radius = the 10th-neighbour distance.

  (4) ivfadc_range_search_device_masked(set = NULL) + copy, against ivfadc_search_device through set_tuning(-2, 0) with K = the largest
      probed total and the cut on the host; asserted equal before timing.

Each group (8-bit, UInt16) is ONE child process under `timeout`; inside it the legs alternate in every window, after a warm-up, a host
clock around work that ends with a synchronise (the range entries block) and the answer in host arrays.  The parent writes the medians
of the windows, their fastest and slowest window and their spread (max - min), and says "not measured" for a group whose child did not finish.

    python tools/range_masked_probe.py [--reps 5] [--windows 5] [--seconds 0.5] [--limit 500] [--out profiles/range_masked_probe.txt]
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
SEL = (1.0, 0.5, 0.01)
NMASKS = 16


def build(ksub, code_t):
    import ivfadc_jl_amd as pkg
    rng = np.random.default_rng(0)
    cent = rng.random((KC, D), dtype=np.float32)
    cbs = ((rng.random((M, ksub, D // M), dtype=np.float32) - 0.5) * 0.5).astype(np.float32)
    labels = np.tile(np.arange(ksub, dtype=code_t), (M, 1))
    lst = rng.integers(0, KC, N)
    sizes = np.bincount(lst, minlength=KC)
    offsets = np.zeros(KC + 1, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    codes = rng.integers(0, ksub, (N, M)).astype(code_t)
    g = pkg.IVFADCIndex.from_arrays(cent, cbs, labels, offsets, codes, np.arange(N, dtype=np.uint32))
    q = (cent[rng.integers(0, KC, NQ)] + rng.normal(0, 0.05, (NQ, D))).astype(np.float32)
    return g, q, sizes, rng


def host_cut(ids, dd, cnt, radii, K):
    keep = (dd <= radii[:, None]) & (np.arange(K)[None, :] < cnt[:, None])
    lims = np.zeros(len(radii) + 1, np.int64)
    np.cumsum(keep.sum(1), out=lims[1:])
    return lims, ids[keep], dd[keep]                        # (rows are sorted: the kept entries of a row are its prefix)


def same(a, b):
    return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))


def run_legs(g, legs, reps, windows, seconds):
    for _, f in legs:             # warm-up: code objects, workspace, LDS attributes
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
    return {name: {"ms_per_batch_median": float(np.median(v)), "ms_per_batch_spread": float(max(v) - min(v)), "ms_per_batch_min": float(min(v)),
                   "ms_per_batch_max": float(max(v)), "batches_per_window": nrep[name]}
            for name, v in wins.items()}


def child_u8(reps, windows, seconds):
    import torch
    from ivfadc_jl_amd import index as ix
    g, q, sizes, rng = build(256, np.uint8)
    masks = [np.ones(N, bool) if SEL[r % 3] >= 1.0 else rng.random(N) < SEL[r % 3] for r in range(NMASKS)]
    ms = g.maskset(masks=masks)
    moq = (np.arange(NQ) % NMASKS).astype(np.int32)
    _, d10, c10 = g.search_masked_raw(q, 10, ms, moq, w=W)
    assert (c10 >= 1).all(), "a query has no selected point among its probes"
    radii = np.ascontiguousarray(d10[np.arange(NQ), c10 - 1])
    lists, _ = g.coarse_search_raw(q, W)
    K = int(sizes[lists].sum(1).max())                      # the largest probed total
    dev = torch.device("cuda:0")
    all_r = [r for r in range(NMASKS) if SEL[r % 3] >= 1.0]
    moq1 = np.array([all_r[i % len(all_r)] for i in range(NQ)], np.int32)
    dq, dr, dm, dm1 = (torch.from_numpy(a).to(dev) for a in (q, radii, moq, moq1))
    oi = torch.zeros(NQ * K, dtype=torch.int32, device=dev)
    od = torch.zeros(NQ * K, dtype=torch.float32, device=dev)
    oc = torch.zeros(NQ, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    last = {}

    def leg1():
        res = g.range_search_device_masked(NQ, dq.data_ptr(), dr.data_ptr(), ms, dm.data_ptr(), W)
        last["1"] = ix.range_result_copy(res)
        ix.range_result_destroy(res)

    def leg2():
        g.search_device_masked(ms, NQ, dq.data_ptr(), K, W, dm.data_ptr(), oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        g.sync()
        last["2"] = host_cut(oi.cpu().numpy().reshape(NQ, K).view(np.uint32), od.cpu().numpy().reshape(NQ, K), oc.cpu().numpy(), radii, K)

    def leg3_masked():
        res = g.range_search_device_masked(NQ, dq.data_ptr(), dr.data_ptr(), ms, dm1.data_ptr(), W)
        last["3m"] = ix.range_result_copy(res)
        ix.range_result_destroy(res)

    def leg3_plain():
        res = g.range_search_device(NQ, dq.data_ptr(), dr.data_ptr(), W)
        last["3p"] = ix.range_result_copy(res)
        ix.range_result_destroy(res)

    legs = (("1_masked_range_search_to_host", leg1), ("2_masked_generic_search_all_probed_and_host_cut", leg2),
            ("3_masked_range_search_selectivity_1", leg3_masked), ("3_plain_range_search", leg3_plain))
    for _, f in legs:
        f()
    assert same(last["1"], last["2"]), "legs 1 and 2 differ in lims, ids or distance bits"
    assert same(last["3m"], last["3p"]), "a selectivity-1.0 mask changes the plain range search's bytes"
    res = run_legs(g, legs, reps, windows, seconds)
    per_sel = {str(s): int(sum(last["1"][0][i + 1] - last["1"][0][i] for i in range(NQ) if SEL[moq[i] % 3] == s)) for s in SEL}
    print(json.dumps({"group": "u8", "measurements": res, "same_answer_1_2": True, "same_answer_3": True, "results_per_batch": int(last["1"][0][-1]),
                      "results_per_selectivity": per_sel, "results_per_batch_leg3": int(last["3p"][0][-1]), "K_of_leg_2": K,
                      "keys_written_by_leg_2": int(sizes[lists].sum()), "kept": [int(k) for k in ms.kept]}))


def child_u16(reps, windows, seconds):
    import torch
    from ivfadc_jl_amd import index as ix
    g, q, sizes, _ = build(1024, np.uint16)
    _, d10, c10 = g.search_raw(q, 10, W)
    assert (c10 == 10).all()
    radii = np.ascontiguousarray(d10[:, 9])
    lists, _ = g.coarse_search_raw(q, W)
    K = int(sizes[lists].sum(1).max())
    dev = torch.device("cuda:0")
    dq, dr = torch.from_numpy(q).to(dev), torch.from_numpy(radii).to(dev)
    oi = torch.zeros(NQ * K, dtype=torch.int32, device=dev)
    od = torch.zeros(NQ * K, dtype=torch.float32, device=dev)
    oc = torch.zeros(NQ, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    last = {}

    def leg4_range():
        res = g.range_search_device_masked(NQ, dq.data_ptr(), dr.data_ptr(), None, 0, W)
        last["r"] = ix.range_result_copy(res)
        ix.range_result_destroy(res)

    def leg4_generic():
        g.set_tuning(-2, 0)
        g.search_device(NQ, dq.data_ptr(), K, W, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        g.sync()
        g.set_tuning(0, 0)
        last["g"] = host_cut(oi.cpu().numpy().reshape(NQ, K).view(np.uint32), od.cpu().numpy().reshape(NQ, K), oc.cpu().numpy(), radii, K)

    legs = (("4_u16_range_search_no_set_to_host", leg4_range), ("4_u16_generic_search_all_probed_and_host_cut", leg4_generic))
    for _, f in legs:
        f()
    assert same(last["r"], last["g"]), "the UInt16 legs differ in lims, ids or distance bits"
    res = run_legs(g, legs, reps, windows, seconds)
    print(json.dumps({"group": "u16", "measurements": res, "same_answer_4": True, "results_per_batch": int(last["r"][0][-1]), "K_of_generic_leg": K,
                      "keys_written_by_generic_leg": int(sizes[lists].sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5, help="work a window holds, at least (and at least --reps batches)")
    ap.add_argument("--limit", type=int, default=500, help="seconds one measuring process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_masked_probe.txt"))
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child:
        return {"u8": child_u8, "u16": child_u16}[args.child](args.reps, args.windows, args.seconds)
    lines = ["masked range search against the masked generic search over every probed point: tools/range_masked_probe.py --reps %d --windows %d --seconds %g"
             % (args.reps, args.windows, args.seconds),
             "SIFT1M bench shape (d = 128, m = 8, n = 1e6, kc = 1024, random quantizers and codes), 1024 device-resident queries, w = 8;",
             "8-bit: one set of 16 masks at selectivities 1.0 / 0.5 / 0.01, radius of a query = its own 10th masked neighbour's distance;",
             "UInt16: k = 1024, no mask set, radius = the 10th-neighbour distance; one MI355X, one bounded process per group, legs alternating",
             "inside every window; milliseconds per batch, median of the windows, fastest .. slowest window (spread = max - min)", ""]
    status = 0
    for group in ("u8", "u16"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", group, "--reps", str(args.reps),
               "--windows", str(args.windows), "--seconds", str(args.seconds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            lines += ["group %s: NOT MEASURED (the measuring process ended with status %d)" % (group, r.returncode), ""]
            status = r.returncode
            break                 # nothing more is started on the GPU after a process that did not end well
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        for name, v in rec["measurements"].items():
            lines.append("%-52s %9.3f ms  (windows %.3f .. %.3f, spread %.3f, %d batches a window)"
                         % (name, v["ms_per_batch_median"], v["ms_per_batch_min"], v["ms_per_batch_max"], v["ms_per_batch_spread"], v["batches_per_window"]))
        lines += ["same answer (lims, ids, distance bits) asserted before timing: True", json.dumps(rec), ""]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return status


if __name__ == "__main__":
    sys.exit(main())
