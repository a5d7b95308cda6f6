"""How long does a subset view take to make?  (ivfadc_clone_subset; csrc/subset.hip.h)

One process, the SIFT1M shape (n = 10^6, d = 128, kc = 1024, m = 8, random quantizers and lists).  After a warm-up, at selectivities
0.01, 0.5 and 1.0: the median of REPS creations with device events around each (the index runs on torch's stream for that, so the events
enclose the two kernels, the memset, the table uploads and the one blocking copy of the item counts in between), next to the bytes of
DESIGN.md's formula, 4n + n (4 + cs) + kept (4 + cs) + the bitmap, over that time.  In the same run, the route that existed before:
get_lists, a numpy filter, a new handle and set_lists (wall clock, the handle's creation included -- it uploads the quantizers and
derives their tables again).  Prints one JSON line; 6.29 TB/s is the copy ceiling the figures stand beside, not a target.

    python tools/subset_probe.py [--reps 25] [--out profiles/subset_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.reps >= 20, "medians of at least 20 creations"
    import ctypes as C
    import torch
    import ivfadc_jl_amd as pkg
    from ivfadc_jl_amd import _native as nat, index as ix
    n, d, kc, m, ksub, cs = a.n, 128, 1024, 8, 256, 8
    rng = np.random.default_rng(1)
    cent = rng.random((kc, d), dtype=np.float32)
    cbs = ((rng.random((m, ksub, d // m), dtype=np.float32) - 0.5) * 0.5).astype(np.float32)
    labels = np.tile(np.arange(ksub, dtype=np.uint8), (m, 1))
    lst = np.sort(rng.integers(0, kc, n))
    offsets = np.zeros(kc + 1, np.int64)
    np.cumsum(np.bincount(lst, minlength=kc), out=offsets[1:])
    codes = rng.integers(0, 256, (n, m), dtype=np.uint8)
    ids = rng.permutation(n).astype(np.uint32)
    g = pkg.IVFADCIndex.from_arrays(cent, cbs, labels, offsets, codes, ids)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    qs = rng.random((256, d), dtype=np.float32)
    g.search_raw(qs, 10, 8)
    out = {"shape": dict(n=n, d=d, kc=kc, m=m, cs=cs), "reps": a.reps, "copy_ceiling_GBps": 6290.0, "selectivity": {}}
    for p in (0.01, 0.5, 1.0):
        mask = rng.random(n) < p if p < 1.0 else np.ones(n, bool)
        words, nbits = ix.pack_bitmap(mask=mask)           # packed once: the events enclose the native call alone
        make = lambda: g._subset(nat.lib().ivfadc_clone_subset, nat.ptr(words, C.c_uint32), nbits)
        for _ in range(3):
            make()
        ms, wall = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            v = make()
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(e0.elapsed_time(e1))
            kept = len(v)
            del v
        # the route that existed before: mirror out, filter on the host, a second full handle
        old = []
        for _ in range(3):
            t0 = time.perf_counter()
            g._mirror = None
            o, c, i = g._lists()
            keep = mask[i]
            no = np.zeros(kc + 1, np.int64)
            np.cumsum([int(keep[o[l]:o[l + 1]].sum()) for l in range(kc)], out=no[1:])
            h = pkg.IVFADCIndex.from_arrays(cent, cbs, labels, no, c[keep], i[keep])
            h.sync()
            old.append((time.perf_counter() - t0) * 1e3)
            assert len(h) == kept
            del h
        formula = 4 * n + n * (4 + cs) + kept * (4 + cs) + (n + 31) // 32 * 4
        med = float(np.median(ms))
        out["selectivity"][str(p)] = dict(kept=kept, device_ms_median=round(med, 4), device_ms_min=round(float(min(ms)), 4),
                                          wall_ms_median=round(float(np.median(wall)), 4),
                                          formula_bytes=formula, formula_GBps=round(formula / med / 1e6, 1),
                                          host_route_ms_median=round(float(np.median(old)), 2))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
