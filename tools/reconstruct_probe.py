"""What ivfadc_locate costs, and what pop! costs with it, on one GPU.

Locate.  Device-synthesised lists (m = 8, kc = 1024, equal lists) carry no id array -- the id is the position -- so the pass is measured on
a SUBSET VIEW of them that keeps everything: the same lists with a stored id array, 4 bytes per entry to stream.  Two sizes, n = 1e6 and
n = 2^28 (1 GB of ids; the largest that leaves the probe quick), and wanted sets of 1, 1 024 and 163 840 distinct stored ids.  Per case:

  host     wall time of ivfadc_locate (sort on the host, upload, ONE pass behind the exact bitmap -- the ids span less than 2^30 --, the
           locations back), median of `--reps` calls
  device   HIP-event time of ivfadc_locate_device on the caller's stream (radix sort, ONE pass -- behind the hashed LDS filter up to
           16 384 wanted ids, behind a bitmap over the ids' own span, read on the device and zeroed first, beyond --, resolve), median of `--reps` calls; bytes
           streamed = 4 n; the rate against the measured copy ceiling (6.29 TB/s)

Pop.  n = 1e6 stored points (ids shuffled, kc = 1024, d = 128, m = 8): wall time of pop(index), median of `--pops` calls, each followed by a
push of the popped vector's id back so that the index keeps its size.  `--package-root DIR` imports the package from another tree (the
parent commit's, built there), which is how the two commits are compared on one machine.

    python tools/reconstruct_probe.py [--reps 7] [--pops 7] [--big 28] [--package-root DIR] [--skip-locate] [--out profiles/reconstruct_probe.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_CEILING_TBS = 6.29
D, M, KC = 128, 8, 1024
FILTER_MAX_WANTED = 16384         # csrc/reconstruct_plan.h: the LDS filter's cap


def quantizers(rng):
    cent = rng.random((KC, D), dtype=np.float32)
    cbs = ((rng.random((M, 256, D // M), dtype=np.float32) - 0.5) * 0.5).astype(np.float32)
    labels = np.tile(np.arange(256, dtype=np.uint8), (M, 1))
    return cent, cbs, labels


def median(xs):
    return float(np.median(np.asarray(xs, np.float64)))


def locate_cases(pkg, n, reps, out):
    import torch
    rng = np.random.default_rng(1)
    g = pkg.IVFADCIndex.from_arrays(*quantizers(rng))
    offsets = (np.arange(KC + 1, dtype=np.int64) * n) // KC
    g.synth_lists(offsets, 7)
    s = g.subset(mask=np.ones(n, bool))                     # the same lists with an id array of their own
    assert len(s) == n
    dev = torch.device("cuda:0")
    s.set_stream(torch.cuda.current_stream().cuda_stream)
    for nwant in (1, 1024, 163840):
        want = rng.choice(n, nwant, replace=False).astype(np.uint32)
        lists, pos = s.locate_raw(want)                     # warm-up, and the answer: id = global position on these lists
        assert np.array_equal(offsets[lists] + pos, want.astype(np.int64)), "locate is wrong on the probe's own lists"
        host = []
        for _ in range(reps):
            t0 = time.perf_counter()
            s.locate_raw(want)
            host.append((time.perf_counter() - t0) * 1e3)
        dw = torch.from_numpy(want.view(np.int32)).to(dev)
        dl = torch.zeros(nwant, dtype=torch.int32, device=dev)
        dp = torch.zeros(nwant, dtype=torch.int64, device=dev)
        s.locate_device(nwant, dw.data_ptr(), dl.data_ptr(), dp.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(dl.cpu().numpy(), lists) and np.array_equal(dp.cpu().numpy(), pos)
        devms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            s.locate_device(nwant, dw.data_ptr(), dl.data_ptr(), dp.data_ptr())
            b.record()
            torch.cuda.synchronize()
            devms.append(a.elapsed_time(b))
        mode = "hashed LDS filter" if nwant <= FILTER_MAX_WANTED else "bitmap over the span the kernels read from the sorted ids"
        streamed = 4 * n
        hm, dm = median(host), median(devms)
        rate = streamed / (dm * 1e-3) / 1e12
        out.append("locate n=%d wanted=%d: %d id bytes; host entry (bitmap over the span) %.3f ms wall [min %.3f]: its pass streams at %.3f TB/s "
                   "or more; device entry (%s) %.3f ms [min %.3f] = %.3f TB/s = %.1f %% of the %.2f TB/s copy ceiling"
                   % (n, nwant, streamed, hm, min(host), 4 * n / (min(host) * 1e-3) / 1e12, mode, dm, min(devms), rate,
                      100 * rate / COPY_CEILING_TBS, COPY_CEILING_TBS))
        print(out[-1], flush=True)


def pop_case(pkg, pops, out, label):
    rng = np.random.default_rng(2)
    n = 1_000_000
    cent, cbs, labels = quantizers(rng)
    lst = rng.integers(0, KC, n)
    sizes = np.bincount(lst, minlength=KC)
    offsets = np.zeros(KC + 1, np.int64)
    np.cumsum(sizes, out=offsets[1:])
    codes = rng.integers(0, 256, (n, M)).astype(np.uint8)
    g = pkg.IVFADCIndex.from_arrays(cent, cbs, labels, offsets, codes, rng.permutation(n).astype(np.uint32))
    g.search_raw(cent[:1], 1, 1)                            # the device layout is current
    times = []
    for i in range(pops + 1):
        t0 = time.perf_counter()
        rec = pkg.pop(g)
        dt = (time.perf_counter() - t0) * 1e3
        if i:                                               # (the first call warms up)
            times.append(dt)
        pkg.push(g, rec)                                    # back to n points
        assert len(g) == n
    out.append("pop n=%d (%s): %.3f ms wall per call, median of %d [min %.3f, max %.3f]" % (n, label, median(times), pops, min(times), max(times)))
    print(out[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pops", type=int, default=7)
    ap.add_argument("--big", type=int, default=28, help="log2 of the large index's size")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--skip-locate", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import ivfadc_jl_amd as pkg
    out = []
    if not args.skip_locate:
        for n in (1_000_000, 1 << args.big):
            locate_cases(pkg, n, args.reps, out)
    pop_case(pkg, args.pops, out, args.label)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
