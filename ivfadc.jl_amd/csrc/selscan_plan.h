// Planner of the large-K search (ivfadc_set_tuning(h, -4, cap_keys); selscan.hip.h holds the kernel).  Plain C++ (no HIP types), in the
// manner of range_plan.h, so that the arithmetic the host runtime and the kernel share compiles and runs without a GPU
// (tests/c/selscan_plan_check.cpp).
//
// sel_scan_kernel runs ONE workgroup of THREADS lanes per query on a compute unit's whole LDS.  The workgroup buffers the keys of the
// query's probed points (f32 bits of the distance << 32 | visit order, generic.hip.h:1-8) in LDS, finds the K-th smallest with a radix
// select whenever the buffer cannot take another step, and sorts the K survivors once at the end.  The layout, in this order:
//   resid    [d rounded up to 4] f32      the residual of the current probe
//   tab      [m][256] f32                 its ADC table, slot = code label
//   keys     [cap] u64                    the buffered keys; cap a multiple of CAP_ALIGN
//   scratch  [pow2ceil(K)] u64            the survivors of a select round, and what the final bitonic sort runs on
//   hist     [WAVES][256] u32             one radix histogram per wave
//   ctl      CTL_BYTES                    counters and the round's min / max (selscan.hip.h: SelCtl)
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SELSCAN_HD __host__ __device__ __forceinline__
#else
#define SELSCAN_HD inline
#endif

namespace selscan {

// Lanes of a workgroup: eight waves, two per SIMD (DESIGN.md 4.6.10 has the figures this was chosen by).
constexpr int THREADS = 512;
constexpr int WAVES = THREADS / 64;
// points a workgroup takes in one step of the probe loop, at most: two per lane where a 16-byte load holds two points (m = 8)
constexpr int STEP_MAX = 2 * THREADS;
constexpr int CAP_ALIGN = 1024;
// a buffer holds the K survivors of a round and at least one further step (K <= pow2ceil(K) <= cap / 2), whatever K
constexpr int MIN_CAP = 2 * STEP_MAX;
constexpr size_t HIST_BYTES = (size_t)WAVES * 256 * 4;
constexpr size_t CTL_BYTES = 64;

SELSCAN_HD uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }
SELSCAN_HD int pow2ceil(int x) { int p = 1; while (p < x) p <<= 1; return p; }

struct Layout {
    size_t resid = 0, tab = 0, keys = 0, scratch = 0, hist = 0, ctl = 0, end = 0;
};

SELSCAN_HD Layout layout(int d, int m, int K, int64_t cap)
{
    Layout l;
    l.resid = 0;
    l.tab = (size_t)round_up((uint64_t)(d > 0 ? d : 1), 4) * 4;
    l.keys = l.tab + (size_t)(m > 0 ? m : 1) * 256 * 4;
    l.scratch = l.keys + (size_t)cap * 8;
    l.hist = (size_t)round_up(l.scratch + (size_t)pow2ceil(K) * 8, 16);   // (16-byte reads of four bins)
    l.ctl = l.hist + HIST_BYTES;
    l.end = l.ctl + CTL_BYTES;
    return l;
}

// the keys a buffer must hold for the search to be served: the survivors of a round and as many again, and never less than two steps
SELSCAN_HD int64_t cap_needed(int K)
{
    const int64_t twice = 2 * (int64_t)pow2ceil(K);
    return twice > MIN_CAP ? twice : (int64_t)MIN_CAP;
}

// the largest multiple of CAP_ALIGN keys that fits lds_max next to everything else (0: not even one)
SELSCAN_HD int64_t cap_max(int d, int m, int K, size_t lds_max)
{
    const size_t fixed = layout(d, m, K, 0).end;
    if (fixed >= lds_max) return 0;
    return (int64_t)((lds_max - fixed) / 8 / CAP_ALIGN) * CAP_ALIGN;
}

struct Facts {
    int d = 0, kc = 0, m = 0;
    bool u16 = false;
    int max_k = 0, max_w = 0;        // IVFADC_MAX_K, IVFADC_MAX_W
    int force_cap = 0;               // ivfadc_set_tuning's chunk_points under qg = -4 (0: automatic)
    size_t ws_budget = 0;            // ivfadc_set_workspace_limit
    size_t lds_max = 0;              // LDS of a CU a workgroup may take (scan_layouts.h: LDS_MAX)
};

struct Plan {
    bool served = false;
    int64_t cap = 0;                 // keys of the buffer
    size_t lds = 0;                  // dynamic LDS of the launch: the layout's end
    int64_t nb = 0;                  // queries of a sub-batch (>= 1)
    Layout lay;
};

inline Plan make_plan(const Facts &f, int64_t nq, int K, int w)
{
    Plan p;
    if (f.u16 || K < 1 || K > f.max_k || w < 1 || w > f.max_w || f.m < 1 || f.d < 1) return p;
    const int64_t most = cap_max(f.d, f.m, K, f.lds_max), need = cap_needed(K);
    if (most < need) return p;
    int64_t cap = most;
    if (f.force_cap > 0) {
        cap = (int64_t)round_up((uint64_t)f.force_cap, CAP_ALIGN);
        if (cap > most) cap = most;
        if (cap < need) cap = need;   // (need is a multiple of CAP_ALIGN: a power of two >= 2048)
    }
    p.cap = cap;
    p.lay = layout(f.d, f.m, K, cap);
    p.lds = p.lay.end;
    // a query's share of the workspace: its row of coarse distances, its probe arrays (list, distance, base), some slack
    const int64_t per_q = (int64_t)f.kc * 4 + (int64_t)w * 12 + 64;
    int64_t nb = (int64_t)(f.ws_budget / (size_t)per_q);
    if (nb > ((int64_t)1 << 22)) nb = (int64_t)1 << 22;   // kernel arguments are 32-bit
    if (nq > 0 && nb > nq) nb = nq;
    if (nb < 1) nb = 1;
    p.nb = nb;
    p.served = true;
    return p;
}

}  // namespace selscan
