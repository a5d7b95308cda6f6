// selscan.hip.h -- the large-K search (ivfadc_set_tuning(h, -4, cap_keys); planned by selscan_plan.h): 64 < K <= 2048 is where it is
// meant to be used, every 1 <= K <= IVFADC_MAX_K is served.
//
// Semantics: generic.hip.h:1-8.  Every probed point has the key f32_bits(distance) << 32 | visit order, the distance is dc, then
// t0 .. t(m-1) added in ascending order with one Float32 rounding per operation; the result is the K smallest keys, ascending.
//
// The selection kernels keep a query's K best in per-wave selectors that are re-sorted every hundred accepted candidates: right for
// K <= 64, wrong where a query keeps an eighth of what it probes.  Here ONE workgroup of selscan::THREADS lanes owns a query and a
// compute unit's whole LDS (selscan::Layout):
//   probe loop   per probe, in ascending dc: residual, ADC table (build_tables_t: the entries' bits are the other kernels'), then the
//                list's code rows in steps of THREADS x PPT points -- 16-byte loads, two points per lane at m = 8, one at m = 16, dwords at
//                the code stride otherwise.  A lane forms its points' keys; keys below the bound (KEY_MAX until the first round) are
//                appended to the key buffer with one LDS atomic per wave: ballot, lane prefix from mbcnt, one ds_add of the popcount.
//   select round when the buffer cannot take another step (and, to get a bound early, at a probe's start once it holds 2 K keys and at
//                least EARLY_MIN): the K-th smallest key T of the cnt buffered keys by an MSB-first radix select over the 64-bit key,
//                8-bit digits, one histogram per wave; the leading digits on which all keys agree are skipped (clz(min ^ max): the
//                distances of a query share their exponent bits).  Keys are unique (the low word is the visit order), so exactly K keys
//                are <= T: they are compacted through the scratch to the front of the buffer and T is the bound.  Later candidates are
//                tested with key < bound; a key that fails lies above K buffered keys and cannot enter the result, so nothing is lost.
//   pruning      ivfadc_set_pruning: a point's sum starts from dc and every table entry is >= +0, so its key is >= f32_bits(dc) << 32;
//                once that lies above the bound no point of this list, nor of a later one (ascending dc), is below it: the query ends.
//   finish       a last round if cnt > K, a bitonic sort of the survivors over pow2ceil(count) keys in the scratch, and ids,
//                distances and counts written the way gen_emit_kernel writes them (emit_result).
// Results cannot depend on when rounds run: every round keeps exactly the K smallest of the keys seen so far.
#pragma once
#include "kernels.hip.h"
#include "selscan_plan.h"

namespace ivf {

struct SelScanArgs {
    IndexView ix;
    const float *queries;
    int w, K;
    u32 cap;                  // keys of the buffer (selscan::Plan::cap)
    const int *probe_list;    // [nq][w], ascending dc (the stand-alone coarse stage: topw_select_kernel, twolevel_topw_kernel)
    const float *probe_dc;
    const u32 *probe_base;    // visit-order base of each probe
    u32 *out_ids;
    float *out_dists;
    int *out_counts;
    u64 *scanned_points;      // word 8 (q & 63) + 1 counts the points pruning skipped (the coarse stage counted the probed ones)
    int prune;
};

struct SelCtl {
    u32 cnt;     // keys in the buffer
    u32 scnt;    // survivors compacted so far (0 between rounds)
    u64 kmin, kmax;   // smallest / largest buffered key of the round under way (KEY_MAX / 0 between rounds)
};
static_assert(sizeof(SelCtl) <= selscan::CTL_BYTES, "the control words fit their block");

// a bound exists from this many buffered keys on, at a probe's start (with 2 K): below, a round costs more than the bound saves
constexpr u32 SEL_EARLY_MIN = 1024;

// position of every lane's entry among the set bits of a wave's ballot
static __device__ __forceinline__ u32 sel_lane_prefix(u64 mask)
{
    return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
}

// One select round.  In: buf[0 .. cnt) are the buffered keys, cnt > K, uniform, every append visible (the caller stands behind a
// barrier).  Out: buf[0 .. K) and scr[0 .. K) hold the K smallest in no particular order, ctl->cnt == K, behind a barrier; returns the
// K-th smallest key.
static __device__ u64 sel_round(u64 *buf, u64 *scr, u32 *hist, SelCtl *ctl, u32 cnt, int K, int tid)
{
    constexpr int NT = selscan::THREADS;
    const int lane = tid & 63, wv = tid >> 6;
    u64 mn = KEY_MAX, mx = 0;
    for (u32 i = tid; i < cnt; i += NT) {
        const u64 k = buf[i];
        mn = k < mn ? k : mn;
        mx = k > mx ? k : mx;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 a = __shfl_xor(mn, off), b = __shfl_xor(mx, off);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if (lane == 0) {
        atomicMin((unsigned long long *)&ctl->kmin, mn);
        atomicMax((unsigned long long *)&ctl->kmax, mx);
    }
    __syncthreads();
    mn = ctl->kmin;
    mx = ctl->kmax;
    // the digit that holds the highest bit in which two keys differ (cnt >= 2 unique keys: mn != mx); everything above it is common
    int shift = (63 - __clzll((long long)(mn ^ mx))) & ~7;
    u64 himask = shift + 8 >= 64 ? 0ull : ~0ull << (shift + 8);
    u64 prefix = mn & himask;
    u32 rank = (u32)K - 1u;   // the wanted key's rank among the keys that match the prefix
    u32 *myhist = hist + wv * 256;
    for (; shift >= 0; shift -= 8) {
        // a wave's keys (i = tid, tid + NT, ...) count into its own histogram: clear and count need no barrier between them
        for (int e = lane; e < 256; e += 64) myhist[e] = 0u;
        wave_sync();
        for (u32 i = tid; i < cnt; i += NT) {
            const u64 k = buf[i];
            if ((k & himask) == prefix) atomicAdd(&myhist[(u32)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        // every wave finds the digit for itself: lane l sums bins 4 l .. 4 l + 3 over the waves, a wave prefix locates the rank
        u32 c[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int g = 0; g < selscan::WAVES; ++g) {
            const uint4 v = *(const uint4 *)(hist + g * 256 + 4 * lane);
            c[0] += v.x; c[1] += v.y; c[2] += v.z; c[3] += v.w;
        }
        const u32 s = c[0] + c[1] + c[2] + c[3];
        u32 incl = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const u32 o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        u32 below = incl - s;
        const bool hit = below <= rank && rank < incl;   // exactly one lane: the counts of the matching keys add up to more than rank
        u32 digit = 4u * (u32)lane;   // (the hit lane's: its first bin whose running count passes the rank)
        bool found = false;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            found = found || rank < below + c[b];
            if (!found) { below += c[b]; ++digit; }
        }
        const int src = __ffsll((long long)__ballot(hit)) - 1;
        digit = (u32)__shfl((int)digit, src);
        below = (u32)__shfl((int)below, src);
        prefix |= (u64)digit << shift;
        himask = ~0ull << shift;
        rank -= below;
        __syncthreads();   // the histograms are read: the next pass may clear them
    }
    const u64 T = prefix;
    // the K keys <= T through the scratch to the front of the buffer
    for (u32 i0 = 0; i0 < cnt; i0 += NT) {
        const u32 i = i0 + (u32)tid;
        const u64 k = i < cnt ? buf[i] : (u64)KEY_MAX;
        const bool keep = i < cnt && k <= T;
        const u64 mask = __ballot(keep);
        u32 base = 0;
        if (lane == 0 && mask != 0ull) base = atomicAdd(&ctl->scnt, (u32)__popcll(mask));
        base = (u32)__builtin_amdgcn_readfirstlane((int)base);
        if (keep) scr[base + sel_lane_prefix(mask)] = k;
    }
    __syncthreads();
    for (int i = tid; i < K; i += NT) buf[i] = scr[i];
    if (tid == 0) {
        ctl->cnt = (u32)K;
        ctl->scnt = 0u;
        ctl->kmin = KEY_MAX;
        ctl->kmax = 0ull;
    }
    __syncthreads();
    return T;
}

// DS: the sub-space width at compile time (the table build's software pipeline), 0: any.  M: 8 or 16 sub-quantizers (16-byte code loads),
// 0: any m at the code stride.
template <int DS, int M>
__global__ __launch_bounds__(selscan::THREADS) void sel_scan_kernel(const SelScanArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int NT = selscan::THREADS;
    constexpr u32 PPT = M == 8 ? 2u : 1u;
    constexpr u32 STEP = (u32)NT * PPT;
    static_assert((int)STEP <= selscan::STEP_MAX, "a step is what the plan leaves room for");
    const IndexView &ix = a.ix;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = a.w, K = a.K, m = ix.m;
    const u32 cap = a.cap;
    const selscan::Layout L = selscan::layout(ix.d, m, K, (int64_t)cap);
    float *resid = (float *)(smem_raw + L.resid);
    float *tab = (float *)(smem_raw + L.tab);
    u64 *buf = (u64 *)(smem_raw + L.keys);
    u64 *scr = (u64 *)(smem_raw + L.scratch);
    u32 *hist = (u32 *)(smem_raw + L.hist);
    SelCtl *ctl = (SelCtl *)(smem_raw + L.ctl);
    const int *prow_list = a.probe_list + (size_t)q * w;
    const float *prow_dc = a.probe_dc + (size_t)q * w;
    const u32 *prow_base = a.probe_base + (size_t)q * w;
    if (tid == 0) {
        ctl->cnt = 0u;
        ctl->scnt = 0u;
        ctl->kmin = KEY_MAX;
        ctl->kmax = 0ull;
    }
    u64 bound = KEY_MAX;   // uniform
    // the table build is written for 256 lanes, one per codeword: the workgroup's groups of 256 take an equal share of the sub-quantizers
    // each through a view that starts at their first one (pair-packed dsub = 6: whole pairs)
    constexpr int UNIT = DS == 6 ? 2 : 1, GROUPS = NT / 256;
    const int per = (((m + UNIT - 1) / UNIT + GROUPS - 1) / GROUPS) * UNIT;
    const int ii0 = (tid >> 8) * per;
    const int mine = min(per, m - ii0);   // <= 0: nothing (m = 1)
    IndexView hx = ix;
    if (mine > 0) {
        constexpr int DP = DS == 6 ? 6 : (DS + 3) & ~3;
        hx.codebooks = ix.codebooks + (size_t)ii0 * ix.ksub * ix.dsub;
        hx.codebooks_t = ix.codebooks_t + (size_t)ii0 * ix.ksub * DP;
        hx.labels = ix.labels + (size_t)ii0 * ix.ksub;
    }
    // a lane's points of the step that starts at p0: never a byte behind the list's last point
    auto load_codes = [&](const uint8_t *codes, u32 p0, u32 len) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        const u32 p = p0 + (u32)tid * PPT;
        if constexpr (M == 8) {
            if (p + 1u < len) v = *(const uint4 *)(codes + (size_t)p * 8);
            else if (p < len) {
                const uint2 h2 = *(const uint2 *)(codes + (size_t)p * 8);
                v.x = h2.x; v.y = h2.y;
            }
        } else if constexpr (M == 16) {
            if (p < len) v = *(const uint4 *)(codes + (size_t)p * 16);
        }
        return v;
    };
    auto lookup4 = [&](float dist, u32 word, int ii) {
#pragma unroll
        for (int b = 0; b < 4; ++b) dist = dist + tab[(ii + b) * 256 + (int)((word >> (8 * b)) & 255u)];
        return dist;
    };
    for (int j = 0; j < w; ++j) {
        const int l = prow_list[j];
        const float dc = prow_dc[j];
        const u32 sbase = prow_base[j];
        const u32 len = ix.list_len[l];
        const uint8_t *codes = ix.codes + ix.list_codeoff[l];
        uint4 cur = load_codes(codes, 0u, len);   // in flight while the table is built
        __syncthreads();   // the previous probe's appends are done and its table is no longer read
        u32 ub = ctl->cnt;   // uniform: nothing writes the counter before the next barrier
        if (ub >= 2u * (u32)K && ub >= SEL_EARLY_MIN) {
            bound = sel_round(buf, scr, hist, ctl, ub, K, tid);
            ub = (u32)K;
        }
        if (a.prune && bound != KEY_MAX && ((u64)__float_as_uint(dc) << 32) > bound) {
            if (tid == 0) {
                u64 skipped = 0;
                for (int pj = j; pj < w; ++pj) skipped += ix.list_len[prow_list[pj]];
                atomicAdd(a.scanned_points + (size_t)(q & 63) * 8 + 1, skipped);
            }
            break;
        }
        if (len == 0u) continue;   // uniform
        for (int i = tid; i < ix.d; i += NT) resid[i] = a.queries[(size_t)q * ix.d + i] - ix.centroids[(size_t)l * ix.d + i];
        __syncthreads();
        if (mine > 0) build_tables_t<1, DS, TAB_SEP>(hx, mine, resid + (size_t)ii0 * ix.dsub, tab + (size_t)ii0 * 256, tid & 255);
        __syncthreads();
        for (u32 p0 = 0; p0 < len; p0 += STEP) {
            const u32 take = min(STEP, len - p0);
            if (ub + take > cap) {   // the buffer may not hold this step: look at the counter, select if it does not
                __syncthreads();
                u32 c = ctl->cnt;
                __syncthreads();
                if (c + take > cap) {
                    bound = sel_round(buf, scr, hist, ctl, c, K, tid);
                    c = (u32)K;
                }
                ub = c;
            }
            const uint4 cv = cur;
            if (p0 + STEP < len) cur = load_codes(codes, p0 + STEP, len);
            const u32 p = p0 + (u32)tid * PPT;
            u64 key[PPT];
            bool ok[PPT];
            if constexpr (M == 8) {
                key[0] = make_key(lookup4(lookup4(dc, cv.x, 0), cv.y, 4), sbase + p);
                key[1] = make_key(lookup4(lookup4(dc, cv.z, 0), cv.w, 4), sbase + p + 1u);
                ok[0] = p < len && key[0] < bound;
                ok[1] = p + 1u < len && key[1] < bound;
            } else if constexpr (M == 16) {
                key[0] = make_key(lookup4(lookup4(lookup4(lookup4(dc, cv.x, 0), cv.y, 4), cv.z, 8), cv.w, 12), sbase + p);
                ok[0] = p < len && key[0] < bound;
            } else {
                float dist = dc;
                if (p < len) {
                    const uint8_t *cp = codes + (size_t)p * ix.cs;
                    for (int ii = 0; ii < m; ii += 4) {
                        const u32 word = *(const u32 *)(cp + ii);   // (the stride is a multiple of 4: a point's own padding at most)
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                            if (ii + b < m) dist = dist + tab[(ii + b) * 256 + (int)((word >> (8 * b)) & 255u)];
                    }
                }
                key[0] = make_key(dist, sbase + p);
                ok[0] = p < len && key[0] < bound;
            }
            // one LDS atomic per wave
            u64 mask[PPT];
            u32 total = 0;
#pragma unroll
            for (u32 s = 0; s < PPT; ++s) {
                mask[s] = __ballot(ok[s]);
                total += (u32)__popcll(mask[s]);
            }
            if (total != 0u) {   // wave-uniform
                u32 base = 0;
                if (lane == 0) base = atomicAdd(&ctl->cnt, total);
                base = (u32)__builtin_amdgcn_readfirstlane((int)base);
#pragma unroll
                for (u32 s = 0; s < PPT; ++s) {
                    if (ok[s]) buf[base + sel_lane_prefix(mask[s])] = key[s];
                    base += (u32)__popcll(mask[s]);
                }
            }
            ub += take;
        }
    }
    __syncthreads();
    u32 count = ctl->cnt;   // (after a break behind a round: K, already behind that round's barrier)
    if (count > (u32)K) {
        sel_round(buf, scr, hist, ctl, count, K, tid);
        count = (u32)K;
    } else {
        for (u32 i = tid; i < count; i += NT) scr[i] = buf[i];
    }
    const u32 n = (u32)selscan::pow2ceil((int)count);
    for (u32 i = count + (u32)tid; i < n; i += NT) scr[i] = KEY_MAX;
    __syncthreads();
    for (u32 k = 2; k <= n; k <<= 1) {
        for (u32 jj = k >> 1; jj > 0; jj >>= 1) {
            for (u32 t = tid; t < (n >> 1); t += NT) {
                const u32 i = ((t & ~(jj - 1u)) << 1) | (t & (jj - 1u));
                const u32 o = i | jj;
                const bool up = (i & k) == 0u;
                const u64 x = scr[i], y = scr[o];
                if ((x > y) == up) { scr[i] = y; scr[o] = x; }
            }
            __syncthreads();
        }
    }
    for (u32 i = tid; i < count; i += NT)
        emit_result(scr[i], (int)i, q, w, K, prow_list, prow_base, ix.list_pos, ix.ids, a.out_ids, a.out_dists);
    if (tid == 0) a.out_counts[q] = (int)count;
}

}  // namespace ivf
