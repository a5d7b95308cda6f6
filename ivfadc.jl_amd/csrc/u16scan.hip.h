// u16scan.hip.h -- the list-major scan for U = UInt16 codes (256 < k <= 65536; any k stored as UInt16), and the exact encoder
// of such an index.
//
// Device codes of a 16-bit handle are CODEWORD INDICES 0..ksub-1 (labels are translated on the host), 2m bytes per point at the
// handle's stride cs.  One (query, probe) table is m x ksub f32 entries: 32 KB per sub-space at k = 1024, 256 KB at k = 65536, so
// the tables of a probe do not fit the LDS together.  The kernel therefore works SUB-SPACE MAJOR:
//
//   for ii = 0 .. m-1:                                   (ascending: every sum gets its terms in the reference's order)
//       for each tile of codewords [c0, c0 + T):         (one tile when P x ksub floats fit the 32 KB table area)
//           build tab[s][c - c0] = sum_t (cb[ii][c][t] - r_s[ii*dsub + t])^2   for the P residuals   (index.jl:232-236)
//           every point whose code ii lies in the tile adds tab[s][code - c0] to its running sum s     (index.jl:240-246)
//
// A work item is up to P = 8 (query, probe) pairs that probe the same list (the probe buckets of the list-major plan), and one
// chunk of that list.  Each codeword read from L2 serves the item's P residuals: the table build, not the list stream, is the
// expensive part at these k (d = 128, k = 1024: 393 k element operations per table against ~8 k lookups per SIFT1M-shape list).
// Running sums live in registers, U16_PPT points per thread, so a chunk is walked in passes of 256 x U16_PPT points and the tables
// are rebuilt per pass.  Each pass pushes its keys (f32 bits << 32 | visit order) into register selectors (WSel<true>, K <= 64); the
// four waves' selectors are merged per pair at the end of the chunk, the partial top-K goes out as the other list-major kernels'
// do, and merge_kernel<true> finishes it.  Exact probe pruning as in scan_kernel: an item whose pairs' K-th keys are all below
// their coarse distances is skipped.
//
// K > 64 (u16_wide_scan_kernel, on request: ivfadc_set_table_mode(h, 10)): the same loop with LDS selectors (WSel<false>), one per wave
// and pair, selbuf[4 waves][qg][cap] u64 with cap = max(128, pow2ceil(K + 64)) as in make_plan.  The buffers sit BESIDE the table area:
// the tables are rebuilt for every sub-space, tile and pass, the selectors live for the whole chunk.  At the end of the chunk the waves
// sort their buffers, wave v absorbs the other waves' entries of pairs v and v + 4 in place, and merge_kernel<false> finishes.
// Reach: 32 (m dsp + qg cap) + 32 912 B <= 160 KB, i.e. m dsp + qg cap <= 4091 (dsp = dsub rounded up to 4); the plan halves qg until
// that holds.  cap = 4096 (K >= 1985) never fits, so K <= 1984 where m dsp <= 2040 (qg = 1), K <= 960 up to m dsp <= 3064, K <= 448 up
// to 3576, K <= 192 up to 3832; beyond that (and for K > 1984) the search takes the generic path as before.
//
// TABLE-FREE (u16_direct_scan_kernel / u16_direct_wide_scan_kernel, on request: ivfadc_set_u16_tables): a point needs one entry per
// sub-space, the one of its own code, and a pass holds at most U16_PASS points -- fewer than the ksub entries a table build computes
// whenever ksub > 1024 or the list is shorter than ksub.  These entries compute that one entry for the point itself:
//
//   for ii = 0 .. m-1:  every point gathers the codeword its code names from codebooks ([m][ksub][dsub], 16-byte loads where
//       dsub % 4 == 0, single floats otherwise), 16 bytes at a time with the next group in flight, and forms for each pair s
//           sum = 0;  for t ascending: df = cw[t] - r_s[ii*dsub + t];  sum = sum + df*df;      then   acc[s] = acc[s] + sum
//
// The sum of a sub-space is formed in its own accumulator from zero and added afterwards: the table entry's expression, in its order,
// hence its bits.  Everything around the accumulate phase is the table form's.  No table area, no tile loop, no barrier inside the
// sub-space loop; a lane without a point (at or behind p1: the chunk's or the list's end) reads neither a code nor a codeword, and a
// code is clamped to ksub - 1 before it becomes an address.  LDS: residuals + the wave-merge exchange (16 KB) for K <= 64
// (u16_direct_lds_bytes); residuals + selbuf[4][qg][cap] beyond (u16_direct_wide_lds_bytes), so the wide reach grows to
// 32 (m dsp + qg cap) + 144 B <= 160 KB, i.e. m dsp + qg cap <= 5115: K <= 1984 where m dsp <= 3064 (qg = 1), K <= 960 up to 4088,
// K <= 448 up to 4600, K <= 192 up to 4856 -- and cap = 4096 fits where m dsp <= 1016, so there K reaches IVFADC_MAX_K = 2048.
#pragma once
#include "kernels.hip.h"
#include "scan_layouts.h"   // U16_P ... U16_DIRECT_COST and the four u16_*_lds_bytes: shared with the plan

namespace ivf {

// qg: the bucket grouping of the plan (1, 2, 4 or 8); items carry up to qg pairs.  SMALL: K <= 64, register selectors;
// DIRECT: table-free accumulate phase
template <bool SMALL, bool DIRECT> static __device__ __forceinline__ void u16_scan_body(const ScanArgs &a, int qg)
{
    constexpr int TABF = DIRECT ? (SMALL ? U16_XCH_FLOATS : 0) : U16_TAB_FLOATS;   // floats between the residuals and what follows
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const IndexView &ix = a.ix;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int d = ix.d, m = ix.m, ksub = ix.ksub, dsub = ix.dsub, K = a.K;
    const int cap = SMALL ? 64 : a.cap;
    const int dsp = (dsub + 3) & ~3, rstride = m * dsp;
    float *resid = (float *)smem_raw;                                  // [P][m][dsp]
    float *tab = resid + (size_t)U16_P * rstride;                     // [P][T] (DIRECT: the exchange only)
    // SMALL: xch[4 waves][P][64] aliases the tables after the scan; else the selector buffers [4 waves][qg][cap], which ARE the exchange
    u64 *xch = SMALL ? (u64 *)tab : (u64 *)(tab + TABF);
    const size_t xw = SMALL ? (size_t)U16_P : (size_t)qg;              // selectors per wave in xch
    int *scnt = SMALL ? (int *)(tab + TABF) : (int *)(xch + (size_t)4 * qg * cap);   // [4][P]
    u32 *swi = (u32 *)(scnt + 4 * U16_P);                              // [2]
    const bool direct = qg == 1 && a.direct_items != 0;
    const u32 total = direct ? a.direct_items : a.wi_off[ix.kc];
    const u32 cs2 = (u32)ix.cs >> 1;                                   // stride in uint16_t
    const int ngrp = (dsub + 3) >> 2;                                  // 16-byte groups per codeword in codebooks_t

    for (;;) {
        __syncthreads();
        if (tid == 0) swi[0] = atomicAdd(a.queue_head, 1u);
        __syncthreads();
        const u32 wi = __builtin_amdgcn_readfirstlane(swi[0]);
        if (wi >= total) break;   // uniform

        int l;
        u32 cnt, chunk, grp, direct_probe = 0;
        if (direct) {   // (the work-item order of scan_kernel's direct mode: rank-major)
            const u32 t = wi / (u32)a.maxch, nqd = a.direct_items / ((u32)a.maxch * (u32)a.w);
            chunk = wi - t * (u32)a.maxch;
            const u32 j = t / nqd;
            direct_probe = (t - j * nqd) * (u32)a.w + j;
            l = a.probe_list[direct_probe];
            cnt = 1;
            grp = 0;
        } else {
            int lo = 0, hi = ix.kc;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (a.wi_off[mid] <= wi) lo = mid; else hi = mid;
            }
            l = lo;
            cnt = a.list_cnt[l];
            const u32 ng = (cnt + qg - 1) / qg;
            const u32 local = wi - a.wi_off[l];
            chunk = local / ng;
            grp = local - chunk * ng;
        }
        const u32 len = ix.list_len[l];
        const u32 p0 = chunk * a.CH;
        if (p0 >= len) continue;   // uniform
        const u32 p1 = min(len, p0 + a.CH);
        const int nvalid = min(qg, (int)(cnt - grp * qg));

        u32 pidx[U16_P], sbase[U16_P];
        int qi[U16_P];
        float dc[U16_P];
        u64 hard[U16_P];
        WSel<SMALL> sel[U16_P];
#pragma unroll
        for (int s = 0; s < U16_P; ++s) {
            const int ss = s < nvalid ? s : 0;
            pidx[s] = direct ? direct_probe : a.bucket_items[a.bucket_off[l] + grp * qg + ss];
            qi[s] = (int)(pidx[s] / (u32)a.w);
            dc[s] = a.probe_dc[pidx[s]];
            sbase[s] = a.probe_base[pidx[s]];
            hard[s] = readfirstlane64(__hip_atomic_load(&a.qthr[qi[s]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            sel[s].init(hard[s], SMALL ? nullptr : xch + ((size_t)wv * xw + ss) * cap, cap, K);   // (slots >= nvalid are never pushed to)
        }
        // exact probe pruning (scan_kernel): no sum of this list is below its coarse distance
        if (a.prune) {
            if (tid == 0) {
                bool all = true;
#pragma unroll
                for (int s = 0; s < U16_P; ++s) all = all && (s >= nvalid || __float_as_uint(dc[s]) > (u32)(hard[s] >> 32));
                swi[1] = all ? 1u : 0u;
            }
            __syncthreads();
            if (swi[1] != 0u) {   // uniform
                if (tid < nvalid) {
                    u32 pi = pidx[0];
#pragma unroll
                    for (int s = 1; s < U16_P; ++s) pi = tid == s ? pidx[s] : pi;
                    a.part_cnt[(size_t)pi * a.maxch + chunk] = 0u;
                    atomicAdd(a.scanned_points + (size_t)(pi & 63u) * 8 + 1, (u64)(p1 - p0));
                }
                continue;
            }
        }
        // residuals r_s = q_s - c_l (coarsequantizers.jl:40-45)
        for (int e = tid; e < nvalid * d; e += 256) {
            const int s = e / d, i = e - s * d;
            int qs = qi[0];
#pragma unroll
            for (int t = 1; t < U16_P; ++t)
                if (s == t) qs = qi[t];
            const int ii = i / dsub;
            resid[s * rstride + ii * dsp + (i - ii * dsub)] = a.queries[(size_t)qs * d + i] - ix.centroids[(size_t)l * d + i];
        }
        if (DIRECT) __syncthreads();   // (the table form's first tile barrier orders the residual writes)
        const int T = U16_TAB_FLOATS / nvalid;   // codewords per tile
        const uint16_t *cbase = (const uint16_t *)(ix.codes + ix.list_codeoff[l]);

        for (u32 pp = p0; pp < p1; pp += U16_PASS) {
            float acc[U16_PPT][U16_P];
#pragma unroll
            for (int k = 0; k < U16_PPT; ++k)
#pragma unroll
                for (int s = 0; s < U16_P; ++s) acc[k][s] = dc[s];
            if (DIRECT) {
                const bool al4 = (dsub & 3) == 0;
                bool valid[U16_PPT];
#pragma unroll
                for (int k = 0; k < U16_PPT; ++k) valid[k] = pp + (u32)(k * 256 + tid) < p1;
                // one group of a point's codeword: a lane without a point reads nothing; the terms behind dsub are never read, nor summed
                auto group = [&](const float *cw, bool v, int g) {
                    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (v) {
                        const float *src = cw + 4 * g;
                        if (al4) o = *(const float4 *)src;
                        else {
                            const int nt = dsub - 4 * g;
                            o.x = src[0];
                            if (nt > 1) o.y = src[1];
                            if (nt > 2) o.z = src[2];
                            if (nt > 3) o.w = src[3];
                        }
                    }
                    return o;
                };
                for (int ii = 0; ii < m; ++ii) {
                    const float *cw[U16_PPT];
                    float4 cur[U16_PPT];
#pragma unroll
                    for (int k = 0; k < U16_PPT; ++k) {
                        const u32 p = pp + (u32)(k * 256 + tid);
                        const u32 c = valid[k] ? min((u32)cbase[(size_t)p * cs2 + ii], (u32)(ksub - 1)) : 0u;
                        cw[k] = ix.codebooks + ((size_t)ii * ksub + c) * dsub;
                        cur[k] = group(cw[k], valid[k], 0);
                    }
                    const float *rr = resid + ii * dsp;
                    float sum[U16_PPT][U16_P];
#pragma unroll
                    for (int k = 0; k < U16_PPT; ++k)
#pragma unroll
                        for (int s = 0; s < U16_P; ++s) sum[k][s] = 0.0f;
                    for (int g = 0; g < ngrp; ++g) {
                        float4 nxt[U16_PPT];
#pragma unroll
                        for (int k = 0; k < U16_PPT; ++k) nxt[k] = group(cw[k], valid[k] && g + 1 < ngrp, g + 1);
                        const int nt = min(4, dsub - 4 * g);
#pragma unroll
                        for (int s = 0; s < U16_P; ++s)
                            if (s < nvalid) {
                                const float4 r4 = *(const float4 *)(rr + s * rstride + 4 * g);   // (uniform address: a broadcast)
                                const float rv[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
                                for (int k = 0; k < U16_PPT; ++k) {
                                    const float vv[4] = {cur[k].x, cur[k].y, cur[k].z, cur[k].w};
#pragma unroll
                                    for (int j = 0; j < 4; ++j)
                                        if (j < nt) {
                                            const float df = vv[j] - rv[j];
                                            sum[k][s] = sum[k][s] + df * df;
                                        }
                                }
                            }
#pragma unroll
                        for (int k = 0; k < U16_PPT; ++k) cur[k] = nxt[k];
                    }
#pragma unroll
                    for (int k = 0; k < U16_PPT; ++k)
#pragma unroll
                        for (int s = 0; s < U16_P; ++s)
                            if (s < nvalid) acc[k][s] = acc[k][s] + sum[k][s];
                }
            } else
            for (int ii = 0; ii < m; ++ii) {
                u32 code[U16_PPT];
#pragma unroll
                for (int k = 0; k < U16_PPT; ++k) {
                    const u32 p = pp + (u32)(k * 256 + tid);
                    code[k] = p < p1 ? (u32)cbase[(size_t)p * cs2 + ii] : 0xFFFFFFFFu;
                }
                // codewords from codebooks_t ([m][dp / 4][ksub][4], zero-padded): the 64 lanes of a wave read 64 consecutive 16-byte groups
                const float4 *cbi = (const float4 *)ix.codebooks_t + (size_t)ii * ngrp * ksub;
                for (int c0 = 0; c0 < ksub; c0 += T) {
                    const int c1 = min(ksub, c0 + T);
                    __syncthreads();   // the previous tile's lookups (and the residual writes) are done
                    for (int c = c0 + tid; c < c1; c += 256) {
                        const float *rr = resid + ii * dsp;
                        float sum[U16_P];
#pragma unroll
                        for (int s = 0; s < U16_P; ++s) sum[s] = 0.0f;
                        for (int g = 0; g < ngrp; ++g) {
                            const float4 v4 = cbi[(size_t)g * ksub + c];
                            const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
                            const int nt = min(4, dsub - 4 * g);
#pragma unroll
                            for (int s = 0; s < U16_P; ++s)
                                if (s < nvalid) {
                                    const float4 r4 = *(const float4 *)(rr + s * rstride + 4 * g);   // (uniform address: a broadcast)
                                    const float rv[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
                                    for (int j = 0; j < 4; ++j)
                                        if (j < nt) {
                                            const float df = vv[j] - rv[j];
                                            sum[s] = sum[s] + df * df;
                                        }
                                }
                        }
#pragma unroll
                        for (int s = 0; s < U16_P; ++s)
                            if (s < nvalid) tab[s * T + (c - c0)] = sum[s];
                    }
                    __syncthreads();
#pragma unroll
                    for (int k = 0; k < U16_PPT; ++k) {
                        const u32 off = code[k] - (u32)c0;
                        if (off < (u32)(c1 - c0)) {
#pragma unroll
                            for (int s = 0; s < U16_P; ++s)
                                if (s < nvalid) acc[k][s] = acc[k][s] + tab[s * T + off];
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < U16_PPT; ++k) {
                const u32 p = pp + (u32)(k * 256 + tid);
                const bool valid = p < p1;
#pragma unroll
                for (int s = 0; s < U16_P; ++s)
                    if (s < nvalid) {
                        const u64 key = make_key(acc[k][s], sbase[s] + p);
                        sel[s].push(valid && key < sel[s].thr(), key, K, lane);
                    }
            }
        }

        // per-wave results -> LDS (SMALL: aliasing the tables; else sorted in place in the selector buffers), then wave v merges pairs v
        // and v + 4 and publishes them
        int mycnt[U16_P];
#pragma unroll
        for (int s = 0; s < U16_P; ++s) mycnt[s] = s < nvalid ? sel[s].finish(K, lane) : 0;
        if (SMALL) __syncthreads();   // the exchange area aliases the tables: every wave must be done scanning
#pragma unroll
        for (int s = 0; s < U16_P; ++s)
            if (s < nvalid) {
                sel[s].store(xch + ((size_t)wv * xw + s) * cap, mycnt[s], lane);
                if (lane == 0) scnt[wv * U16_P + s] = mycnt[s];
            }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < U16_P; ++s) {
            if ((s & 3) == wv && s < nvalid) {
                merge_waves(sel[s], xch + (size_t)s * cap, xw * cap, scnt + s, U16_P, K, hard[s], wv, lane);
                const int fc = sel[s].finish(K, lane);
                const size_t slot = (size_t)pidx[s] * a.maxch + chunk;
                u64 *dst = a.part_keys + slot * K;
                sel[s].for_each(fc, lane, [&](int i, u64 key) { dst[i] = key; });
                if (lane == 0) {
                    a.part_cnt[slot] = (u32)fc;
                    if (fc == K) atomicMin(&a.qthr[qi[s]], sel[s].thr());
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void u16_scan_kernel(const ScanArgs a, int qg) { u16_scan_body<true, false>(a, qg); }
// 64 < K: LDS selectors beside the tables (a.cap; dynamic LDS u16_wide_lds_bytes)
__global__ __launch_bounds__(256) void u16_wide_scan_kernel(const ScanArgs a, int qg) { u16_scan_body<false, false>(a, qg); }
// table-free (ivfadc_set_u16_tables): dynamic LDS u16_direct_lds_bytes / u16_direct_wide_lds_bytes
__global__ __launch_bounds__(256) void u16_direct_scan_kernel(const ScanArgs a, int qg) { u16_scan_body<true, true>(a, qg); }
__global__ __launch_bounds__(256) void u16_direct_wide_scan_kernel(const ScanArgs a, int qg) { u16_scan_body<false, true>(a, qg); }

// _encode_point's quantize_data for UInt16 codes (utils.jl:148-161): per sub-space the codeword index with the smallest
// sum_t (cb[t] - r[t])^2, first minimum on ties (keys f32 bits << 32 | index).  One workgroup per point; out: n x m uint16_t indices.
__global__ __launch_bounds__(256) void encode_u16_kernel(const float *__restrict__ pts, const int *__restrict__ assign, int d, int m,
                                                         int ksub, int dsub, const float *__restrict__ centroids,
                                                         const float *__restrict__ codebooks, uint16_t *__restrict__ out_codes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *resid = (float *)smem_raw;                               // [d]
    u64 *best = (u64 *)(resid + (((size_t)d + 3) & ~(size_t)3));    // [m]
    const int p = blockIdx.x, tid = threadIdx.x;
    const int l = assign[p];
    for (int i = tid; i < d; i += 256) resid[i] = pts[(size_t)p * d + i] - centroids[(size_t)l * d + i];
    for (int i = tid; i < m; i += 256) best[i] = KEY_MAX;
    __syncthreads();
    for (int ii = 0; ii < m; ++ii) {
        const float *rr = resid + (size_t)ii * dsub;
        u64 key = KEY_MAX;
        for (int c = tid; c < ksub; c += 256) {
            const float *cw = codebooks + ((size_t)ii * ksub + c) * dsub;
            float sum = 0.0f;
            for (int t = 0; t < dsub; ++t) {
                const float df = cw[t] - rr[t];
                sum = sum + df * df;
            }
            const u64 k2 = make_key(sum, (u32)c);
            key = k2 < key ? k2 : key;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u64 o = __shfl_xor(key, off);
            key = o < key ? o : key;
        }
        if ((tid & 63) == 0) atomicMin(&best[ii], key);
    }
    __syncthreads();
    for (int i = tid; i < m; i += 256) out_codes[(size_t)p * m + i] = (uint16_t)(u32)best[i];
}

}  // namespace ivf
