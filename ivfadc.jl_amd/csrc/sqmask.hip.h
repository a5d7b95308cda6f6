// sqmask.hip.h -- the latency path of the per-query filtered search (ivfadc_set_masked_latency(h, 1); ivfadc_search_masked and
// ivfadc_search_device_masked): sq_kernel's one launch (smallq.hip.h) around a point loop that reads the MASK first and touches codes for
// selected entries only.  gfx950, wave64.  Mask layout and bit addressing: maskset_plan.h; MaskView: maskset.hip.h.
//
//   workgroup (q, j, c)   as sq_kernel: the coarse row (from coarse_lane_kernel, or computed in the launch), the exact stable top-w, probe j
//                         alone.  These stages are sq_kernel's statements restated -- that kernel's code stays where its registers were
//                         measured -- on the same functions: select_row_short / select_row, merge_waves, build_residuals,
//                         build_tables_t<1, DS, TAB_SEP>, emit_result.
//   the mask number       mask_of_query[q] clamped into [-1, nmasks) as it is read (null: mask 0), so the device entry needs no ingest
//                         launch; -1: no row, every position below the chunk's end counts as selected.
//   mask first            the chunk's rounds of 64 points are dealt to the four waves in four consecutive runs.  A wave takes its run 64
//                         rounds at a time: every lane loads ONE round's two words (one coalesced 512-byte load covers 4096 points), the
//                         bits at or behind the chunk's end are cut, and the rounds that hold a bit are walked from the ballot, each word
//                         made uniform with readlane.  A lane whose bit is set writes its position into the wave's pending queue in LDS
//                         at the rank mbcnt gives it; the count advances by the popcount.
//   dense consumption     once 64 positions are pending the wave takes them, one per lane: the point's m code bytes in one 8- or 16-byte
//                         load (three at m = 48; dword loads at the generic stride), then d = dc; d += tab_ii[code_ii] for ascending ii
//                         -- the reference's sum (index.jl:242-246), one rounding per add -- and make_key(d, sbase + p) with the ORIGINAL
//                         position p.  What is left at the end of the run is drained.  Keys are unique and carry their visit numbers, so
//                         the order of consumption changes no result; under a full mask the pending positions are consecutive and the
//                         code loads coalesce as in the plain scan.
//   cost                  code bytes and lookups for selected points; 8 bytes of mask per 64 positions.  The mask is looked at BEFORE the
//                         tables are built: a workgroup whose chunk holds no selected point counts its arrival with a result of 0 keys and
//                         builds nothing (a tenant that lives in a few cells).
// Bounds come from selected points only (the four waves share sthr as in scan_range).  Positions at or behind list_len never reach a
// selector: their bits are 0 by the set's construction and the words are cut at the chunk's end all the same.
// Plain C++, vector loads and stores; the one piece of inline assembly is the hand-off's s_waitcnt vmcnt(0), as in sq_kernel.
#pragma once

#include "maskset.hip.h"

namespace ivf {

// the row of query q's mask for list l (null: no filter); the mask number is clamped here, on read
static __device__ __forceinline__ const u32 *sqm_mask_row(const MaskView &mv, int nmasks, int q, int l)
{
    const int32_t r = mv.mask_of_query ? maskset::clamp_mask(mv.mask_of_query[q], nmasks) : 0;
    return r < 0 ? (const u32 *)nullptr : mv.words + maskset::row_start(mv.W, mv.word_off[l], (u32)r);
}

// the bits of the round at pb (a multiple of 64, pb < p1), those of positions >= p1 cut
static __device__ __forceinline__ u64 sqm_round(const u32 *row, u32 pb, u32 p1)
{
    const u64 bits = mask_round(row, pb);
    const u32 left = p1 - pb;
    return left < 64u ? bits & ((1ull << left) - 1ull) : bits;
}

// n <= 64 pending positions from `head` of the wave's queue on: one point per lane
template <int M>
static __device__ __forceinline__ void sqm_consume(const float *tab, const uint8_t *cbase, int cs, int m, const u32 *queue, u32 head, int n, float dc,
                                                   u32 sbase, WSel<true> (&sel)[1], int K, int lane, u64 *sthr, u32 &thr_hi)
{
    static_assert(M == 0 || M == 8 || M % 16 == 0, "one 8-byte load, or whole 16-byte loads");
    const bool ok = lane < n;
    u32 p = 0;
    float d = dc;
    if (ok) {
        p = queue[(head + (u32)lane) & (u32)(SQM_QUEUE - 1)];
        if constexpr (M > 0) {
            u32 wd[M / 4];
            const uint8_t *cp = cbase + (size_t)p * M;
            if constexpr (M == 8) {
                const uint2 v = *(const uint2 *)cp;
                wd[0] = v.x; wd[1] = v.y;
            } else {
#pragma unroll
                for (int k = 0; k < M / 16; ++k) {
                    const uint4 v = ((const uint4 *)cp)[k];
                    wd[4 * k] = v.x; wd[4 * k + 1] = v.y; wd[4 * k + 2] = v.z; wd[4 * k + 3] = v.w;
                }
            }
#pragma unroll
            for (int ii = 0; ii < M; ++ii) d = d + tab[ii * 256 + (int)((wd[ii >> 2] >> (8 * (ii & 3))) & 0xffu)];
        } else {
            const u32 *cp = (const u32 *)(cbase + (size_t)p * cs);
            const int nw = cs >> 2;
            for (int w4 = 0; w4 < nw; ++w4) {
                const u32 dw = cp[w4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int ii = w4 * 4 + b;
                    if (ii < m) d = d + tab[ii * 256 + (int)((dw >> (8 * b)) & 0xffu)];
                }
            }
        }
    }
    if (__any(ok && __float_as_uint(d) <= thr_hi)) {
        const float acc1[1] = {d};
        const u32 sb1[1] = {sbase};
        sel[0].tighten(readfirstlane64(sthr[0]));
        scan_emit<1>(acc1, p, ok, 1, sb1, sel, K, lane);
        publish_bound<1>(sthr, 0, sel[0], K, (u32)(sel[0].thr() >> 32) < thr_hi, lane);
        thr_hi = (u32)(sel[0].thr() >> 32);
    }
}

// The selected points of [p0, p1) of one list (p0 a multiple of 64) for the query whose tables are in `tab`.  queue: this wave's
// SQM_QUEUE words, used as a ring: fewer than 64 positions are pending whenever a round is pushed, so at most 127 ever are.
template <int M>
static __device__ __forceinline__ void sqm_scan_chunk(const float *tab, const uint8_t *cbase, int cs, int m, const u32 *row, u32 p0, u32 p1, float dc,
                                                      u32 sbase, WSel<true> (&sel)[1], int K, int wv, int lane, u32 *queue, u64 *sthr)
{
    sel[0].tighten(readfirstlane64(sthr[0]));
    u32 thr_hi = (u32)(sel[0].thr() >> 32);
    const u32 nr = (p1 - p0 + 63u) >> 6, per = (nr + 3u) >> 2;
    const u32 rbeg = min(nr, (u32)wv * per), rend = min(nr, rbeg + per);
    u32 head = 0, pending = 0;
    for (u32 r0 = rbeg; r0 < rend; r0 += 64) {
        u64 mword = 0;
        if (r0 + (u32)lane < rend) mword = sqm_round(row, p0 + (r0 + (u32)lane) * 64u, p1);
        u64 live = __ballot(mword != 0ull);
        while (live) {   // uniform: the rounds of this load that hold a selected point
            const int i = __builtin_ctzll(live);
            live &= live - 1ull;
            const u64 bits = readlane64(mword, i);
            const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(bits >> 32), __builtin_amdgcn_mbcnt_lo((u32)bits, 0u));
            if ((bits >> lane) & 1ull) queue[(head + pending + rank) & (u32)(SQM_QUEUE - 1)] = p0 + (r0 + (u32)i) * 64u + (u32)lane;
            pending += (u32)__popcll(bits);
            if (pending >= 64u) {
                wave_sync();
                sqm_consume<M>(tab, cbase, cs, m, queue, head, 64, dc, sbase, sel, K, lane, sthr, thr_hi);
                wave_sync();   // the ring's slots are read before the next round overwrites them
                head = (head + 64u) & (u32)(SQM_QUEUE - 1);
                pending -= 64u;
            }
        }
    }
    if (pending) {
        wave_sync();
        sqm_consume<M>(tab, cbase, cs, m, queue, head, (int)pending, dc, sbase, sel, K, lane, sthr, thr_hi);
    }
}

template <int M, int DS>
__global__ __launch_bounds__(256) void sq_masked_kernel(const SqArgs a, const MaskView mv, const int nmasks)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const IndexView &ix = a.ix;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m = (M > 0) ? M : ix.m;
    const int K = a.K, w = a.w, nch = a.nch, per_q = w * nch;
    const int q = blockIdx.x / per_q, rem = blockIdx.x - q * per_q;
    const int j = rem / nch, c = rem - j * nch;
    const LdsCarve L = carve_lds<1, true>(smem_raw, m, ix.d, 64);
    // behind the carve: sq_kernel's tail (SqLds) and, behind the row of coarse distances, the four pending queues (SqmLds, scan_layouts.h)
    constexpr SqLds S = sq_tail(0, 0);
    unsigned char *tail = (unsigned char *)L.scnt;
    int *s_list = (int *)(tail + S.s_list);
    float *s_dc = (float *)(tail + S.s_dc);
    u32 *s_base = (u32 *)(tail + S.s_base);
    u64 *wbound = (u64 *)(tail + S.wbound);
    u32 *ccnt = (u32 *)(tail + S.ccnt);
    float *s_row = (float *)(((size_t)(tail + S.row_lo) + 15) & ~(size_t)15);
    u32 *queue = (u32 *)(tail + sqm_queue_off(S.end, a.cdist ? 0 : ix.kc)) + wv * SQM_QUEUE;
    const float *qv = a.queries + (size_t)q * ix.d;

    // ---- coarse distances of the query (sq_kernel's: a lane owns a centroid of the regrouped [d / 4][kc][4] matrix, the reference's order)
    const float *row = a.cdist ? a.cdist + (size_t)q * ix.kc : s_row;
    if (!a.cdist) {
        const float4 *ct = (const float4 *)a.centroids_t;
        for (int c0 = tid; c0 < ix.kc; c0 += 1024) {
            const int c1 = c0 + 256 < ix.kc ? c0 + 256 : c0, c2 = c0 + 512 < ix.kc ? c0 + 512 : c0, c3 = c0 + 768 < ix.kc ? c0 + 768 : c0;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            auto acc4 = [](float s, const float4 &cv, const float4 &qq) {
                float t = cv.x - qq.x; s = s + t * t;
                t = cv.y - qq.y; s = s + t * t;
                t = cv.z - qq.z; s = s + t * t;
                t = cv.w - qq.w; s = s + t * t;
                return s;
            };
#pragma unroll 4
            for (int g = 0; g < (ix.d >> 2); ++g) {     // d % 4 == 0
                const float4 qq = *(const float4 *)(qv + 4 * g);
                const float4 *row4 = ct + (size_t)g * ix.kc;
                const float4 x0 = row4[c0], x1 = row4[c1], x2 = row4[c2], x3 = row4[c3];
                a0 = acc4(a0, x0, qq); a1 = acc4(a1, x1, qq); a2 = acc4(a2, x2, qq); a3 = acc4(a3, x3, qq);
            }
            s_row[c0] = a0;
            if (c0 + 256 < ix.kc) s_row[c1] = a1;
            if (c0 + 512 < ix.kc) s_row[c2] = a2;
            if (c0 + 768 < ix.kc) s_row[c3] = a3;
        }
    }
    if (tid == 0) arm_bound<1>(L.sthr, 0, KEY_MAX);
    __syncthreads();

    // ---- top-w, exact and stable; the probes of the query into LDS
    WSel<true> ws;
    ws.init(KEY_MAX, nullptr, 64, w);
    bool have = false;
    if (w <= SHORT_ROW_MAXK && ix.kc <= 8192 && (ix.kc & 3) == 0) {
        if (ix.kc <= 2048) have = select_row_short<false, 2>(ws, row, ix.kc, w, wv, lane, tid, L.xch, wbound, ccnt);
        else if (ix.kc <= 4096) have = select_row_short<false, 4>(ws, row, ix.kc, w, wv, lane, tid, L.xch, wbound, ccnt);
        else have = select_row_short<false, 8>(ws, row, ix.kc, w, wv, lane, tid, L.xch, wbound, ccnt);
    }
    if (!have) {
        ws.init(KEY_MAX, nullptr, 64, w);
        select_row<false, 4>(ws, row, ix.kc, w, wv, lane, L.sthr);
        const int wc = ws.finish(w, lane);
        ws.store(L.xch + (size_t)wv * 64, wc, lane);
        if (lane == 0) L.scnt[wv] = wc;
        __syncthreads();
        if (wv == 0) merge_waves(ws, L.xch, (size_t)64, L.scnt, 1, w, KEY_MAX, 0, lane);
    }
    if (wv == 0) {
        const int fcw = ws.finish(w, lane);       // == min(w, kc)
        u32 len = 0;
        int l = 0;
        if (lane < fcw) {
            l = (int)(u32)ws.top;
            len = ix.list_len[l];
        }
        u32 incl = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const u32 v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        if (lane < fcw) {
            s_list[lane] = l;
            s_dc[lane] = __uint_as_float((u32)(ws.top >> 32));
            s_base[lane] = incl - len;
        }
        const u32 total = __shfl(incl, 63);      // by every lane
        if (lane == 0) {
            arm_bound<1>(L.sthr, 0, KEY_MAX);    // re-armed for the scan
            ccnt[0] = 0u;                        // "this chunk holds a selected point" (the row selection is done with the word)
            // every probed point once, selected or not (the masked contract)
            if (j == 0 && c == 0) atomicAdd(a.scanned_points + (size_t)(q & 63) * 8, (u64)total);
        }
    }
    __syncthreads();

    // ---- probe j, chunk c: the mask first
    const int l = s_list[j];
    const float dcv = s_dc[j];
    const u32 sb = s_base[j];
    const u32 len = ix.list_len[l];
    const u32 p0 = (u32)c * a.CH, p1 = min(len, p0 + a.CH);
    const u32 *mrow = sqm_mask_row(mv, nmasks, q, l);
    bool mine = false;
    if (p0 < len) {   // uniform
        const u32 nr = (p1 - p0 + 63u) >> 6;
        for (u32 r = (u32)tid; r < nr; r += 256u) mine = mine || sqm_round(mrow, p0 + r * 64u, p1) != 0ull;
    }
    if (__any(mine) && lane == 0) ccnt[0] = 1u;   // (a flag in the carve: __syncthreads_or would bring static LDS, which the host refuses)
    __syncthreads();
    const bool any = ccnt[0] != 0u;
    WSel<true> sel[1];
    sel[0].init(KEY_MAX, nullptr, 64, K);
    int fc = 0;
    if (any) {   // uniform
        const uint8_t *cbase = ix.codes + ix.list_codeoff[l];
        const int qi[1] = {q}, li[1] = {l};
        build_residuals<1>(ix, a.queries, qi, li, L.resid, tid);
        __syncthreads();
        build_tables_t<1, DS, TAB_SEP>(ix, m, L.resid, L.tab, tid);
        __syncthreads();
        sqm_scan_chunk<M>(L.tab, cbase, ix.cs, m, mrow, p0, p1, dcv, sb, sel, K, wv, lane, queue, L.sthr);
        const int mycnt = sel[0].finish(K, lane);
        __syncthreads();              // the exchange area aliases the tables
        sel[0].store(L.xch + (size_t)wv * L.xcap, mycnt, lane);
        if (lane == 0) L.scnt[wv] = mycnt;
        __syncthreads();
        if (wv == 0) {
            merge_waves(sel[0], L.xch, (size_t)L.xcap, L.scnt, 1, K, KEY_MAX, 0, lane);
            fc = sel[0].finish(K, lane);
        }
    }
    if (per_q == 1) {   // one workgroup is the whole query: nothing to hand over
        if (wv == 0) {
            sel[0].for_each(fc, lane, [&](int i, u64 key) { emit_result(key, i, q, w, K, s_list, s_base, ix.list_pos, ix.ids, a.out_ids, a.out_dists); });
            if (lane == 0) a.out_counts[q] = fc;
        }
        return;
    }

    // ---- hand-off (sq_kernel's: write-through stores, drained; the arrival; the last arriver reads with agent-scope loads)
    const size_t slot = (size_t)q * per_q + rem;
    if (wv == 0) {
        u64 *dst = a.part_keys + slot * K;
        sel[0].for_each(fc, lane, [&](int i, u64 key) { __hip_atomic_store(&dst[i], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
        if (lane == 0) __hip_atomic_store(&a.part_cnt[slot], (u32)fc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (tid == 0) {
        const u32 prev = __hip_atomic_fetch_add(&a.arrive[q], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = prev == (u32)per_q - 1u;
        ccnt[1] = last ? 1u : 0u;
        if (last) __hip_atomic_store(&a.arrive[q], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every arrival of this launch is in: re-armed
    }
    __syncthreads();
    if (ccnt[1] == 0u || wv != 0) return;   // uniform per wave

    // ---- last arriver, wave 0: K smallest of the w * nch partial results, visit order -> stored id
    WSel<true> fin;
    fin.init(KEY_MAX, nullptr, 64, K);
    const int T = per_q * K;
    for (int e0 = 0; e0 < T; e0 += 64) {
        const int e = e0 + lane;
        bool pred = e < T;
        u64 key = KEY_MAX;
        if (pred) {
            const int s = e / K, i = e - s * K;
            const size_t sl = (size_t)q * per_q + s;
            pred = (u32)i < __hip_atomic_load(&a.part_cnt[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (pred) key = __hip_atomic_load(&a.part_keys[sl * K + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        pred = pred && key < fin.thr();
        fin.push(pred, key, K, lane);
    }
    const int nres = fin.finish(K, lane);
    fin.for_each(nres, lane, [&](int i, u64 key) { emit_result(key, i, q, w, K, s_list, s_base, ix.list_pos, ix.ids, a.out_ids, a.out_dists); });
    if (lane == 0) a.out_counts[q] = nres;
}

typedef void (*sq_masked_fn_t)(const SqArgs, const MaskView, const int);

}  // namespace ivf
