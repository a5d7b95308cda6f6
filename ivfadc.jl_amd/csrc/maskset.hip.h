// maskset.hip.h -- per-query filtered search (ivfadc_maskset_create, ivfadc_search_masked): mask sets in slot space and the list-major
// scan that tests them.  gfx950, wave64.  Layout and bit addressing: maskset_plan.h.
//
//   maskset_build_kernel   id-space bitmaps -> slot-space rows.  Work items (list, chunk of SUBSET_CHUNK points) as subset_count_kernel's;
//                          a lane reads the id of its entry ONCE, tests it against each of the nmasks id-space rows with
//                          subset::subset_selected, and the wave's __ballot goes out as the two words of its round, one 8-byte vector store
//                          per round and mask.  Positions at or behind list_len get bit 0 whatever stale ids lie there; rounds wholly behind
//                          the end have no words.  Optional kept counts: one vector atomic add per wave and mask.
//   masked_scan_kernel     the skeleton of scan_kernel<0, 0, QG, SMALL> (work queue, bucket and direct-mode items, build_residuals,
//                          build_tables_t<QG, 0, TAB_INTERLEAVED>, per-wave WSel selectors, publish_bound, merge_waves, partial keys and
//                          counts for merge_kernel) around a point loop of its own: one point per lane, dword code loads, and per slot the
//                          64 mask bits of the wave's round.  A round rejected for every valid slot costs two words per slot and nothing
//                          else: no code loads, no lookups.  Only selected points reach scan_emit, so every bound (sthr, qthr) comes from
//                          selected points and exact pruning stays exact.  A key keeps its ORIGINAL visit number (probe base + position).
// Plain C++ and vector loads and stores only.
#pragma once

#include "kernels.hip.h"
#include "maskset_plan.h"
#include "search_call.h"
#include "subset_plan.h"

namespace ivf {

// bits: nmasks id-space rows of bits_stride words each; words: nmasks slot-space rows of W words; kept: [nmasks] or null
__global__ __launch_bounds__(256) void maskset_build_kernel(const subset::Item *__restrict__ items, const int64_t *__restrict__ list_pos,
                                                            const uint32_t *__restrict__ list_len, const uint32_t *__restrict__ ids,
                                                            const uint32_t *__restrict__ bits, uint64_t nbits, uint64_t bits_stride, int nmasks,
                                                            const uint64_t *__restrict__ word_off, uint64_t W, uint32_t *__restrict__ words,
                                                            unsigned long long *__restrict__ kept)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const subset::Item it = items[blockIdx.x];
    const uint32_t len = list_len[it.list];
    const int64_t lpos = list_pos[it.list];
    uint32_t id[subset::SUBSET_ROUNDS];
#pragma unroll
    for (int r = 0; r < subset::SUBSET_ROUNDS; ++r) {
        const int64_t p = subset::subset_point(it.chunk, wv, r, lane);
        id[r] = 0;
        if (p < (int64_t)len) id[r] = ids ? ids[lpos + p] : (uint32_t)(lpos + p);   // (synthetic lists: the id emit_result returns)
    }
    for (int k = 0; k < nmasks; ++k) {
        const uint32_t *row_bits = bits + (size_t)k * bits_stride;
        uint32_t *row = words + maskset::row_start(W, word_off[it.list], (uint32_t)k);
        uint32_t total = 0;
#pragma unroll
        for (int r = 0; r < subset::SUBSET_ROUNDS; ++r) {
            const int64_t p = subset::subset_point(it.chunk, wv, r, lane);
            const int64_t p_first = p - lane;   // uniform: the round's first position
            const bool keep = p < (int64_t)len && subset::subset_selected(row_bits, nbits, id[r]);
            const unsigned long long mask = __ballot(keep);
            total += (uint32_t)__popcll(mask);
            if (lane == 0 && p_first < (int64_t)len)
                *(uint2 *)(row + maskset::round_word((uint64_t)p_first)) = make_uint2((uint32_t)mask, (uint32_t)(mask >> 32));
        }
        if (kept && lane == 0 && total != 0) atomicAdd(kept + k, (unsigned long long)total);
    }
}

// mask_of_query of the device entry: clamped into [-1, nmasks) so that a violated precondition cannot read outside the set (src null: mask 0)
__global__ __launch_bounds__(256) void maskset_ingest_kernel(const int32_t *__restrict__ src, int64_t n, int32_t nmasks, int32_t *__restrict__ dst)
{
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256)
        dst[q] = src ? maskset::clamp_mask(src[q], nmasks) : 0;
}

// what a masked search hands its scan: the slot-space words, the layout, and the mask number of every query of the sub-batch
struct MaskView {
    const u32 *words;            // [nmasks][W]
    const uint64_t *word_off;    // [kc + 1]
    uint64_t W;
    const int32_t *mask_of_query;   // [queries of the sub-batch], every value in [-1, nmasks)
};

// The one place a MaskView is filled: the set and the mask numbers of the queries of c (host).  No set: words null, which the range and
// generic kernels read as "no filter".
inline MaskView mask_view(const SearchCall &c)
{
    MaskView mv{};
    mv.words = c.mask_words;
    mv.word_off = c.mask_word_off;
    mv.W = c.mask_W;
    mv.mask_of_query = c.mask_of_query;
    return mv;
}

// the row of query q's mask for list l, or null (no filter)
static __device__ __forceinline__ const u32 *mask_row(const MaskView &mv, int q, int l)
{
    const int32_t r = mv.mask_of_query[q];
    return r < 0 ? (const u32 *)nullptr : mv.words + maskset::row_start(mv.W, mv.word_off[l], (u32)r);
}

// the 64 bits of the round that starts at position pb (a multiple of 64) of a row; null counts as all ones
static __device__ __forceinline__ u64 mask_round(const u32 *row, u32 pb)
{
    if (!row) return ~0ull;
    const uint2 v = *(const uint2 *)(row + maskset::round_word(pb));
    return maskset::round_bits(v.x, v.y);
}

// Points [p0, p1) of one list (p0 a multiple of 64) for the QG queries whose tables are in `tab`: one point per lane, the four waves
// interleave rounds of 64.  row[s]: the mask row of slot s for this list (null: no filter).
template <int QG, class S>
static __device__ __forceinline__ void masked_scan_range(const float *tab, const uint8_t *cbase, int cs, int m, u32 p0, u32 p1, const float (&dc)[QG],
                                                         const u32 (&sbase)[QG], const u32 *(&row)[QG], int nvalid, S (&sel)[QG], int K,
                                                         int wv, int lane, u64 *sthr)
{
    u32 thr_hi[QG];
#pragma unroll
    for (int s = 0; s < QG; ++s) {
        sel[s].tighten(readfirstlane64(sthr[s]));
        thr_hi[s] = (u32)(sel[s].thr() >> 32);
    }
    const int nw = cs >> 2;
    for (u32 pb = p0 + wv * 64; pb < p1; pb += 256) {
        const u32 p = pb + lane;
        bool ok[QG], any = false;
#pragma unroll
        for (int s = 0; s < QG; ++s) {
            ok[s] = p < p1 && s < nvalid && ((mask_round(row[s], pb) >> lane) & 1ull) != 0ull;
            any = any || ok[s];
        }
        if (!__any(any)) continue;   // uniform: the round is rejected for every valid slot -- no code loads, no lookups
        float acc[QG];
#pragma unroll
        for (int s = 0; s < QG; ++s) acc[s] = dc[s];
        if (any) {
            const u32 *cp = (const u32 *)(cbase + (size_t)p * cs);
            for (int wd = 0; wd < nw; ++wd) {
                const u32 dw = cp[wd];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int ii = wd * 4 + b;
                    if (ii < m) {
                        const u32 byte = (dw >> (8 * b)) & 0xffu;
                        float tv[QG];
                        TabV<QG>::ld(tab + ((size_t)ii * 256 + byte) * QG, tv);
#pragma unroll
                        for (int s = 0; s < QG; ++s) acc[s] = acc[s] + tv[s];
                    }
                }
            }
        }
        bool anyc = false;
#pragma unroll
        for (int s = 0; s < QG; ++s) anyc = anyc || (ok[s] && __float_as_uint(acc[s]) <= thr_hi[s]);
        if (__any(anyc)) {
#pragma unroll
            for (int s = 0; s < QG; ++s) sel[s].tighten(readfirstlane64(sthr[s]));
#pragma unroll
            for (int s = 0; s < QG; ++s) {   // slot by slot: validity is the slot's own
                const float acc1[1] = {acc[s]};
                const u32 sb1[1] = {sbase[s]};
                scan_emit<1>(acc1, p, ok[s], 1, sb1, reinterpret_cast<S(&)[1]>(sel[s]), K, lane);
            }
#pragma unroll
            for (int s = 0; s < QG; ++s) {
                publish_bound<QG>(sthr, s, sel[s], K, (u32)(sel[s].thr() >> 32) < thr_hi[s], lane);
                thr_hi[s] = (u32)(sel[s].thr() >> 32);
            }
        }
    }
}

template <int QG, bool SMALL>
__global__ __launch_bounds__(256) void masked_scan_kernel(const ScanArgs a, const MaskView mv)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const IndexView &ix = a.ix;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m = ix.m;
    const int K = a.K, cap = a.cap;
    const LdsCarve L = carve_lds<QG, SMALL>(smem_raw, m, ix.d, cap, 0);
    const bool direct = QG == 1 && a.direct_items != 0;
    const u32 total = direct ? a.direct_items : a.wi_off[ix.kc];

    for (;;) {
        __syncthreads();
        if (tid == 0) L.swi[0] = atomicAdd(a.queue_head, 1u);
        __syncthreads();
        const u32 wi = __builtin_amdgcn_readfirstlane(L.swi[0]);
        if (wi >= total) break;   // uniform

        int l;
        u32 cnt, chunk, grp, direct_probe = 0;
        if (direct) {   // (rank-major order: see scan_kernel)
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
            const u32 ng = (cnt + QG - 1) / QG;
            const u32 local = wi - a.wi_off[l];
            chunk = local / ng;
            grp = local - chunk * ng;
        }
        const u32 len = ix.list_len[l];
        const u32 p0 = chunk * a.CH;   // (CH is a multiple of 1024: whole rounds)
        if (p0 >= len) continue;   // uniform
        const u32 p1 = min(len, p0 + a.CH);
        const int nvalid = min((int)QG, (int)(cnt - grp * QG));

        u32 pidx[QG], sbase[QG];
        int qi[QG];
        float dc[QG];
        u64 hard[QG];
        const u32 *row[QG];
        WSel<SMALL> sel[QG];
#pragma unroll
        for (int s = 0; s < QG; ++s) {
            const int ss = s < nvalid ? s : 0;
            pidx[s] = direct ? direct_probe : a.bucket_items[a.bucket_off[l] + grp * QG + ss];
            qi[s] = (int)(pidx[s] / (u32)a.w);
            dc[s] = a.probe_dc[pidx[s]];
            sbase[s] = a.probe_base[pidx[s]];
            row[s] = mask_row(mv, qi[s], l);
            const u64 t0 = readfirstlane64(__hip_atomic_load(&a.qthr[qi[s]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            sel[s].init(t0, SMALL ? nullptr : L.selbuf + ((size_t)wv * QG + s) * cap, cap, K);
            hard[s] = t0;
            if (tid == 0) arm_bound<QG>(L.sthr, s, t0);    // published by the barrier after the residuals
        }

        // exact pruning as in scan_kernel: the bounds come from selected points only, so a bound below dc still means nothing to gain here
        if (a.prune) {
            if (tid == 0) {
                bool all = true;
#pragma unroll
                for (int s = 0; s < QG; ++s) all = all && (s >= nvalid || __float_as_uint(dc[s]) > (u32)(hard[s] >> 32));
                L.swi[1] = all ? 1u : 0u;
            }
            __syncthreads();
            if (L.swi[1] != 0u) {   // uniform
                if (tid < nvalid) {
                    u32 pi = pidx[0];
#pragma unroll
                    for (int s = 1; s < QG; ++s) pi = tid == s ? pidx[s] : pi;
                    a.part_cnt[(size_t)pi * a.maxch + chunk] = 0u;
                    atomicAdd(a.scanned_points + (size_t)(pi & 63u) * 8 + 1, (u64)(p1 - p0));
                }
                continue;
            }
        }
        int li[QG];
#pragma unroll
        for (int s = 0; s < QG; ++s) li[s] = l;
        const uint8_t *cbase = ix.codes + ix.list_codeoff[l];
        build_residuals<QG>(ix, a.queries, qi, li, L.resid, tid);
        __syncthreads();
        build_tables_t<QG, 0, TAB_INTERLEAVED>(ix, m, L.resid, L.tab, tid);
        __syncthreads();

        masked_scan_range<QG>(L.tab, cbase, ix.cs, m, p0, p1, dc, sbase, row, nvalid, sel, K, wv, lane, L.sthr);

        // ---- per-wave flush, then wave s merges slot s of the four waves and publishes it (a slot with no selected point: count 0)
        int mycnt[QG];
#pragma unroll
        for (int s = 0; s < QG; ++s) mycnt[s] = sel[s].finish(K, lane);
        if (SMALL) __syncthreads();   // the exchange area aliases the tables: every wave must be done scanning
#pragma unroll
        for (int s = 0; s < QG; ++s) {
            sel[s].store(L.xch + ((size_t)wv * QG + s) * L.xcap, mycnt[s], lane);
            if (lane == 0) L.scnt[wv * QG + s] = mycnt[s];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < QG; ++s) {
            if (s == wv && s < nvalid) {
                merge_waves(sel[s], L.xch + (size_t)s * L.xcap, (size_t)QG * L.xcap, L.scnt + s, QG, K, hard[s], wv, lane);
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

typedef void (*masked_fn_t)(const ScanArgs, const MaskView);

}  // namespace ivf
