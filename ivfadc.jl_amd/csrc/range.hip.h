// range.hip.h -- range search (ivfadc_range_search): every point of the w probed lists within Float32 distance r of the query.
//
// NO REFERENCE COUNTERPART: IVFADC.jl has knn_search only.  The definition is knn_search (index.jl:204-258) with K at
// least the number of probed points, cut after the last entry with d <= r (inclusive, as NearestNeighbors.jl's inrange): the same w
// cells, the same sums (d = dc, then += tab_ii[code[ii]] in ascending ii), the same order (distance, probe rank, list position), the
// same stored ids.  No selection structure and no bound but the radius: two passes over one grid of work items (range_plan.h),
//   count:  survivors of every item, one u32 each;
//   (range_offsets_kernel: exclusive scan of a query's items, the query's total)
//   fill:   every survivor's key f32_bits(d) << 32 | visit order into the item's slot range, in any order -- keys are unique,
// then the segmented radix sort of the generic path over the survivors only, and range_emit_kernel: keys -> ids and distances (CSR).
// Plain C++ and vector stores only.
//
// range_scan_item is ONE body, a template on (pass, distance form, masked); six kernels are its instantiations:
//   range_count_kernel / range_fill_kernel                 8-bit codes, no mask (ivfadc_range_search, as before)
//   range_masked_count_kernel / range_masked_fill_kernel   8-bit codes, a mask row per (query, list) (ivfadc_range_search_masked)
//   range_u16_count_kernel / range_u16_fill_kernel         16-bit codes, table-free, with or without a mask set (a null set: no row)
// Distance forms.  TABLES (8-bit): residual and m x 256 tables in LDS, dword code loads.  TABLE-FREE (16-bit; u16scan.hip.h's
// arithmetic, one point per lane, one query per item): the residual lies in LDS as [m][dsp]; a point gathers the codeword its code names
// from codebooks ([m][ksub][dsub]; 16-byte groups where dsub % 4 == 0, single floats otherwise), forms the sub-space sum in its own
// accumulator from zero (df = cw[t] - r[t]; sum = sum + df * df, t ascending) and adds it to the running sum afterwards: the table
// entry's expression, hence its bits.  Exact early-out: terms are >= +0 and Float32 addition of a non-negative term never decreases a
// sum, so a lane whose running sum is above r (strictly: a point whose remaining terms are all +0 and whose partial sum equals r
// belongs to the result) can never pass and stops gathering; a wave leaves the sub-space loop when no lane is alive.
// Mask test.  A chunk begins at a multiple of 64 (range_plan.h's invariant), so the 64 points of a wave's round are one round of the
// mask row: two whole words (mask_round).  A lane is valid iff p < p1 and its bit is set; a wave without a valid lane loads no code and
// looks nothing up.  Count and fill see the same lanes.  The probe skip stays exact: removing points cannot make a survivor appear.
#pragma once
#include "kernels.hip.h"
#include "maskset.hip.h"
#include "range_plan.h"

namespace ivf {

struct RangeArgs {
    IndexView ix;
    const float *queries;     // the launch's queries, [gridDim.y][d]
    const float *radii;       // [gridDim.y]
    int w;
    u32 chunk, maxch;
    const int *probe_list;    // [gridDim.y][w]
    const float *probe_dc;
    const u32 *probe_base;
    u32 *item_cnt;            // [gridDim.y][gridDim.x]: written by the count pass, read by the fill pass
    const u32 *item_off;      // fill pass: exclusive scan of item_cnt within the query
    const u32 *key_off;       // fill pass: first key of every query in `keys`
    u64 *keys;
};

// One work item: (query blockIdx.y, probe j, chunk c), blockIdx.x = j * maxch + c.  U16: the table-free form over 16-bit codes (codeword
// indices: no label lookup); MASKED: mv may hold a set (mv.words null: no query is filtered) and the mask numbers of THIS launch's queries.
template <bool FILL, bool U16, bool MASKED> static __device__ __forceinline__ void range_scan_item(const RangeArgs &a, const MaskView &mv)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const IndexView &ix = a.ix;
    const int dsp = (ix.dsub + 3) & ~3;
    float *resid = (float *)smem_raw;                          // tables: [d]; table-free: [m][dsp]
    float *tab = resid + (((size_t)ix.d + 3) & ~(size_t)3);    // [m][256] (tables only)
    u32 *s_cnt = U16 ? (u32 *)(resid + (size_t)ix.m * dsp) : (u32 *)(tab + (size_t)ix.m * 256);   // survivors of the item so far
    const int tid = threadIdx.x, lane = tid & 63, q = blockIdx.y;
    const u32 j = (u32)range_plan::probe_of(blockIdx.x, a.maxch), c = (u32)range_plan::chunk_of(blockIdx.x, a.maxch);
    const size_t it = (size_t)q * gridDim.x + blockIdx.x;
    const int l = a.probe_list[(size_t)q * a.w + j];
    const uint64_t len = ix.list_len[l];
    const uint64_t p0 = range_plan::chunk_begin(c, a.chunk), p1 = range_plan::chunk_end(len, c, a.chunk);
    const float r = a.radii[q];
    const float dc = a.probe_dc[(size_t)q * a.w + j];
    // Everything below is uniform within the item.  r < 0 or NaN: no results.  dc > r: no point of this probe can pass -- table entries
    // are non-negative and Float32 addition of a non-negative term never decreases a sum, so d >= dc > r (exact, not a heuristic).
    bool live = p0 < p1 && range_plan::radius_live(r) && !(dc > r);
    u32 limit = 0;
    if (FILL) {
        limit = live ? a.item_cnt[it] : 0u;   // an item without survivors builds nothing
        live = limit != 0;
    }
    if (!live) {
        if (!FILL && tid == 0) a.item_cnt[it] = 0;
        return;
    }
    const u32 rb = range_plan::radius_bits(r, __float_as_uint(r));
    // residual (coarsequantizers.jl:40-45) and tables (index.jl:232-236) in the reference's sum order, through the labels: gen_dump_kernel's
    if (U16) {
        for (int i = tid; i < ix.d; i += 256) {
            const int ii = i / ix.dsub;
            resid[ii * dsp + (i - ii * ix.dsub)] = a.queries[(size_t)q * ix.d + i] - ix.centroids[(size_t)l * ix.d + i];
        }
    } else {
        for (int i = tid; i < ix.d; i += 256) resid[i] = a.queries[(size_t)q * ix.d + i] - ix.centroids[(size_t)l * ix.d + i];
    }
    if (tid == 0) *s_cnt = 0;
    __syncthreads();
    if (!U16) {
        for (int e = tid; e < ix.m * 256; e += 256) {
            const int ii = e >> 8, cw_i = e & 255;
            if (cw_i < ix.ksub) {
                const float *cw = ix.codebooks + ((size_t)ii * ix.ksub + cw_i) * ix.dsub;
                const float *rr = resid + (size_t)ii * ix.dsub;
                float sum = 0.0f;
                for (int t = 0; t < ix.dsub; ++t) {
                    const float df = cw[t] - rr[t];
                    sum = sum + df * df;
                }
                tab[ii * 256 + (ix.identity_labels ? cw_i : (int)ix.labels[ii * ix.ksub + cw_i])] = sum;
            }
        }
        __syncthreads();
    }
    const uint8_t *codes = ix.codes + ix.list_codeoff[l];    // 256-byte aligned, stride cs a multiple of 4: dword loads
    const u32 base = a.probe_base[(size_t)q * a.w + j];
    u64 *dst = FILL ? a.keys + a.key_off[q] + a.item_off[it] : (u64 *)nullptr;
    // the row of this query's mask for this list, taken once per item: null for -1 and for a null set
    const u32 *row = (MASKED && mv.words) ? mask_row(mv, q, l) : (const u32 *)nullptr;
    const bool al4 = (ix.dsub & 3) == 0;
    u32 mine = 0;   // count pass: survivors this wave has seen
    for (uint64_t pb = p0; pb < p1; pb += 256) {
        const uint64_t p = pb + (uint64_t)tid;
        bool valid = p < p1;   // nothing at or behind list_len is read
        if (MASKED) {
            // p0 is a multiple of 64 (range_plan.h), so this wave's 64 points are one round of the row: two whole words.  A round that
            // begins at or behind p1 has no lane (and may have no words).
            const uint64_t pw = pb + (uint64_t)(tid & ~63);
            if (row && pw < p1) valid = valid && ((mask_round(row, (u32)pw) >> lane) & 1ull) != 0ull;
            if (__ballot(valid) == 0) continue;   // uniform within the wave: no code loads, no lookups (no barrier inside this loop)
        }
        bool hit = false;
        float dist = dc;
        if (!U16) {
            if (valid) {
                const u32 *cp = (const u32 *)(codes + (size_t)p * ix.cs);
                for (int i0 = 0; i0 < ix.m; i0 += 4) {
                    const u32 wd = cp[i0 >> 2];
                    const int nt = min(4, ix.m - i0);
                    for (int t = 0; t < nt; ++t) dist = dist + tab[(i0 + t) * 256 + (int)((wd >> (8 * t)) & 255u)];
                }
                hit = __float_as_uint(dist) <= rb;   // both non-negative and no NaN: the bit patterns order as the values do
            }
        } else {
            // table-free: a lane without a point reads neither a code nor a codeword.  alive: the running sum is not above r yet
            // (dc <= r: the probe skip above)
            bool alive = valid;
            const u32 *cp = (const u32 *)(codes + (size_t)p * ix.cs);
            u32 wd = 0;
            for (int ii = 0; ii < ix.m; ++ii) {
                if (__ballot(alive) == 0) break;   // uniform within the wave
                if (alive) {
                    if ((ii & 1) == 0) wd = cp[ii >> 1];   // two codes a dword; cs covers m codes rounded up to a dword
                    const int c = min((int)((wd >> (16 * (ii & 1))) & 0xffffu), ix.ksub - 1);   // clamped before it becomes an address
                    const float *cw = ix.codebooks + ((size_t)ii * ix.ksub + c) * ix.dsub;
                    const float *rr = resid + ii * dsp;
                    float sum = 0.0f;   // the sub-space sum: its own accumulator from zero, added afterwards
                    if (al4) {
                        for (int t = 0; t < ix.dsub; t += 4) {
                            const float4 cv = *(const float4 *)(cw + t);
                            const float4 rv = *(const float4 *)(rr + t);   // the same address in every lane: a broadcast read
                            float df = cv.x - rv.x;
                            sum = sum + df * df;
                            df = cv.y - rv.y;
                            sum = sum + df * df;
                            df = cv.z - rv.z;
                            sum = sum + df * df;
                            df = cv.w - rv.w;
                            sum = sum + df * df;
                        }
                    } else {
                        for (int t = 0; t < ix.dsub; ++t) {
                            const float df = cw[t] - rr[t];
                            sum = sum + df * df;
                        }
                    }
                    dist = dist + sum;
                    alive = __float_as_uint(dist) <= rb;   // strict: the lane stops only when bits(dist) > rb
                }
            }
            hit = alive;
        }
        const u64 bal = __ballot(hit);
        if (!FILL) {
            mine += (u32)__popcll(bal);
        } else if (bal != 0) {
            // the survivors of this wave's round take consecutive slots from ONE atomic on the item's counter
            u32 first = 0;
            if (lane == 0) first = atomicAdd(s_cnt, (u32)__popcll(bal));
            first = (u32)__shfl((int)first, 0);
            if (hit) {
                const u32 slot = first + (u32)__popcll(bal & (((u64)1 << lane) - 1));
                if (slot < limit) dst[slot] = ((u64)__float_as_uint(dist) << 32) | (u64)(base + (u32)p);   // (slot < limit always: the count pass saw the same points)
            }
        }
    }
    if (!FILL) {
        if (lane == 0 && mine != 0) atomicAdd(s_cnt, mine);
        __syncthreads();
        if (tid == 0) a.item_cnt[it] = *s_cnt;
    }
}

__global__ __launch_bounds__(256) void range_count_kernel(const RangeArgs a) { range_scan_item<false, false, false>(a, MaskView{}); }
__global__ __launch_bounds__(256) void range_fill_kernel(const RangeArgs a) { range_scan_item<true, false, false>(a, MaskView{}); }
// ivfadc_range_search_masked: 8-bit codes with a set; 16-bit codes with a set or without (mv.words null)
__global__ __launch_bounds__(256) void range_masked_count_kernel(const RangeArgs a, const MaskView mv) { range_scan_item<false, false, true>(a, mv); }
__global__ __launch_bounds__(256) void range_masked_fill_kernel(const RangeArgs a, const MaskView mv) { range_scan_item<true, false, true>(a, mv); }
__global__ __launch_bounds__(256) void range_u16_count_kernel(const RangeArgs a, const MaskView mv) { range_scan_item<false, true, true>(a, mv); }
__global__ __launch_bounds__(256) void range_u16_fill_kernel(const RangeArgs a, const MaskView mv) { range_scan_item<true, true, true>(a, mv); }
typedef void (*range_masked_fn_t)(const RangeArgs, const MaskView);

// Exclusive scan of the item counts of every query (one workgroup each), and the query's total.  A query probes fewer than 2^32 points
// (range_plan.h), so 32 bits hold every sum.
__global__ __launch_bounds__(256) void range_offsets_kernel(const u32 *__restrict__ item_cnt, u32 nitems, u32 *__restrict__ item_off,
                                                            u32 *__restrict__ totals)
{
    __shared__ u32 s_part[256];
    __shared__ u32 s_run;
    const int q = blockIdx.x, tid = threadIdx.x;
    const u32 *cnt = item_cnt + (size_t)q * nitems;
    u32 *off = item_off + (size_t)q * nitems;
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (u32 i0 = 0; i0 < nitems; i0 += 256) {
        const u32 i = i0 + (u32)tid;
        const u32 v = i < nitems ? cnt[i] : 0u;
        s_part[tid] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {   // inclusive scan (Hillis-Steele), as gen_probes_kernel
            const u32 x = tid >= o ? s_part[tid - o] : 0u;
            __syncthreads();
            s_part[tid] += x;
            __syncthreads();
        }
        const u32 run = s_run;
        if (i < nitems) off[i] = run + s_part[tid] - v;
        __syncthreads();
        if (tid == 0) s_run = run + s_part[255];
        __syncthreads();
    }
    if (tid == 0) totals[q] = s_run;
}

// sorted keys of every query of a group -> ids and distances at lims[q] (index.jl:248,252,257 through emit_result); grid (queries, y)
__global__ __launch_bounds__(256) void range_emit_kernel(const u64 *__restrict__ sorted, const u32 *__restrict__ key_off, int w,
                                                         const int *__restrict__ probe_list, const u32 *__restrict__ probe_base,
                                                         const int64_t *__restrict__ list_pos, const u32 *__restrict__ ids,
                                                         const int64_t *__restrict__ lims, u32 *__restrict__ out_ids,
                                                         float *__restrict__ out_dists)
{
    const int q = blockIdx.x;
    const u32 k0 = key_off[q], cnt = key_off[q + 1] - k0;
    const u64 *row = sorted + k0;
    u32 *oi = out_ids + lims[q];
    float *od = out_dists + lims[q];
    for (u32 i = blockIdx.y * 256u + threadIdx.x; i < cnt; i += gridDim.y * 256u)
        emit_result(row[i], 0, 0, w, 0, probe_list + (size_t)q * w, probe_base + (size_t)q * w, list_pos, ids, oi + i, od + i);   // (slot i of a CSR row: K-strided addressing is not used)
}

}  // namespace ivf
