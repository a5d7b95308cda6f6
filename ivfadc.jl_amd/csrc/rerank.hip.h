// rerank.hip.h -- exact re-ranking (ivfadc_rerank, ivfadc_search_refined; IVFADC+R): candidate ids re-scored against the ORIGINAL vectors
// of a vector store (ivfadc_vectors_t), the K best kept.  gfx950, wave64.  Plan, pair arithmetic, LDS layout: rerank_plan.h.
//
//   rerank_dist_kernel<F16, VEC>   grid (tiles of candidates, queries); a wave owns 64 consecutive slots of one query.  The distance is
//                        DEFINED as a chain sequential in t, Float32, one rounding per operation (the build's -ffp-contract=off covers this
//                        file), the chain of the coarse distance (coarsequantizers.jl:33-34):
//                          s = 0;  t ascending:  u = x_v[t] - q[t];  s = s + u * u
//                        so a row cannot be reduced across lanes, and one lane per row read straight from HBM would turn every wave load
//                        into 64 different cache lines of which it uses 4 or 16 bytes.  Instead the wave FETCHES its 64 rows together,
//                        one 128-byte line of each row per chunk: eight lanes of 16 bytes cover a row's line, a wave load brings eight
//                        whole lines, eight loads bring the chunk of all 64 rows.  The chunk goes into the wave's LDS tile, [row][dword],
//                        row stride 33 dwords, and lane r then advances ITS row's chain over the chunk, reading dword t of row r (no bank
//                        conflict beyond the two lanes per bank of any wave64 read) against the query chunk, an LDS broadcast.
//                        The loads of chunk c + 1 are issued into 32 staging registers per lane BEFORE chunk c is consumed and are
//                        written to the tile after it: the second buffer of the pipeline is the register file, not a second LDS tile,
//                        which keeps a workgroup at 33 KB + the query and four workgroups on a CU -- for random HBM reads the bytes in
//                        flight per CU are what counts (reasoned; not measured against a second tile).  The tile is private to its wave:
//                        wave_sync, no workgroup barrier in the loop.
//                        A dead slot (at or behind counts[q]) and an id at or beyond n load nothing and carry the all-ones key.
//                        VEC false: rows whose byte length is no multiple of 16 (d = 10) are fetched one component per load into the
//                        same tile.  F16: a line holds 64 components; a component is widened exactly on its way into the chain.
//                        Output: one key per slot, f32_bits(s) << 32 | slot -- the project's key order with the slot as visit order.
//                        NO MATRIX INSTRUCTIONS: every query has its own rows, so a tile has no shared operand; and the form
//                        ||x||^2 - 2 x.q + ||q||^2 that would make one changes the rounding the result is defined by.
//   rerank_select_kernel<SORTED>   one workgroup per query.  SORTED false (C <= 4096): the keys go into LDS, padded to a power of two with
//                        all-ones; every 64-key run is sorted in registers (wave_sort64), then merge widths 128 .. P: the flip stage and
//                        the strides >= 64 in LDS, the strides 32 .. 1 in registers again.  SORTED true: the row was sorted by the
//                        segmented radix sort of the generic search path.  Then the first min(K, live) keys are emitted with the id of
//                        their slot and their distance bits.
//   vectors_to_f16_kernel   the Float16 store: round-to-nearest-even, one flag raised (plain atomic OR) when a FINITE component overflows.
// Plain C++ and vector loads and stores only.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.hip.h"
#include "rerank_plan.h"

namespace ivf {

struct RerankArgs {
    const uint8_t *rows;      // the store: n rows of d components
    uint64_t n;
    int d;
    const float *queries;     // d x (all queries of the call)
    const u32 *ids;           // nq x C
    const int32_t *counts;    // null: every slot is live
    int64_t C;
    int64_t q0;               // first query of this slice (blockIdx.y counts from it)
    u64 *keys;                // the slice's keys, rerank::key_index
};

// one step of the chain: u = x - y; acc = acc + u * u
__device__ __forceinline__ float rerank_step(float acc, float x, float y)
{
    const float u = x - y;
    return acc + u * u;
}

__device__ __forceinline__ float rerank_widen(u32 half_bits) { return (float)__builtin_bit_cast(_Float16, (unsigned short)half_bits); }

// the 16 bytes of chunk c this lane fetches of the row at byte offset `row` (ok false: nothing is read)
template <bool F16, bool VEC>
__device__ __forceinline__ uint4 rerank_fetch(const RerankArgs &a, bool ok, uint64_t row, int c, int lane)
{
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (!ok) return r;
    const uint8_t *__restrict__ p = a.rows + row;
    const int dw0 = rerank::gather_dword(lane, 0);
    if constexpr (VEC) {
        const uint64_t b = rerank::chunk_byte(c, dw0);
        if (b < rerank::row_bytes(a.d, F16)) r = *(const uint4 *)(p + b);
    } else {
        u32 w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t dw = (int64_t)c * rerank::CHUNK_DWORDS + dw0 + k;   // dword of the row
            w[k] = 0u;
            if constexpr (F16) {
                const unsigned short *hp = (const unsigned short *)p;
                if (2 * dw < a.d) w[k] = hp[2 * dw];
                if (2 * dw + 1 < a.d) w[k] |= (u32)hp[2 * dw + 1] << 16;
            } else {
                if (dw < a.d) w[k] = ((const u32 *)p)[dw];
            }
        }
        r = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return r;
}

// lane r's chain over the `len` components of a chunk: tile row r against the query chunk qc
template <bool F16>
__device__ __forceinline__ float rerank_consume(float s, const u32 *__restrict__ row, const float *__restrict__ qc, int len)
{
    if (len == rerank::chunk_elems(F16)) {
#pragma unroll
        for (int w = 0; w < rerank::CHUNK_DWORDS; ++w) {
            const u32 x = row[w];
            if constexpr (F16) {
                s = rerank_step(s, rerank_widen(x & 0xFFFFu), qc[2 * w]);
                s = rerank_step(s, rerank_widen(x >> 16), qc[2 * w + 1]);
            } else {
                s = rerank_step(s, __uint_as_float(x), qc[w]);
            }
        }
    } else {
        for (int t = 0; t < len; ++t) {
            if constexpr (F16) {
                const u32 x = row[t >> 1];
                s = rerank_step(s, rerank_widen((t & 1) ? x >> 16 : x & 0xFFFFu), qc[t]);
            } else {
                s = rerank_step(s, __uint_as_float(row[t]), qc[t]);
            }
        }
    }
    return s;
}

template <bool F16, bool VEC>
__global__ __launch_bounds__(rerank::TILE) void rerank_dist_kernel(const RerankArgs a)
{
    extern __shared__ __align__(16) u32 rr_lds[];
    float *qs = (float *)rr_lds;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t qy = blockIdx.y, q = a.q0 + qy;
    const float *__restrict__ qrow = a.queries + rerank::query_row(q, a.d);
    for (int t = tid; t < a.d; t += rerank::TILE) qs[t] = qrow[t];
    __syncthreads();
    const int64_t j = rerank::tile_slot(blockIdx.x, tid);
    const int64_t live = rerank::live_slots(a.counts != nullptr, a.counts ? a.counts[q] : 0, a.C);
    u32 v = 0u;
    bool ok = false;
    if (j < live) {
        v = a.ids[rerank::id_index(q, a.C, j)];
        ok = (uint64_t)v < a.n;
    }
    const u64 mask = __ballot(ok);   // wave-uniform from here on
    float s = 0.0f;
    if (mask != 0ull) {
        u32 *tile = rr_lds + rerank::tile_base(a.d, wv);
        // the rows this lane fetches a piece of: row gather_row(lane, i) of the wave's 64
        uint64_t frow[rerank::LOADS];
        bool fok[rerank::LOADS];
#pragma unroll
        for (int i = 0; i < rerank::LOADS; ++i) {
            const int r = rerank::gather_row(lane, i);
            frow[i] = rerank::row_offset((uint64_t)(u32)__shfl((int)v, r), a.d, F16);
            fok[i] = (mask >> r) & 1ull;
        }
        const int nch = rerank::chunks(a.d, F16);
        uint4 st[rerank::LOADS];
#pragma unroll
        for (int i = 0; i < rerank::LOADS; ++i) st[i] = rerank_fetch<F16, VEC>(a, fok[i], frow[i], 0, lane);
        for (int c = 0; c < nch; ++c) {
            // the staged chunk c into the tile (the reads of chunk c - 1 are behind the wave_sync that ended its turn)
#pragma unroll
            for (int i = 0; i < rerank::LOADS; ++i) {
                u32 *dst = tile + rerank::tile_index(rerank::gather_row(lane, i), rerank::gather_dword(lane, 0));
                dst[0] = st[i].x; dst[1] = st[i].y; dst[2] = st[i].z; dst[3] = st[i].w;
            }
            wave_sync();
            if (c + 1 < nch) {
#pragma unroll
                for (int i = 0; i < rerank::LOADS; ++i) st[i] = rerank_fetch<F16, VEC>(a, fok[i], frow[i], c + 1, lane);
            }
            s = rerank_consume<F16>(s, tile + rerank::tile_index(lane, 0), qs + (size_t)c * rerank::chunk_elems(F16), rerank::chunk_len(a.d, F16, c));
            wave_sync();
        }
    }
    if (j < a.C) a.keys[rerank::key_index(qy, a.C, j)] = ok ? (((u64)__float_as_uint(s) << 32) | (u32)j) : (u64)KEY_MAX;
}

// the tail of a merge inside a 64-key run: strides 32 .. 1, the minimum to the lower lane
static __device__ __forceinline__ u64 rerank_merge_tail(u64 v, int lane)
{
    v = sort_stage<32>(v, lane); v = sort_stage<16>(v, lane); v = sort_stage<8>(v, lane);
    v = sort_stage<4>(v, lane);  v = sort_stage<2>(v, lane);  v = sort_stage<1>(v, lane);
    return v;
}

__device__ __forceinline__ void rerank_cmpx(u64 *keys, int lo, int hi)
{
    const u64 x = keys[lo], y = keys[hi];
    if (y < x) { keys[lo] = y; keys[hi] = x; }
}

// keys: the slice's keys (SORTED: each row ascending already); P: rerank::padded_keys(C) (SORTED: unused); ids: nq x C of the call;
// out_*: nq x K, nq x K, nq of the call.  Slots at or behind out_counts[q] are not written.
template <bool SORTED>
__global__ __launch_bounds__(256) void rerank_select_kernel(const u64 *__restrict__ keys, int64_t C, int P, int64_t q0, const u32 *__restrict__ ids,
                                                            int K, u32 *__restrict__ out_ids, float *__restrict__ out_dists,
                                                            int32_t *__restrict__ out_counts)
{
    extern __shared__ __align__(16) u64 rr_keys[];
    __shared__ int s_live;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t qy = blockIdx.x, q = q0 + qy;
    const u64 *__restrict__ row = keys + rerank::key_index(qy, C, 0);
    const u64 *sorted = row;
    int64_t live = 0;
    if constexpr (SORTED) {
        // the keys that are not all ones stand first
        int64_t lo = 0, hi = C;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (row[mid] != KEY_MAX) lo = mid + 1; else hi = mid;
        }
        live = lo;
    } else {
        if (tid == 0) s_live = 0;
        __syncthreads();
        int mine = 0;
        for (int r0 = wv * 64; r0 < P; r0 += 256) {
            const int i = r0 + lane;
            const u64 key = i < C ? row[i] : (u64)KEY_MAX;
            mine += __popcll(__ballot(key != KEY_MAX));
            rr_keys[i] = wave_sort64(key, lane);
        }
        if (lane == 0 && mine) atomicAdd(&s_live, mine);
        __syncthreads();
        for (int k = 128; k <= P; k <<= 1) {
            for (int p = tid; p < P / 2; p += 256) {
                int lo, hi;
                rerank::flip_pair(p, k, lo, hi);
                rerank_cmpx(rr_keys, lo, hi);
            }
            __syncthreads();
            for (int jj = k >> 2; jj >= 64; jj >>= 1) {
                for (int p = tid; p < P / 2; p += 256) {
                    int lo, hi;
                    rerank::stride_pair(p, jj, lo, hi);
                    rerank_cmpx(rr_keys, lo, hi);
                }
                __syncthreads();
            }
            for (int r0 = wv * 64; r0 < P; r0 += 256) rr_keys[r0 + lane] = rerank_merge_tail(rr_keys[r0 + lane], lane);
            __syncthreads();
        }
        live = s_live;
        sorted = rr_keys;
    }
    const int cnt = live < (int64_t)K ? (int)live : K;
    for (int i = tid; i < cnt; i += 256) {
        const u64 key = sorted[i];
        out_ids[rerank::out_index(q, K, i)] = ids[rerank::id_index(q, C, (int64_t)(u32)key)];
        out_dists[rerank::out_index(q, K, i)] = __uint_as_float((u32)(key >> 32));
    }
    if (tid == 0) out_counts[q] = cnt;
}

// segment offsets of the sort form: row i of the slice starts at i * C (n + 1 entries; n * C < 2^31)
__global__ __launch_bounds__(256) void rerank_offsets_kernel(u32 *__restrict__ off, int64_t n, int64_t C)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= n) off[i] = (u32)(i * C);
}

// a call with no candidate slots: every query finds nothing (a kernel, not a memset: the device entries may be captured into a graph)
__global__ __launch_bounds__(256) void rerank_zero_counts_kernel(int32_t *__restrict__ out_counts, int64_t nq)
{
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) out_counts[q] = 0;
}

// src: total Float32 components -> dst: their Float16 bits, round-to-nearest-even.  *flag |= 1 when a finite component became infinite.
__global__ __launch_bounds__(256) void vectors_to_f16_kernel(const float *__restrict__ src, uint64_t total, unsigned short *__restrict__ dst,
                                                             u32 *__restrict__ flag)
{
    bool over = false;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
        const float x = src[e];
        const unsigned short h = __builtin_bit_cast(unsigned short, (_Float16)x);
        over |= (h & 0x7FFFu) == 0x7C00u && (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u;
        dst[e] = h;
    }
    if (over) atomicOr(flag, 1u);
}

}  // namespace ivf
