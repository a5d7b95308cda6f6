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
//   rerank_pq_dist_kernel<VEC, STAGED>   the distance pass against a PQ store (store_type 2; vstore_pq_plan.h): the same decomposition, but a row
//                        is not fetched, it is RECONSTRUCTED.  The wave first brings its 64 records (8 .. 128 bytes each) into LDS, in
//                        16-byte pieces, consecutive lanes on consecutive pieces.  Per chunk, the eight lanes of a row then each build
//                        four components: a 16-byte piece of the centroid row, one of the base codeword of sub-space t / dsub, one of
//                        the refinement codeword of sub-space t / dsub2 (all three read-only, a few hundred KB, served by the L2), two
//                        additions, y = (c + p) + r, and the write into the tile.  Chunk c + 1 is reconstructed into the staging
//                        registers before chunk c is consumed, as the fetch of the other stores is.  VEC false (dsub or dsub2 no
//                        multiple of four): the four components are addressed one by one.  The chain itself is rerank_consume's.
//                        STAGED (the other codebook route, on request: ivfadc_vectors_set_pq_route): per chunk the workgroup first copies
//                        the chunk's slices of both codebooks into LDS (2 x 32 KB at k = 256) and the codeword pieces come from there.
//   vstore_pq_encode_kernel        creation of a PQ store, one workgroup per row, the row's residual in LDS throughout: the base code
//                        (encode_kernel's chain and tie rule on x - c), the second residual e = x - (c + p), optionally written out for
//                        the trainer, the refinement code (the same chain on e), and the record.  Nothing but the record goes to memory.
//   rerank_sq_dist_kernel          the distance pass against an 8-bit scalar-quantised store (store_type 3; vstore_sq_plan.h): the same
//                        decomposition and the same fetch, but a row's 128-byte line is now 128 components, so a d = 128 row is ONE line
//                        where the Float16 store reads two.  Lane r takes dword w of its tile row apart with four byte-extract
//                        conversions and decodes each code on its way into the chain, y = lo[t] + (float)c * step[t]; the chunk's q,
//                        lo and step are wave-uniform LDS reads of 16 bytes (broadcasts), all three whole in LDS beside the tiles.  Rows
//                        are padded to 16 bytes, so the kernel has one form and no VEC twin.
//   vstore_sq_range_kernel         per-dimension minimum and maximum of a block of rows for a trained range: consecutive lanes on
//                        consecutive columns, a running min / max per lane over the rows of its workgroup, then one atomic min and one
//                        atomic max per column and workgroup on order-preserving unsigned images of the floats -- exact, the same for
//                        any grid.  A non-finite component raises a flag (plain atomic OR).
//   vstore_sq_encode_kernel        one lane per 16 output bytes: four float4 loads, sixteen codes c = min(255, max(0, rintf((x - lo) * inv))),
//                        one uint4 store; lo / inv from LDS when they fit, through the L2 otherwise; the last piece of a row carries
//                        its zero padding.  The same flag.  The device never divides: step and inv come from the host.
// Plain C++ and vector loads and stores only.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.hip.h"
#include "rerank_plan.h"
#include "vstore_pq_plan.h"
#include "vstore_sq_plan.h"

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

// ---- the PQ store (vstore_pq_plan.h) ------------------------------------------------------------------------------------------------------
struct PqBooks {
    const float *centroids;   // [kc][d]
    const float *codebooks;   // [m][ksub][dsub]
    const float *refine;      // [m2][k2][dsub2]
    int kc, d, m, ksub, dsub, m2, k2, dsub2;
    u32 stride;               // bytes of a record
};

struct RerankPqArgs {
    RerankArgs r;             // rows: the records
    PqBooks b;
};

// the four components from t0 on of the row whose record lies at `rec` (LDS), reconstructed: (centre + base codeword) + refinement codeword.
// j1 / a1, j2 / a2: sub-space and place in it of component t0 under the base and the refinement quantizer.  STAGED: the two codeword
// pieces are piece g of the chunk's slices in LDS (vstore_pq_plan.h), not reads of the codebooks.
template <bool VEC, bool STAGED>
__device__ __forceinline__ uint4 rerank_pq_piece(const PqBooks &b, bool ok, const uint8_t *rec, int t0, int j1, int a1, int j2, int a2,
                                                 const float *slices, int g)
{
    float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ok && t0 < b.d) {
        // (every record was written by vstore_pq_encode_kernel and names a list and two codewords; the bounds keep a damaged one inside the arrays)
        const u32 list = min(*(const u32 *)(rec + vspq::off_list()), (u32)b.kc - 1u);
        if constexpr (VEC) {
            const u32 c1 = min((u32)rec[vspq::off_code(j1)], (u32)b.ksub - 1u), c2 = min((u32)rec[vspq::off_code2(b.m, j2)], (u32)b.k2 - 1u);
            const float4 c = *(const float4 *)(b.centroids + vspq::centroid_elem(list, b.d, t0));
            float4 p, r;
            if constexpr (STAGED) {
                p = *(const float4 *)(slices + vspq::slice_piece(c1, g));
                r = *(const float4 *)(slices + vspq::slice_dwords(b.ksub) + vspq::slice_piece(c2, g));
            } else {
                p = *(const float4 *)(b.codebooks + vspq::codeword_elem(j1, c1, a1, b.dsub, b.ksub));
                r = *(const float4 *)(b.refine + vspq::codeword_elem(j2, c2, a2, b.dsub2, b.k2));
            }
            y[0] = (c.x + p.x) + r.x; y[1] = (c.y + p.y) + r.y; y[2] = (c.z + p.z) + r.z; y[3] = (c.w + p.w) + r.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = t0 + k;
                if (t >= b.d) break;
                const int s1 = vspq::sub_of(t, b.dsub), s2 = vspq::sub_of(t, b.dsub2);
                const u32 c1 = min((u32)rec[vspq::off_code(s1)], (u32)b.ksub - 1u), c2 = min((u32)rec[vspq::off_code2(b.m, s2)], (u32)b.k2 - 1u);
                y[k] = (b.centroids[vspq::centroid_elem(list, b.d, t)] + b.codebooks[vspq::codeword_elem(s1, c1, vspq::sub_at(t, b.dsub), b.dsub, b.ksub)])
                       + b.refine[vspq::codeword_elem(s2, c2, vspq::sub_at(t, b.dsub2), b.dsub2, b.k2)];
            }
        }
    }
    return make_uint4(__float_as_uint(y[0]), __float_as_uint(y[1]), __float_as_uint(y[2]), __float_as_uint(y[3]));
}

// the reconstruction of chunk c of the rows this lane serves (fok: the row's slot is live with an id below n)
template <bool VEC, bool STAGED>
__device__ __forceinline__ void rerank_pq_stage(const PqBooks &b, const bool *fok, const uint8_t *recs, const float *slices, int c, int lane, uint4 *st)
{
    const int t0 = vspq::chunk_comp(c, rerank::gather_dword(lane, 0));   // the same four components of every row this lane serves
    const int j1 = vspq::sub_of(t0, b.dsub), a1 = vspq::sub_at(t0, b.dsub), j2 = vspq::sub_of(t0, b.dsub2), a2 = vspq::sub_at(t0, b.dsub2);
#pragma unroll
    for (int i = 0; i < rerank::LOADS; ++i)
        st[i] = rerank_pq_piece<VEC, STAGED>(b, fok[i], recs + (size_t)rerank::gather_row(lane, i) * b.stride, t0, j1, a1, j2, a2, slices,
                                             rerank::gather_dword(lane, 0) / 4);
}

// the staged route: chunk c's slices of both codebooks into LDS, the workgroup's 256 lanes on consecutive pieces (a piece whose four
// components lie at or beyond d is not read and never used)
__device__ __forceinline__ void rerank_pq_fill_slices(const PqBooks &b, float *slices, int c, int tid)
{
    const u32 n1 = vspq::slice_pieces(b.ksub), n2 = vspq::slice_pieces(b.k2);
#pragma unroll 4
    for (u32 e = (u32)tid; e < n1 + n2; e += (u32)rerank::TILE) {
        const bool base = e < n1;
        const u32 f = base ? e : e - n1, code = vspq::slice_code(f);
        const int g = vspq::slice_g(f), t0 = vspq::chunk_comp(c, 4 * g), ds = base ? b.dsub : b.dsub2;
        if (t0 >= b.d) continue;
        const float *src = (base ? b.codebooks : b.refine) + vspq::codeword_elem(vspq::sub_of(t0, ds), code, vspq::sub_at(t0, ds), ds, base ? b.ksub : b.k2);
        *(float4 *)(slices + (base ? 0u : vspq::slice_dwords(b.ksub)) + vspq::slice_piece(code, g)) = *(const float4 *)src;
    }
}

// STAGED (with VEC only): every wave of a workgroup that holds a slot below the live count walks the chunks, because every chunk begins
// with the workgroup's copy of its slices between two barriers; the chunk is then reconstructed and consumed at once (the slices of chunk
// c + 1 are not there yet, so nothing is built ahead).
template <bool VEC, bool STAGED>
__global__ __launch_bounds__(rerank::TILE) void rerank_pq_dist_kernel(const RerankPqArgs pa)
{
    static_assert(VEC || !STAGED, "the staged route serves the 16-byte form only");
    extern __shared__ __align__(16) u32 rr_lds[];
    const RerankArgs &a = pa.r;
    const PqBooks &b = pa.b;
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
    const bool active = mask != 0ull;
    float s = 0.0f;
    if (STAGED ? rerank::tile_slot(blockIdx.x, 0) < live : active) {   // STAGED: uniform over the workgroup
        u32 *tile = rr_lds + rerank::tile_base(a.d, wv);
        uint8_t *recs = (uint8_t *)(rr_lds + vspq::record_base(a.d, wv, b.stride));
        float *slices = (float *)(rr_lds + vspq::slice_base(a.d, b.stride));
        // the wave's 64 records into LDS: piece i is bytes piece_byte(i) .. of row piece_row(i) (pieces: a multiple of 64, every lane takes every turn)
        const u32 np = vspq::pieces(b.stride);
        for (u32 i = (u32)lane; i < np; i += 64u) {
            const int r = vspq::piece_row(i, b.stride);
            const u32 at = vspq::piece_byte(i, b.stride);
            const u32 id = (u32)__shfl((int)v, r);
            if ((mask >> r) & 1ull) {
                const uint8_t *src = a.rows + vspq::record_offset(id, b.stride) + at;
                uint8_t *dst = recs + (size_t)r * b.stride + at;
                if (vspq::piece_bytes(b.stride) == 16u) *(uint4 *)dst = *(const uint4 *)src;
                else *(u32 *)dst = *(const u32 *)src;
            }
        }
        wave_sync();
        bool fok[rerank::LOADS];
#pragma unroll
        for (int i = 0; i < rerank::LOADS; ++i) fok[i] = (mask >> rerank::gather_row(lane, i)) & 1ull;
        const int nch = rerank::chunks(a.d, false);
        uint4 st[rerank::LOADS];
        if constexpr (!STAGED) rerank_pq_stage<VEC, false>(b, fok, recs, slices, 0, lane, st);
        for (int c = 0; c < nch; ++c) {
            if constexpr (STAGED) {
                __syncthreads();   // every wave has taken its pieces of chunk c - 1's slices
                rerank_pq_fill_slices(b, slices, c, tid);
                __syncthreads();
                if (!active) continue;
                rerank_pq_stage<VEC, true>(b, fok, recs, slices, c, lane, st);
            }
            // the staged chunk c into the tile (the reads of chunk c - 1 are behind the wave_sync that ended its turn)
#pragma unroll
            for (int i = 0; i < rerank::LOADS; ++i) {
                u32 *dst = tile + rerank::tile_index(rerank::gather_row(lane, i), rerank::gather_dword(lane, 0));
                dst[0] = st[i].x; dst[1] = st[i].y; dst[2] = st[i].z; dst[3] = st[i].w;
            }
            wave_sync();
            if constexpr (!STAGED)
                if (c + 1 < nch) rerank_pq_stage<VEC, false>(b, fok, recs, slices, c + 1, lane, st);
            s = rerank_consume<false>(s, tile + rerank::tile_index(lane, 0), qs + (size_t)c * rerank::CHUNK_DWORDS, rerank::chunk_len(a.d, false, c));
            wave_sync();
        }
    }
    if (j < a.C) a.keys[rerank::key_index(qy, a.C, j)] = ok ? (((u64)__float_as_uint(s) << 32) | (u32)j) : (u64)KEY_MAX;
}

struct PqEncodeArgs {
    PqBooks b;                // refine null: the residual pass of the trainer (no refinement code, no record)
    const float *pts;         // rows of this block, [rows][d]
    const int *assign;        // their nearest centre
    float *out_resid;         // null, or [rows][d]: the second residuals
    uint8_t *records;         // the record of the block's first row
};

// best[j] <- min over c < k of (chain bits << 32 | c): encode_kernel's chain, first minimum on ties.  best[] holds KEY_MAX; k <= 256.
__device__ __forceinline__ void vstore_pq_argmin(const float *__restrict__ books, const float *rr, int nsub, int k, int dsub, u64 *best, int tid)
{
    for (int e = tid; e < nsub * 256; e += 256) {
        const int ii = e >> 8, c = e & 255;
        u64 key = KEY_MAX;
        if (c < k) {
            const float *cw = books + vspq::codeword_elem(ii, (u32)c, 0, dsub, k);
            const float *x = rr + (size_t)ii * dsub;
            float sum = 0.0f;
            for (int t = 0; t < dsub; ++t) {
                const float df = cw[t] - x[t];
                sum = sum + df * df;
            }
            key = make_key(sum, (u32)c);
        }
        // wave min, then one LDS atomic per wave (ii is wave-uniform: 256 % 64 == 0)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const u64 o = __shfl_xor(key, off);
            key = o < key ? o : key;
        }
        if ((tid & 63) == 0) atomicMin(&best[ii], key);
    }
}

__global__ __launch_bounds__(256) void vstore_pq_encode_kernel(const PqEncodeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const PqBooks &b = a.b;
    float *resid = (float *)smem_raw;                                  // [d]: x - c, then e = x - (c + p)
    u64 *best1 = (u64 *)(resid + rerank::query_dwords(b.d));           // [m]
    u64 *best2 = best1 + b.m;                                          // [m2]
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    const int l = a.assign[p];
    const float *__restrict__ x = a.pts + (size_t)p * b.d;
    const float *__restrict__ centre = b.centroids + vspq::centroid_elem((u32)l, b.d, 0);
    for (int i = tid; i < b.d; i += 256) resid[i] = x[i] - centre[i];
    for (int i = tid; i < b.m + b.m2; i += 256) best1[i] = KEY_MAX;
    __syncthreads();
    vstore_pq_argmin(b.codebooks, resid, b.m, b.ksub, b.dsub, best1, tid);
    __syncthreads();
    for (int t = tid; t < b.d; t += 256) {
        const int j = vspq::sub_of(t, b.dsub);
        const float y1 = centre[t] + b.codebooks[vspq::codeword_elem(j, (u32)best1[j], vspq::sub_at(t, b.dsub), b.dsub, b.ksub)];
        const float e = x[t] - y1;
        resid[t] = e;
        if (a.out_resid) a.out_resid[(size_t)p * b.d + t] = e;
    }
    if (!b.refine) return;
    __syncthreads();
    vstore_pq_argmin(b.refine, resid, b.m2, b.k2, b.dsub2, best2, tid);
    __syncthreads();
    uint8_t *rec = a.records + vspq::record_offset((uint64_t)p, b.stride);
    for (u32 i = (u32)tid; i < b.stride; i += 256u) {
        uint8_t byte = 0u;
        if (i < (u32)vspq::LIST_BYTES) byte = (uint8_t)((u32)l >> (8u * i));
        else if (i < vspq::off_code2(b.m, 0)) byte = (uint8_t)(u32)best1[i - vspq::off_code(0)];
        else if (i < vspq::raw_bytes(b.m, b.m2)) byte = (uint8_t)(u32)best2[i - vspq::off_code2(b.m, 0)];
        rec[i] = byte;
    }
}

// *flag |= 1 when a component of src is not finite (the refusal of ivfadc_vectors_create_pq_device)
__global__ __launch_bounds__(256) void vstore_pq_finite_kernel(const float *__restrict__ src, uint64_t total, u32 *__restrict__ flag)
{
    bool bad = false;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256)
        bad |= (__float_as_uint(src[e]) & 0x7F800000u) == 0x7F800000u;
    if (bad) atomicOr(flag, 1u);
}

// ---- the 8-bit scalar-quantised store (vstore_sq_plan.h) ----------------------------------------------------------------------------------
struct SqRangeArgs {
    const float *src;         // rows of this block, [rows][d]
    int64_t rows;
    int d;
    u32 *img_min, *img_max;   // [d] each: vssq::image of the smallest and the largest component seen so far
    u32 *flag;                // |= 1: a component is not finite
};

__global__ __launch_bounds__(vssq::RANGE_LANES) void vstore_sq_range_kernel(const SqRangeArgs a)
{
    __shared__ u32 s_min[vssq::RANGE_LANES], s_max[vssq::RANGE_LANES];
    const int tid = threadIdx.x, cols = vssq::range_cols(a.d), par = vssq::range_rows_par(a.d);
    const int cx = tid % cols, ry = tid / cols;
    const int t = (int)blockIdx.x * cols + cx;
    const int64_t r0 = vssq::range_row_begin(a.rows, gridDim.y, blockIdx.y), r1 = vssq::range_row_begin(a.rows, gridDim.y, blockIdx.y + 1u);
    u32 lo = vssq::IMAGE_MIN_INIT, hi = vssq::IMAGE_MAX_INIT;
    bool bad = false;
    if (t < a.d) {
        const float *__restrict__ col = a.src + t;
#pragma unroll 4
        for (int64_t r = r0 + ry; r < r1; r += par) {
            const u32 bits = __float_as_uint(col[(uint64_t)r * (uint64_t)a.d]);
            const u32 img = vssq::image(bits);
            bad |= vssq::not_finite(bits);
            lo = min(lo, img);
            hi = max(hi, img);
        }
    }
    // the `par` lanes of a column meet in LDS: one atomic min and one atomic max per column and workgroup
    s_min[tid] = lo;
    s_max[tid] = hi;
    __syncthreads();
    if (ry == 0 && t < a.d) {
        for (int k = 1; k < par; ++k) {
            lo = min(lo, s_min[k * cols + cx]);
            hi = max(hi, s_max[k * cols + cx]);
        }
        if (lo <= hi) {   // (a workgroup without rows has seen nothing)
            atomicMin(a.img_min + t, lo);
            atomicMax(a.img_max + t, hi);
        }
    }
    if (bad) atomicOr(a.flag, 1u);
}

struct SqEncodeArgs {
    const float *src;         // rows of this block, [rows][d]
    int64_t rows;
    int d;
    bool vec;                 // vssq::encode_vec: a whole piece comes as four float4 loads
    const float *lo, *inv;    // [d] each
    uint8_t *dst;             // the block's first row in the store
    u32 *flag;                // |= 1: a component is not finite
};

// the four codes of components t .. t + 3 in one dword, component t in the low byte
__device__ __forceinline__ u32 vstore_sq_pack(float4 x, const float *lo, const float *inv, int t, bool &bad)
{
    bad |= vssq::not_finite(__float_as_uint(x.x)) | vssq::not_finite(__float_as_uint(x.y)) | vssq::not_finite(__float_as_uint(x.z)) |
           vssq::not_finite(__float_as_uint(x.w));
    return vssq::encode(x.x, lo[t], inv[t]) | vssq::encode(x.y, lo[t + 1], inv[t + 1]) << 8 | vssq::encode(x.z, lo[t + 2], inv[t + 2]) << 16 |
           vssq::encode(x.w, lo[t + 3], inv[t + 3]) << 24;
}

__global__ __launch_bounds__(vssq::ENCODE_LANES) void vstore_sq_encode_kernel(const SqEncodeArgs a)
{
    extern __shared__ __align__(16) float vsq_lds[];
    const int tid = threadIdx.x;
    const float *lo = a.lo, *inv = a.inv;
    if (vssq::encode_in_lds(a.d)) {
        float *l = vsq_lds, *v = vsq_lds + rerank::query_dwords(a.d);
        for (int t = tid; t < a.d; t += vssq::ENCODE_LANES) { l[t] = a.lo[t]; v[t] = a.inv[t]; }
        __syncthreads();
        lo = l;
        inv = v;
    }
    const u32 ppr = vssq::pieces_per_row(a.d);
    const uint64_t total = vssq::encode_pieces(a.rows, a.d);
    bool bad = false;
    for (uint64_t e = (uint64_t)blockIdx.x * vssq::ENCODE_LANES + tid; e < total; e += (uint64_t)gridDim.x * vssq::ENCODE_LANES) {
        const uint64_t r = vssq::piece_row(e, ppr);
        const int t0 = vssq::piece_comp(e, ppr);
        const float *__restrict__ x = a.src + r * (uint64_t)a.d + t0;
        u32 w[4] = {0u, 0u, 0u, 0u};
        if (a.vec && t0 + vssq::PIECE <= a.d) {
            const float4 x0 = ((const float4 *)x)[0], x1 = ((const float4 *)x)[1], x2 = ((const float4 *)x)[2], x3 = ((const float4 *)x)[3];
            w[0] = vstore_sq_pack(x0, lo, inv, t0, bad);
            w[1] = vstore_sq_pack(x1, lo, inv, t0 + 4, bad);
            w[2] = vstore_sq_pack(x2, lo, inv, t0 + 8, bad);
            w[3] = vstore_sq_pack(x3, lo, inv, t0 + 12, bad);
        } else {
            // the last piece of a row (its padding stays zero), and every piece of a source without 16-byte rows
#pragma unroll
            for (int k = 0; k < vssq::PIECE; ++k) {
                if (t0 + k < a.d) {
                    const float xv = x[k];
                    bad |= vssq::not_finite(__float_as_uint(xv));
                    w[k >> 2] |= vssq::encode(xv, lo[t0 + k], inv[t0 + k]) << vssq::comp_shift(k);
                }
            }
        }
        *(uint4 *)(a.dst + vssq::row_offset(r, vssq::stride(a.d)) + (uint64_t)t0) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (bad) atomicOr(a.flag, 1u);
}

struct RerankSqArgs {
    RerankArgs r;             // rows: the codes
    const float *lo, *step;   // [d] each
    u32 stride;               // bytes of a row
};

// the four components of dword x of a row, from component t on: decoded and taken into the chain.  qc, lo, st: the chunk's, in LDS.
__device__ __forceinline__ float rerank_sq_dword(float s, u32 x, const float *qc, const float *lo, const float *st, int t)
{
    const float4 q = *(const float4 *)(qc + t), l = *(const float4 *)(lo + t), p = *(const float4 *)(st + t);   // wave-uniform: broadcasts
    s = rerank_step(s, l.x + (float)(x & 0xFFu) * p.x, q.x);
    s = rerank_step(s, l.y + (float)((x >> 8) & 0xFFu) * p.y, q.y);
    s = rerank_step(s, l.z + (float)((x >> 16) & 0xFFu) * p.z, q.z);
    s = rerank_step(s, l.w + (float)(x >> 24) * p.w, q.w);
    return s;
}

__global__ __launch_bounds__(rerank::TILE) void rerank_sq_dist_kernel(const RerankSqArgs sa)
{
    extern __shared__ __align__(16) u32 rr_lds[];
    const RerankArgs &a = sa.r;
    float *qs = (float *)rr_lds, *los = qs + vssq::lo_base(a.d), *steps = qs + vssq::step_base(a.d);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t qy = blockIdx.y, q = a.q0 + qy;
    const float *__restrict__ qrow = a.queries + rerank::query_row(q, a.d);
    for (int t = tid; t < a.d; t += rerank::TILE) { qs[t] = qrow[t]; los[t] = sa.lo[t]; steps[t] = sa.step[t]; }
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
        u32 *tile = rr_lds + vssq::tile_base(a.d, wv);
        // this lane's 16 bytes of the line of row gather_row(lane, i): null where the slot is dead or the line ends before them
        const uint8_t *frow[rerank::LOADS];
        const u32 at = (u32)rerank::gather_dword(lane, 0) * 4u;
#pragma unroll
        for (int i = 0; i < rerank::LOADS; ++i) {
            const int r = rerank::gather_row(lane, i);
            const u32 id = (u32)__shfl((int)v, r);
            frow[i] = (mask >> r) & 1ull ? a.rows + vssq::row_offset(id, sa.stride) + at : nullptr;
        }
        const int nch = vssq::chunks(a.d);
        auto fetch = [&](int i, int c) -> uint4 {
            const uint64_t b = rerank::chunk_byte(c, 0);
            return frow[i] && b + at < sa.stride ? *(const uint4 *)(frow[i] + b) : make_uint4(0u, 0u, 0u, 0u);
        };
        uint4 st[rerank::LOADS];
#pragma unroll
        for (int i = 0; i < rerank::LOADS; ++i) st[i] = fetch(i, 0);
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
                for (int i = 0; i < rerank::LOADS; ++i) st[i] = fetch(i, c + 1);
            }
            const u32 *row = tile + rerank::tile_index(lane, 0);
            const int t0 = c * vssq::CHUNK_ELEMS, len = vssq::chunk_len(a.d, c);
            if (len == vssq::CHUNK_ELEMS) {
#pragma unroll
                for (int w = 0; w < rerank::CHUNK_DWORDS; ++w) s = rerank_sq_dword(s, row[w], qs + t0, los + t0, steps + t0, 4 * w);
            } else {
                int t = 0;
                for (; t + 4 <= len; t += 4) s = rerank_sq_dword(s, row[vssq::comp_dword(t)], qs + t0, los + t0, steps + t0, t);
                for (; t < len; ++t) {
                    const u32 code = (row[vssq::comp_dword(t)] >> vssq::comp_shift(t)) & 0xFFu;
                    s = rerank_step(s, vssq::decode(code, los[t0 + t], steps[t0 + t]), qs[t0 + t]);
                }
            }
            wave_sync();
        }
    }
    if (j < a.C) a.keys[rerank::key_index(qy, a.C, j)] = ok ? (((u64)__float_as_uint(s) << 32) | (u32)j) : (u64)KEY_MAX;
}

}  // namespace ivf
