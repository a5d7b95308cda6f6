// score.hip.h -- "what distance would knn_search report between this query and this stored id" (ivfadc_score_ids): the exact ADC
// distance of (query, candidate id) pairs with no scan of the lists.  gfx950, wave64.  Plan, pair arithmetic and tile shape: score_plan.h.
// The ids are located first by the pass of reconstruct.hip.h (last list, first position: utils.jl:49-55), which leaves (list, position)
// per located slot; the kernel below evaluates the pairs.
//
//   score_pairs_kernel   one workgroup = one query and score::TILE consecutive slots of it; the query sits in LDS (d floats, dynamic).
//                        ONE LANE OWNS ONE PAIR and runs the reference's three chains itself, in Float32, one rounding per operation (the
//                        build's -ffp-contract=off covers this file: no product is fused into a sum):
//                          dc      = 0; t ascending: u = C_l[t] - q[t]; dc = dc + u * u          coarsequantizers.jl:33-34
//                          r[t]    = q[t] - C_l[t]                                               coarsequantizers.jl:40-45
//                          s_ii    = 0; t of sub-space ii ascending: u = CB_ii[c_ii][t] - r[t]; s_ii = s_ii + u * u      index.jl:232-236
//                          dist    = dc; ii ascending: dist = dist + s_ii                        index.jl:242-246
//                        The chains are sequential by definition, so the parallelism is across pairs, not inside a sum.  Pass 1 streams
//                        the centre row for dc; pass 2 streams it again (an L1 / L2 hit), forms r[t] on the fly, finishes each s_ii as
//                        its sub-space ends and adds it to dist at once.  m and dsub are run-time values and no per-lane array exists,
//                        so there is no scratch.  Rows are read 16 bytes at a time where their offsets allow (score::centre_vec4,
//                        score::codeword_vec4), else one float at a time (d = 10: 40-byte rows).  The stored code is read as
//                        recon_decode_kernel reads it: an 8-bit code is a LABEL and goes through the inverse labels, a 16-bit code is
//                        the little-endian codeword index, both clamped to ksub - 1.  Written once for both code widths.
//                        A dead slot (at or behind counts[q]) and an absent id write +Inf / 0 and read nothing of the index.
// Plain C++ and vector loads and stores only.
#pragma once

#include <hip/hip_runtime.h>

#include "reconstruct.hip.h"
#include "score_plan.h"

namespace ivf {

// the codeword the stored code of sub-space ii names (recon_decode_kernel's rule)
__device__ __forceinline__ uint32_t score_codeword(const DecodeArgs &a, const uint8_t *__restrict__ row, uint32_t ii)
{
    uint32_t c;
    if (a.label_inv) c = a.label_inv[recon::label_slot(ii, row[ii])];
    else c = (uint32_t)row[2 * ii] | ((uint32_t)row[2 * ii + 1] << 8);
    return c < (uint32_t)a.ksub ? c : (uint32_t)a.ksub - 1u;
}

// one step of a chain: u = x - y; acc = acc + u * u
__device__ __forceinline__ float score_step(float acc, float x, float y)
{
    const float u = x - y;
    return acc + u * u;
}

// the distance of the query in qs (LDS) to the entry at position p of list l; l in [0, kc), p below the list's length
__device__ __forceinline__ float score_pair(const DecodeArgs &a, const float *__restrict__ qs, int32_t l, int64_t p)
{
    const float *__restrict__ centre = a.centroids + (size_t)l * a.d;
    const uint8_t *__restrict__ row = a.codes + recon::code_row((uint64_t)a.list_codeoff[l], (uint64_t)p, (uint32_t)a.cs);
    float dc = 0.0f;
    if (score::centre_vec4(a.d)) {
        for (int t = 0; t < a.d; t += 4) {
            const float4 c4 = *(const float4 *)(centre + t);
            const float4 q4 = *(const float4 *)(qs + t);
            dc = score_step(dc, c4.x, q4.x);
            dc = score_step(dc, c4.y, q4.y);
            dc = score_step(dc, c4.z, q4.z);
            dc = score_step(dc, c4.w, q4.w);
        }
    } else {
        for (int t = 0; t < a.d; ++t) dc = score_step(dc, centre[t], qs[t]);
    }
    float dist = dc;
    if (score::codeword_vec4(a.dsub)) {
        for (uint32_t ii = 0; ii < (uint32_t)a.m; ++ii) {
            const uint32_t c = score_codeword(a, row, ii);
            const uint32_t t0 = ii * (uint32_t)a.dsub;
            const float *__restrict__ cw = a.codebooks + recon::codeword_elem(ii, c, t0, (uint32_t)a.dsub, (uint32_t)a.ksub);
            float s = 0.0f;
            for (int k = 0; k < a.dsub; k += 4) {
                const float4 w4 = *(const float4 *)(cw + k);
                const float4 c4 = *(const float4 *)(centre + t0 + k);
                const float4 q4 = *(const float4 *)(qs + t0 + k);
                s = score_step(s, w4.x, q4.x - c4.x);
                s = score_step(s, w4.y, q4.y - c4.y);
                s = score_step(s, w4.z, q4.z - c4.z);
                s = score_step(s, w4.w, q4.w - c4.w);
            }
            dist = dist + s;
        }
    } else {
        for (uint32_t ii = 0; ii < (uint32_t)a.m; ++ii) {
            const uint32_t c = score_codeword(a, row, ii);
            const uint32_t t0 = ii * (uint32_t)a.dsub;
            const float *__restrict__ cw = a.codebooks + recon::codeword_elem(ii, c, t0, (uint32_t)a.dsub, (uint32_t)a.ksub);
            float s = 0.0f;
            for (int k = 0; k < a.dsub; ++k) s = score_step(s, cw[k], qs[t0 + k] - centre[t0 + k]);
            dist = dist + s;
        }
    }
    return dist;
}

// queries: d x (all queries of the call); q0: first query of this slice (blockIdx.y counts from it); counts: null = every slot is live;
// loc_list / loc_pos: what recon_resolve_kernel wrote, at score::loc_index; out_dists / out_found: nq x C (out_found may be null)
__global__ __launch_bounds__(score::TILE) void score_pairs_kernel(const DecodeArgs a, int kc, const float *__restrict__ queries, int64_t q0,
                                                                  int64_t C, bool shared, const int32_t *__restrict__ counts,
                                                                  const int32_t *__restrict__ loc_list, const int64_t *__restrict__ loc_pos,
                                                                  float *__restrict__ out_dists, uint8_t *__restrict__ out_found)
{
    extern __shared__ __align__(16) float score_qs[];
    const int64_t qy = blockIdx.y, q = q0 + qy;
    const float *__restrict__ qrow = queries + score::query_row(q, a.d);
    for (int t = threadIdx.x; t < a.d; t += score::TILE) score_qs[t] = qrow[t];
    __syncthreads();
    const int64_t j = score::tile_slot(blockIdx.x, threadIdx.x);
    if (j >= C) return;
    float dist = __builtin_huge_valf();
    uint8_t found = 0;
    if (j < score::live_slots(counts != nullptr, counts ? counts[q] : 0, C)) {
        const uint64_t li = score::loc_index(shared, qy, C, j);
        const int32_t l = loc_list[li];
        const int64_t p = loc_pos[li];
        if (l >= 0 && l < kc && p >= 0) {
            dist = score_pair(a, score_qs, l, p);
            found = 1;
        }
    }
    const uint64_t pair = score::pair_index(q, C, j);
    out_dists[pair] = dist;
    if (out_found) out_found[pair] = found;
}

}  // namespace ivf
