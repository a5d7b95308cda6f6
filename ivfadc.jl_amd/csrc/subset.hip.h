// subset.hip.h -- device-built subset views (ivfadc_clone_subset): a stable stream compaction of the inverted lists by a bitmap over the
// stored ids, out of place, into the Lists group a subset view owns.  gfx950, wave64.
//
// Stands for deleteat!(list.idxs, ...) / deleteat!(list.codes, ...) of utils.jl:98-99 applied to every entry that is NOT selected, WITHOUT
// the _shift_inverse_index! that follows it there: the kept entries stay in their stored order and keep their stored ids.
//
// A work item is (list, chunk of SUBSET_CHUNK points) (subset_plan.h: the host builds the items from the list lengths it owns).  One
// workgroup of 256 per item; wave v takes the item's points [v * SUBSET_WAVE_POINTS, (v + 1) * SUBSET_WAVE_POINTS) in SUBSET_ROUNDS rounds
// of 64 consecutive points, so a wave's kept entries are consecutive in the output and ONE total per wave is all the workgroup shares:
//   subset_count_kernel    ids -> keep bit -> __ballot / __popcll -> one u32 per item.
//   (host)                 per-list totals, per-item exclusive bases, the new layout (subset_plan.h, layout_from_caps)
//   subset_scatter_kernel  recomputes the keep bits (no stored mask to go stale) and writes id and code row of every kept point to
//                          item base + kept points of the waves before + kept points of the rounds before + __popcll(mask & lanes below).
// No atomics (the order comes from the prefix), no scratch, 16 bytes of LDS (the four wave totals).  List offsets and code byte offsets
// are 64-bit, positions within a list 32-bit.  Bytes moved by one creation, n points of which `kept` are selected, cs bytes per code row:
//     4n  (count: the ids)  +  n (4 + cs)  (scatter: the ids again, the code rows)  +  kept (4 + cs)  (scatter: what it writes)
// plus the bitmap words the ids name.  The figure is an upper bound: the code row of a dropped point is not read as such (its cache
// line is, wherever a neighbour is kept), and device-synthesised lists have no id array to read (the id is the position).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "subset_plan.h"

namespace ivf {

// the keep bits of one wave's share of an item: mask[r] = ballot of round r, id[r] = this lane's id in round r; returns the wave's total
static __device__ __forceinline__ uint32_t subset_wave_masks(const subset::Item it, int wv, int lane, uint32_t len, int64_t lpos,
                                                             const uint32_t *__restrict__ ids, const uint32_t *__restrict__ bits,
                                                             uint64_t nbits, unsigned long long (&mask)[subset::SUBSET_ROUNDS],
                                                             uint32_t (&id)[subset::SUBSET_ROUNDS])
{
    uint32_t total = 0;
#pragma unroll
    for (int r = 0; r < subset::SUBSET_ROUNDS; ++r) {
        const int64_t p = subset::subset_point(it.chunk, wv, r, lane);
        bool keep = false;
        id[r] = 0;
        if (p < (int64_t)len) {
            id[r] = ids ? ids[lpos + p] : (uint32_t)(lpos + p);   // (synthetic lists: the id is the global position)
            keep = subset::subset_selected(bits, nbits, id[r]);
        }
        mask[r] = __ballot(keep);
        total += (uint32_t)__popcll(mask[r]);
    }
    return total;
}

__global__ __launch_bounds__(256) void subset_count_kernel(const subset::Item *__restrict__ items, const int64_t *__restrict__ list_pos,
                                                           const uint32_t *__restrict__ list_len, const uint32_t *__restrict__ ids,
                                                           const uint32_t *__restrict__ bits, uint64_t nbits,
                                                           uint32_t *__restrict__ item_count)
{
    __shared__ uint32_t s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const subset::Item it = items[blockIdx.x];
    unsigned long long mask[subset::SUBSET_ROUNDS];
    uint32_t id[subset::SUBSET_ROUNDS];
    const uint32_t total = subset_wave_masks(it, wv, lane, list_len[it.list], list_pos[it.list], ids, bits, nbits, mask, id);
    if (lane == 0) s_wave[wv] = total;
    __syncthreads();
    if (tid == 0) item_count[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// one code row of nw dwords; rows start at multiples of 4 nw bytes inside 256-byte aligned blocks, so the wider forms are aligned
static __device__ __forceinline__ void subset_copy_row(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int nw)
{
    if ((nw & 3) == 0) {
        for (int i = 0; i < nw; i += 4) *(uint4 *)(dst + i) = *(const uint4 *)(src + i);
    } else if ((nw & 1) == 0) {
        for (int i = 0; i < nw; i += 2) *(uint2 *)(dst + i) = *(const uint2 *)(src + i);
    } else {
        for (int i = 0; i < nw; ++i) dst[i] = src[i];
    }
}

// src_*: the index's lists; dst_*: the subset view's (new buffers: nothing read here is written here).  nw = cs / 4 dwords per code row.
__global__ __launch_bounds__(256) void subset_scatter_kernel(const subset::Item *__restrict__ items, const int64_t *__restrict__ src_pos,
                                                             const uint32_t *__restrict__ src_len, const int64_t *__restrict__ src_codeoff,
                                                             const uint32_t *__restrict__ src_ids, const uint8_t *__restrict__ src_codes,
                                                             const uint32_t *__restrict__ bits, uint64_t nbits,
                                                             const uint32_t *__restrict__ item_base, const int64_t *__restrict__ dst_pos,
                                                             const int64_t *__restrict__ dst_codeoff, uint32_t *__restrict__ dst_ids,
                                                             uint8_t *__restrict__ dst_codes, int nw)
{
    __shared__ uint32_t s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const subset::Item it = items[blockIdx.x];
    unsigned long long mask[subset::SUBSET_ROUNDS];
    uint32_t id[subset::SUBSET_ROUNDS];
    const uint32_t total = subset_wave_masks(it, wv, lane, src_len[it.list], src_pos[it.list], src_ids, bits, nbits, mask, id);
    if (lane == 0) s_wave[wv] = total;
    __syncthreads();
    uint32_t run = item_base[blockIdx.x];
    for (int v = 0; v < wv; ++v) run += s_wave[v];
    const uint32_t *srow = (const uint32_t *)(src_codes + src_codeoff[it.list]);
    uint32_t *drow = (uint32_t *)(dst_codes + dst_codeoff[it.list]);
    uint32_t *did = dst_ids + dst_pos[it.list];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < subset::SUBSET_ROUNDS; ++r) {
        if ((mask[r] >> lane) & 1ull) {
            const int64_t p = subset::subset_point(it.chunk, wv, r, lane);
            const uint32_t dst = run + (uint32_t)__popcll(mask[r] & below);
            did[dst] = id[r];
            subset_copy_row(srow + (size_t)p * nw, drow + (size_t)dst * nw, nw);
        }
        run += (uint32_t)__popcll(mask[r]);
    }
}

}  // namespace ivf
