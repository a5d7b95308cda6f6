// reconstruct.hip.h -- "what is stored under this id" (ivfadc_locate, ivfadc_reconstruct): the reference's _pop! loop (utils.jl:49-55)
// and _get_quantizer_vector + _decode_point (utils.jl:58-59, 71-81) for a batch of ids, on the device copy of the lists.  gfx950, wave64.
// Plan, index arithmetic and the rule of a hit: reconstruct_plan.h.
//
//   recon_chunk_prefix_kernel  list_len -> the exclusive prefix of the lists' chunk counts, by ONE workgroup, on the stream: no entry uploads
//                             anything about the lists, so the device entries only enqueue
//   recon_bitmap_zero_kernel  (device entries) zeroes the words of the wanted ids' span, read from the sorted ids themselves
//   recon_bitmap_fill_kernel  the wanted ids -> one bit each in the exact bitmap over their span (vector atomic OR)
//   recon_locate_kernel<HASH> one pass over the stored ids, the scan shape of maskset_build_kernel: a work item is (list, chunk of
//                             SUBSET_CHUNK points), a lane reads the ids of its four rounds first (nothing at or behind list_len: spare
//                             capacity holds stale rows after a delete), then puts each to the prefilter -- HASH: the workgroup's LDS filter,
//                             filled once per workgroup from the wanted ids; otherwise the exact bitmap -- and only what passes
//                             is searched for among the wanted ids.  A hit is ONE 64-bit vector atomic maximum of
//                             recon::hit_key(list, pos) in its slot: last list, first position, whatever the work split.
//                             Workgroups stride over the work items (the grid is capped, reconstruct_plan.h).
//   recon_resolve_kernel      request order: slot of every requested id (repeats find the same slot) -> list, position, found
//   recon_decode_kernel       one workgroup per request: the lanes run along d (coalesced stores), each gathers the code of its
//                             sub-space from the cs-strided row -- an 8-bit handle's byte is a LABEL and goes through the inverse labels
//                             (pack::label_inverse), a 16-bit handle's code is the codeword index -- and writes centre + codeword, ONE
//                             Float32 addition per component (no product next to it: nothing to contract).  Any dsub, any d.  An absent id: +0.0.
// Plain C++ and vector loads, stores and atomics only.
#pragma once

#include <hip/hip_runtime.h>

#include "reconstruct_plan.h"
#include "subset_plan.h"

namespace ivf {

__global__ __launch_bounds__(256) void recon_chunk_prefix_kernel(const uint32_t *__restrict__ list_len, uint32_t nlists, uint64_t *__restrict__ chunk_off)
{
    __shared__ uint64_t part[256];
    const uint32_t t = threadIdx.x;
    const uint32_t b = recon::prefix_begin(nlists, 256, t), e = recon::prefix_begin(nlists, 256, t + 1);
    uint64_t sum = 0;
    for (uint32_t l = b; l < e; ++l) sum += recon::list_chunks(list_len[l]);
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        uint64_t run = 0;
        for (int i = 0; i < 256; ++i) {
            const uint64_t v = part[i];
            part[i] = run;
            run += v;
        }
        chunk_off[nlists] = run;
    }
    __syncthreads();
    uint64_t run = part[t];
    for (uint32_t l = b; l < e; ++l) {
        chunk_off[l] = run;
        run += recon::list_chunks(list_len[l]);
    }
}

// from_want: the span is that of the nwant sorted wanted ids (recon::span_of), not (lo, nbits)
__global__ __launch_bounds__(256) void recon_bitmap_zero_kernel(const uint32_t *__restrict__ want, uint64_t nwant, uint32_t *__restrict__ bitmap)
{
    uint32_t lo;
    uint64_t nbits;
    recon::span_of(want, nwant, lo, nbits);
    const uint64_t words = recon::bitmap_words(nbits);
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (uint64_t)gridDim.x * 256) bitmap[i] = 0u;
}

__global__ __launch_bounds__(256) void recon_bitmap_fill_kernel(const uint32_t *__restrict__ want, uint64_t nwant, uint32_t lo, uint64_t nbits,
                                                                bool from_want, uint32_t *__restrict__ bitmap)
{
    if (from_want) recon::span_of(want, nwant, lo, nbits);
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nwant; i += (uint64_t)gridDim.x * 256) {
        const uint32_t id = want[i];
        if (recon::bitmap_covers(lo, nbits, id)) atomicOr(bitmap + recon::bitmap_word(lo, id), 1u << recon::bitmap_bit(lo, id));
    }
}

// want: the nwant sorted wanted ids; best: one key per wanted slot, 0 = nothing yet
template <bool HASH>
__global__ __launch_bounds__(256) void recon_locate_kernel(const uint64_t *__restrict__ chunk_off, uint32_t nlists, uint64_t items,
                                                           const int64_t *__restrict__ list_pos, const uint32_t *__restrict__ list_len,
                                                           const uint32_t *__restrict__ ids, const uint32_t *__restrict__ want, uint64_t nwant,
                                                           uint32_t lo, uint64_t nbits, bool from_want, const uint32_t *__restrict__ bitmap,
                                                           unsigned long long *__restrict__ best)
{
    __shared__ uint32_t filt[HASH ? recon::FILTER_WORDS : 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (HASH) {
        for (uint32_t i = tid; i < recon::FILTER_WORDS; i += 256) filt[i] = 0u;
        __syncthreads();
        for (uint64_t i = tid; i < nwant; i += 256) {
            const uint32_t hsh = recon::filter_hash(want[i]);
            atomicOr(&filt[recon::filter_word(hsh)], 1u << recon::filter_bit(hsh));
        }
        __syncthreads();
    } else if (from_want) {
        recon::span_of(want, nwant, lo, nbits);
    }
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t l = recon::item_list(chunk_off, nlists, item);
        const uint32_t chunk = (uint32_t)(item - chunk_off[l]);
        const uint32_t len = list_len[l];
        const int64_t lpos = list_pos[l];
        uint32_t id[subset::SUBSET_ROUNDS];
#pragma unroll
        for (int r = 0; r < subset::SUBSET_ROUNDS; ++r) {
            const int64_t p = subset::subset_point(chunk, wv, r, lane);
            id[r] = 0;
            if (p < (int64_t)len) id[r] = ids ? ids[lpos + p] : (uint32_t)(lpos + p);   // (synthetic lists: the id emit_result returns)
        }
#pragma unroll
        for (int r = 0; r < subset::SUBSET_ROUNDS; ++r) {
            const int64_t p = subset::subset_point(chunk, wv, r, lane);
            if (p >= (int64_t)len) continue;
            bool maybe;
            if (HASH) {
                const uint32_t hsh = recon::filter_hash(id[r]);
                maybe = ((filt[recon::filter_word(hsh)] >> recon::filter_bit(hsh)) & 1u) != 0u;
            } else {
                maybe = recon::bitmap_covers(lo, nbits, id[r]) &&
                        ((bitmap[recon::bitmap_word(lo, id[r])] >> recon::bitmap_bit(lo, id[r])) & 1u) != 0u;
            }
            if (!maybe) continue;
            const int64_t slot = recon::slot_of(want, 0, nwant, id[r]);
            if (slot >= 0) atomicMax(best + slot, (unsigned long long)recon::hit_key(l, (uint32_t)p));
        }
    }
}

// out_list / out_pos / out_found: any may be null
__global__ __launch_bounds__(256) void recon_resolve_kernel(const uint32_t *__restrict__ req, int64_t n, const uint32_t *__restrict__ want,
                                                            uint64_t nwant, const unsigned long long *__restrict__ best,
                                                            int32_t *__restrict__ out_list, int64_t *__restrict__ out_pos,
                                                            uint8_t *__restrict__ out_found)
{
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        const int64_t slot = recon::slot_of(want, 0, nwant, req[j]);
        const uint64_t key = slot >= 0 ? (uint64_t)best[slot] : 0ull;
        if (out_list) out_list[j] = recon::key_list(key);
        if (out_pos) out_pos[j] = recon::key_pos(key);
        if (out_found) out_found[j] = recon::key_found(key) ? 1 : 0;
    }
}

// what the decode reads of the index
struct DecodeArgs {
    const float *centroids;        // [kc][d]
    const float *codebooks;        // [m][ksub][dsub]
    const uint8_t *label_inv;      // [m][256] (8-bit handles), null on a 16-bit handle
    const uint8_t *codes;
    const int64_t *list_codeoff;   // [kc]
    int d, m, dsub, ksub, cs;
};

// loc_list / loc_pos: what recon_resolve_kernel wrote for the n requests; out: d x n
__global__ __launch_bounds__(256) void recon_decode_kernel(const DecodeArgs a, int64_t n, const int32_t *__restrict__ loc_list,
                                                           const int64_t *__restrict__ loc_pos, float *__restrict__ out)
{
    for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
        const int32_t l = loc_list[j];
        const int64_t p = loc_pos[j];
        float *dst = out + (size_t)j * a.d;
        if (l < 0 || p < 0) {
            for (int t = threadIdx.x; t < a.d; t += 256) dst[t] = 0.0f;
            continue;
        }
        const uint8_t *row = a.codes + recon::code_row((uint64_t)a.list_codeoff[l], (uint64_t)p, (uint32_t)a.cs);
        const float *centre = a.centroids + (size_t)l * a.d;
        for (int t = threadIdx.x; t < a.d; t += 256) {
            const uint32_t ii = recon::decode_block((uint32_t)t, (uint32_t)a.dsub);
            uint32_t c;
            if (a.label_inv) c = a.label_inv[recon::label_slot(ii, row[ii])];
            else c = (uint32_t)row[2 * ii] | ((uint32_t)row[2 * ii + 1] << 8);
            c = c < (uint32_t)a.ksub ? c : (uint32_t)a.ksub - 1u;   // (every stored code names a codeword: set_lists and the encoder see to it)
            dst[t] = centre[t] + a.codebooks[recon::codeword_elem(ii, c, (uint32_t)t, (uint32_t)a.dsub, (uint32_t)a.ksub)];
        }
    }
}

}  // namespace ivf
