// Planner and index arithmetic of ivfadc_locate / ivfadc_reconstruct (reconstruct.hip.h holds the kernels).  Plain C++ (no HIP types), in
// the manner of range_plan.h and maskset_plan.h, so that the plan and every index the kernels form compile and run without a GPU
// (tests/c/reconstruct_plan_check.cpp).
//
// LOCATE is one pass over the stored ids of every list.  The lists are cut into the work items of subset_plan.h (list, chunk of
// SUBSET_CHUNK points; a lane reads position subset_point(chunk, wave, round, lane) and nothing at or behind list_len); item i is found
// from chunk_off, the exclusive prefix of the lists' chunk counts, so the item list is never materialised (kc + 1 numbers instead of one
// per 1024 points).  The WANTED ids are sorted ascending as unsigned numbers (the host entry also removes repeats; the device entry keeps
// them, which changes nothing: a hit always lands in the FIRST slot that holds its id, the slot a request finds again).  A stored id is
// first put to a PREFILTER, and only what passes is searched for among the wanted ids:
//   BITMAP  one bit per id of the span [lo, hi] of the wanted ids, in device memory: exact, whatever the number of wanted ids.  The host
//           entries know the span.  The device entries do not (that would take a synchronisation): the buffer is sized for the whole id
//           space, 2^32 bits = 512 MB, and the kernels read the span from the sorted wanted ids themselves (span_of), so that only the
//           words of the real span are zeroed and read;
//   HASH    a hashed bit filter in LDS, FILTER_BITS bits per workgroup, filled by every workgroup from the wanted ids: no device memory,
//           but at most FILTER_MAX_WANTED wanted ids (the filter fills up) and two workgroups per compute unit.
// Either way the stored ids stream ONCE.  The bitmap is taken while its span stays within BITMAP_MAX_BITS, and beyond that as soon as the
// wanted ids exceed the LDS filter's cap; the LDS filter is left with few wanted ids of a wide or unknown span.
// A hit resolves with ONE 64-bit atomic maximum on key(list, pos) = list << 32 | ~pos in the slot of its id: the largest list wins and,
// within it, the smallest position -- the reference's loop (utils.jl:49-55: no break, so later lists overwrite; findfirst within a list)
// -- whatever the order in which workgroups and waves arrive.  A slot nothing hit keeps 0, which no entry produces.
//
// Measured: profiles/reconstruct_probe.txt, quoted in DESIGN.md 4.6.6.  The constants below are REASONED, NOT MEASURED: the probe has not
// varied them.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "subset_plan.h"

#if defined(__HIPCC__)
#define RECON_HD __host__ __device__ __forceinline__
#else
#define RECON_HD inline
#endif

namespace recon {

// ---- the hashed LDS filter ---------------------------------------------------------------------------------------------------------
// 64 KB of LDS per workgroup of four waves: two workgroups per compute unit (160 KB), eight waves streaming ids.  (the size: REASONED)
constexpr int FILTER_LOG2_BITS = 19;
constexpr uint32_t FILTER_BITS = 1u << FILTER_LOG2_BITS;
constexpr uint32_t FILTER_WORDS = FILTER_BITS / 32;
// the cap on wanted ids behind the LDS filter: it is then at most 1 / 32 full, so about 3 % of the stored ids that are NOT wanted pay a
// binary search of 14 steps in an array that stays in cache; the other 97 % cost their 4 bytes and one LDS read.  (REASONED)
constexpr uint32_t FILTER_MAX_WANTED = FILTER_BITS / 32;
// the span of the wanted ids up to which the exact bitmap is used whatever their number: 2^30 bits = 128 MB, half of the chip's 256 MB
// last-level cache, so the bits the stored ids ask for in no particular order are served from cache.  (REASONED)
constexpr uint64_t BITMAP_MAX_BITS = (uint64_t)1 << 30;
// the whole id space: the span of wanted ids the host has not seen
constexpr uint64_t ID_SPACE_BITS = (uint64_t)1 << 32;
// workgroups of the locate pass: a memory-bound pass is capped at eight workgroups per compute unit and strides over the rest
constexpr uint32_t GRID_WG_PER_CU_BITMAP = 8, GRID_WG_PER_CU_HASH = 2;

// multiplicative hash of an id into the filter (the top bits of id * odd constant)
RECON_HD uint32_t filter_hash(uint32_t id) { return (id * 0x9E3779B1u) >> (32 - FILTER_LOG2_BITS); }
RECON_HD uint32_t filter_word(uint32_t hash) { return hash >> 5; }
RECON_HD uint32_t filter_bit(uint32_t hash) { return hash & 31u; }

// ---- the exact bitmap over [lo, lo + nbits) ----------------------------------------------------------------------------------------
RECON_HD bool bitmap_covers(uint32_t lo, uint64_t nbits, uint32_t id) { return id >= lo && (uint64_t)(id - lo) < nbits; }
RECON_HD uint64_t bitmap_word(uint32_t lo, uint32_t id) { return (uint64_t)(id - lo) >> 5; }
RECON_HD uint32_t bitmap_bit(uint32_t lo, uint32_t id) { return (id - lo) & 31u; }
RECON_HD uint64_t bitmap_words(uint64_t nbits) { return (nbits + 31) / 32; }
// the span of nwant > 0 ascending wanted ids, as the kernels of a device entry read it
RECON_HD void span_of(const uint32_t *want, uint64_t nwant, uint32_t &lo, uint64_t &nbits)
{
    lo = want[0];
    nbits = (uint64_t)want[nwant - 1] - (uint64_t)lo + 1;
}

// ---- the key of a hit ----------------------------------------------------------------------------------------------------------------
// larger list first, then smaller position; never 0 (pos < 2^32 - 1: a list holds fewer than 2^32 points)
RECON_HD uint64_t hit_key(uint32_t list, uint32_t pos) { return ((uint64_t)list << 32) | (uint64_t)(uint32_t)~pos; }
RECON_HD bool key_found(uint64_t key) { return key != 0; }
RECON_HD int32_t key_list(uint64_t key) { return key ? (int32_t)(key >> 32) : -1; }
RECON_HD int64_t key_pos(uint64_t key) { return key ? (int64_t)(uint32_t)~(uint32_t)key : -1; }

// first index in [a, b) of the ascending (unsigned) array whose value is >= id; b if there is none
RECON_HD uint64_t lower_bound_u32(const uint32_t *v, uint64_t a, uint64_t b, uint32_t id)
{
    while (a < b) {
        const uint64_t mid = a + ((b - a) >> 1);
        if (v[mid] < id) a = mid + 1; else b = mid;
    }
    return a;
}

// the slot of id among the wanted ids [a, b): the first one that holds it, or -1
RECON_HD int64_t slot_of(const uint32_t *want, uint64_t a, uint64_t b, uint32_t id)
{
    const uint64_t s = lower_bound_u32(want, a, b, id);
    return (s < b && want[s] == id) ? (int64_t)s : (int64_t)-1;
}

// ---- work items --------------------------------------------------------------------------------------------------------------------
// chunks of a list of len points
RECON_HD uint64_t list_chunks(uint64_t len) { return (len + (uint64_t)subset::SUBSET_CHUNK - 1) / (uint64_t)subset::SUBSET_CHUNK; }

// chunk_off is built ON THE DEVICE from list_len by one workgroup (recon_chunk_prefix_kernel), so that no entry uploads it: thread t of
// nthreads sums the chunk counts of lists [prefix_begin(t), prefix_begin(t + 1)), the threads' sums are scanned, every thread writes its
// lists' exclusive prefixes
RECON_HD uint32_t prefix_share(uint32_t nlists, uint32_t nthreads) { return (nlists + nthreads - 1) / nthreads; }
RECON_HD uint32_t prefix_begin(uint32_t nlists, uint32_t nthreads, uint32_t t)
{
    const uint64_t b = (uint64_t)t * prefix_share(nlists, nthreads);
    return (uint32_t)(b < nlists ? b : nlists);
}

// the same on the host (the number of work items sizes the grid): chunk_off[l] = chunks of the lists before l; chunk_off[nlists] = items
inline std::vector<uint64_t> make_chunk_off(const std::vector<int64_t> &len)
{
    std::vector<uint64_t> off(len.size() + 1, 0);
    for (size_t l = 0; l < len.size(); ++l) off[l + 1] = off[l] + list_chunks((uint64_t)(len[l] > 0 ? len[l] : 0));
    return off;
}

// the list of work item `item` (item < chunk_off[nlists]): the last l with chunk_off[l] <= item.  Empty lists share their offset with
// the next list and are stepped over.
RECON_HD uint32_t item_list(const uint64_t *chunk_off, uint32_t nlists, uint64_t item)
{
    uint32_t lo = 0, hi = nlists;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (chunk_off[mid] <= item) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------------
enum Mode : int { MODE_NONE = 0, MODE_BITMAP = 1, MODE_HASH = 2 };

struct Plan {
    int mode = MODE_NONE;        // MODE_NONE: nothing wanted or nothing stored -- no launch, every id is absent
    bool span_from_want = false; // BITMAP: the host does not know the span -- the kernels take it from the wanted ids (span_of)
    uint32_t lo = 0;             // BITMAP, span known: first id of the span
    uint64_t nbits = 0;          // BITMAP, span known: ids of the span (hi - lo + 1); otherwise the id space, which bounds it
    uint64_t words = 0;          // BITMAP: words of the buffer
    uint64_t items = 0;          // work items of the pass
    uint32_t grid = 0;           // workgroups of the launch
    uint64_t id_bytes = 0;       // bytes of stored ids the pass streams (4 per stored entry below list_len)
};

// nwant sorted wanted ids (repeats allowed); span_known: want_lo / want_hi are the smallest and the largest of them
inline Plan make_plan(uint64_t nwant, bool span_known, uint32_t want_lo, uint32_t want_hi, uint64_t items, uint64_t stored, int num_cu)
{
    Plan p;
    p.items = items;
    p.id_bytes = stored * 4;
    if (nwant == 0 || items == 0) return p;
    const uint64_t cu = (uint64_t)(num_cu > 0 ? num_cu : 1);
    const uint64_t span = span_known ? (uint64_t)want_hi - (uint64_t)want_lo + 1 : ID_SPACE_BITS;
    if (span <= BITMAP_MAX_BITS || nwant > FILTER_MAX_WANTED) {
        p.mode = MODE_BITMAP;
        p.span_from_want = !span_known;
        p.lo = span_known ? want_lo : 0u;
        p.nbits = span;
        p.words = bitmap_words(span);
        const uint64_t cap = cu * GRID_WG_PER_CU_BITMAP;
        p.grid = (uint32_t)(items < cap ? items : cap);
    } else {
        p.mode = MODE_HASH;
        const uint64_t cap = cu * GRID_WG_PER_CU_HASH;
        p.grid = (uint32_t)(items < cap ? items : cap);
    }
    return p;
}

// ---- decode --------------------------------------------------------------------------------------------------------------------------
// component t of a vector lies in sub-space t / dsub, at offset t % dsub of its codeword; codebooks are m blocks of ksub codewords of dsub
RECON_HD uint32_t decode_block(uint32_t t, uint32_t dsub) { return t / dsub; }
RECON_HD uint64_t codeword_elem(uint32_t ii, uint32_t c, uint32_t t, uint32_t dsub, uint32_t ksub)
{
    return ((uint64_t)ii * ksub + c) * dsub + (t - ii * dsub);
}
// byte offset of the code row of position pos in a list whose codes start at codeoff (cs: the code stride in bytes)
RECON_HD uint64_t code_row(uint64_t codeoff, uint64_t pos, uint32_t cs) { return codeoff + pos * (uint64_t)cs; }
// the 8-bit handle's inverse labels: [m][256], slot = label byte, value = codeword index (0 for a byte that is no label)
RECON_HD uint32_t label_slot(uint32_t ii, uint32_t byte) { return ii * 256u + byte; }

}  // namespace recon
