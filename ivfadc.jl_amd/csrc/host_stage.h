// What the host-pointer service entries (ivfadc_locate, ivfadc_reconstruct, ivfadc_score_ids, ivfadc_rerank, ivfadc_search_refined,
// ivfadc_coarse_search, the host range entries) do on the host besides HIP calls; DESIGN.md 4.8 states the arena's rule.
// Plain C++ (no HIP types, no handle), in the manner of batch_plan.h / range_plan.h: it compiles and runs without a GPU
// (tests/c/host_stage_check.cpp).  The .hip file keeps the HIP calls: the arena's one ensure, h2d_copy, d2h_copy.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace host_stage {

// ---- the layout of one call's staging arena -----------------------------------------------------------------------------------------
// Parts are added with their byte length and stand in the order they were added, each at a multiple of ALIGN (the alignment of a device
// allocation's start, so a part is aligned as a buffer of its own was).  The layout is FINISHED before a pointer is formed from it: the
// arena grows once, to `total`, and no pointer handed out can be left behind by a later part.  A part of no bytes is legal, takes no room
// and has a valid offset.  A total past size_t, or a part too many, sets `overflow` (refused by the caller), never wraps.
constexpr size_t ALIGN = 256;
constexpr int MAX_PARTS = 8;
struct Layout {
    size_t off[MAX_PARTS] = {}, len[MAX_PARTS] = {};
    int parts = 0;
    size_t total = 0;
    bool overflow = false;
    // the new part's number (with overflow set: the last part's, which the caller never uses)
    int add(size_t bytes)
    {
        const size_t padded = bytes + (ALIGN - 1);   // (wraps exactly when rounding `bytes` up would)
        if (parts == MAX_PARTS || padded < bytes || padded / ALIGN * ALIGN > ~(size_t)0 - total) {
            overflow = true;
            return MAX_PARTS - 1;
        }
        off[parts] = total;
        len[parts] = bytes;
        total += padded / ALIGN * ALIGN;
        return parts++;
    }
};

// ---- counts[q] in [0, C] ---------------------------------------------------------------------------------------------------------------
// -1, or the first query whose count lies outside (no counts: -1)
inline int64_t first_bad_count(const int32_t *counts, int64_t nq, int64_t C)
{
    for (int64_t q = 0; counts && q < nq; ++q)
        if (counts[q] < 0 || (int64_t)counts[q] > C) return q;
    return -1;
}

// ---- the ids of the live slots of a score call -----------------------------------------------------------------------------------------
// Per-query rows: row q is ids[q * C ..], its first counts[q] slots are live (no counts: all C).  The shared row: ids[0 .. C), live up to
// the LARGEST count (no counts: C) -- a slot any query reads.  Counts are taken as clamped to [0, C].  No live slot: a span of one id, 0.
struct IdSpan {
    bool any;
    uint32_t lo, hi;
};
inline IdSpan live_id_span(int64_t nq, int64_t C, bool shared, const uint32_t *ids, const int32_t *counts)
{
    const auto live = [&](int64_t q) { return !counts ? C : counts[q] < 0 ? 0 : counts[q] > C ? C : (int64_t)counts[q]; };
    int64_t longest = 0;
    for (int64_t q = 0; q < nq; ++q) longest = live(q) > longest ? live(q) : longest;
    IdSpan s{false, 0xFFFFFFFFu, 0u};
    for (int64_t q = 0; q < (shared && nq > 0 ? 1 : nq); ++q) {
        const uint32_t *row = ids + (shared ? 0 : (size_t)q * (size_t)C);
        for (int64_t j = 0, n = shared ? longest : live(q); j < n; ++j) {
            s.lo = row[j] < s.lo ? row[j] : s.lo;
            s.hi = row[j] > s.hi ? row[j] : s.hi;
            s.any = true;
        }
    }
    return s.any ? s : IdSpan{false, 0u, 0u};
}

// ---- result rows of the re-rank host entries ---------------------------------------------------------------------------------------------
// src: nq rows of Kw 32-bit slots; dst: nq rows of K.  The first counts[q] slots (clamped to [0, Kw]) of every row go over; a destination
// slot at or behind the count is not written.
inline void compact_rows(int64_t nq, int Kw, int K, const int32_t *counts, const void *src, void *dst)
{
    for (int64_t q = 0; q < nq; ++q) {
        const size_t cnt = (size_t)(counts[q] < 0 ? 0 : counts[q] > Kw ? Kw : counts[q]);
        memcpy((uint8_t *)dst + (size_t)q * (size_t)K * 4, (const uint8_t *)src + (size_t)q * (size_t)Kw * 4, cnt * 4);
    }
}

}  // namespace host_stage
