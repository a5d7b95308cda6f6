// Planner of the range search (ivfadc_range_search; range.hip.h holds the kernels).  Plain C++ (no HIP types), in the manner of
// maskset_plan.h / subset_plan.h, so that the arithmetic the host runtime and the kernels share compiles and runs without a GPU
// (tests/c/range_plan_check.cpp).
//
// A range search has no reference counterpart: it is knn_search (index.jl:204-258) with K at least the number of
// probed points, cut after the last entry whose Float32 distance d satisfies d <= r.
//
// Work item: one (query, probe j, chunk c of the probed list).  The items of a query are a dense w x maxch grid, maxch the chunks of the
// LONGEST list: item j * maxch + c covers positions [c * chunk, min(len, (c + 1) * chunk)) of probe j's list and is empty where that
// range is.  Two passes over the same grid: the count pass leaves one u32 per item, an exclusive scan of a query's items gives every
// item its slot range among the query's keys, the fill pass writes the keys there.
//
// INVARIANT (masked items, range.hip.h): a chunk is a multiple of 64 points -- the default chunks are multiples of CHUNK_ALIGN = 256, the
// table-free default is TABLE_FREE_CHUNK = 1024, a forced chunk is rounded up to FORCED_ALIGN = 64 -- so chunk_begin(c, chunk) is a
// multiple of 64 for every c, and the 64 points a wave takes in a round of THREADS = 256 (positions chunk_begin + 256 k + 64 wave ...)
// are exactly one round of a mask row (maskset_plan.h: maskset::round_word, two whole words).  chunk_is_round_aligned states it;
// tests/c/range_masked_plan_check.cpp checks it and the word addressing of every item of every list.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define RANGE_HD __host__ __device__ __forceinline__
#else
#define RANGE_HD inline
#endif

namespace range_plan {

constexpr int THREADS = 256;          // lanes of a work item: one point per lane and round
constexpr int CHUNK_ALIGN = 256;      // the default chunk is a multiple of a round
constexpr int FORCED_ALIGN = 64;      // a forced chunk (ivfadc_set_tuning's chunk_points) is rounded up to whole waves: 64 is the smallest
constexpr size_t COUNTER_BYTES = 16;  // the item's survivor counter, behind the tables
constexpr uint64_t VISIT_LIMIT = (uint64_t)1 << 32;   // visit orders are the low 32 bits of a key (as everywhere else)

RANGE_HD uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// LDS of a work item: residual (d floats, padded to 4), m tables of 256 floats, the counter
RANGE_HD size_t lds_bytes(int d, int m) { return ((size_t)round_up((uint64_t)d, 4) + (size_t)m * 256) * 4 + COUNTER_BYTES; }

// Table-free items (16-bit codes, range_u16_*_kernel): no tables.  The residual lies in LDS as [m][dsp], dsp = dsub rounded up to 4 so
// that one 16-byte broadcast read serves four terms, and the counter behind it.
RANGE_HD size_t lds_bytes_table_free(int m, int dsub) { return (size_t)m * (size_t)round_up((uint64_t)(dsub > 0 ? dsub : 1), 4) * 4 + COUNTER_BYTES; }
// Their default chunk: the 8 * ksub * d / m rule below prices a table build that does not exist here.  A table-free item pays only its
// residual (d subtractions) and its launch slot, so the chunk is short: four rounds of 256 points keep the residual's cost below a
// thousandth of the gathers and give a 100 000-point list about a hundred items to spread over the compute units.
// REASONED, NOT MEASURED: no sweep of this constant has been run; ivfadc_set_tuning(h, qg, chunk_points) overrides it.
constexpr uint32_t TABLE_FREE_CHUNK = 1024;

RANGE_HD bool chunk_is_round_aligned(uint32_t chunk) { return chunk != 0 && chunk % 64u == 0; }

// Chunk length when none is forced (table form).  A work item builds its probe's tables (ksub * d multiply-adds: m tables of ksub entries of dsub
// terms) before it looks anything up (chunk * m lookups): the chunk is long enough that the build costs at most about an eighth of the
// lookups -- chunk >= 8 * ksub * d / m -- rounded up to a multiple of 256.  REASONED, NOT MEASURED: no sweep of this constant has been
// run; ivfadc_set_tuning(h, qg, chunk_points) overrides it.
RANGE_HD uint32_t default_chunk(int d, int m, int ksub)
{
    const uint64_t build = (uint64_t)ksub * (uint64_t)d;
    const uint64_t want = (8 * build + (uint64_t)m - 1) / (uint64_t)m;
    const uint64_t c = round_up(want < 1 ? 1 : want, CHUNK_ALIGN);
    return (uint32_t)(c > ((uint64_t)1 << 30) ? ((uint64_t)1 << 30) : c);
}

RANGE_HD uint32_t forced_chunk(int chunk_points)
{
    const uint64_t c = round_up((uint64_t)chunk_points, FORCED_ALIGN);
    return (uint32_t)(c > ((uint64_t)1 << 30) ? ((uint64_t)1 << 30) : c);
}

// chunks of a list of `len` points
RANGE_HD uint64_t chunks_of(uint64_t len, uint32_t chunk) { return (len + chunk - 1) / chunk; }

// the one definition of "positions of chunk c" (kernels, CPU check): [chunk_begin, chunk_end), empty when chunk_begin >= len
RANGE_HD uint64_t chunk_begin(uint64_t c, uint32_t chunk) { return c * (uint64_t)chunk; }
RANGE_HD uint64_t chunk_end(uint64_t len, uint64_t c, uint32_t chunk)
{
    const uint64_t e = (c + 1) * (uint64_t)chunk;
    return e < len ? e : len;
}

// item of (probe j, chunk c), and back
RANGE_HD uint64_t item_of(uint64_t j, uint64_t c, uint64_t maxch) { return j * maxch + c; }
RANGE_HD uint64_t probe_of(uint64_t item, uint64_t maxch) { return item / maxch; }
RANGE_HD uint64_t chunk_of(uint64_t item, uint64_t maxch) { return item % maxch; }

// The radius as the kernels compare it.  Distances are non-negative finite floats (dc >= +0, table entries >= +0), whose bit patterns
// order as unsigned integers; a radius joins that order only when it is >= 0 and no NaN -- the caller ends the item first otherwise
// (radius_live) -- and -0.0f, which compares equal to +0.0f, must not compare as 0x80000000.
RANGE_HD bool radius_live(float r) { return r >= 0.0f; }   // false for r < 0 and for NaN: no results
RANGE_HD uint32_t radius_bits(float r, uint32_t bits_of_r) { return r == 0.0f ? 0u : bits_of_r; }

struct Facts {
    int d = 0, kc = 0, m = 0, ksub = 0;
    int64_t n = 0, maxlen = 0;       // stored points, longest list
    int force_chunk = 0;             // ivfadc_set_tuning's chunk_points (0: the default)
    size_t ws_budget = 0;            // ivfadc_set_workspace_limit
    size_t lds_max = 0;              // LDS of a CU a workgroup may take (scan_layouts.h: LDS_MAX)
    bool table_free = false;         // 16-bit codes: sums straight from the codebook, LDS from the residual alone (d = m * dsub)
    bool masked = false;             // ivfadc_range_search_masked with a set: a query's share grows by its ingested mask number
};

struct Plan {
    bool fits = false;
    const char *why = "";            // what does not fit
    uint32_t chunk = 0;
    size_t lds = 0;
    int64_t maxch = 0;               // chunks of the longest list (>= 1)
    int64_t items = 0;               // work items of a query: w * maxch
    int64_t nb = 0;                  // queries of a sub-batch (>= 1): probe arrays, coarse keys and item words inside ws_budget
    int64_t cap_keys = 0;            // keys of a sort group: two key buffers and the sort's scratch (24 B a key) inside ws_budget
    int64_t per_query_bytes = 0;
};

// a launch's gridDim.x * blockDim.x stays below 2^32 (HIP refuses the launch otherwise): 2^32 / THREADS - 1 work items of a query
constexpr int64_t MAX_GRID_X = ((int64_t)1 << 32) / THREADS - 1, MAX_GRID_Y = 65535;

// keys of a sort group (range search and the generic path alike): two key buffers and the sort's scratch, 24 B a key, inside the
// workspace budget; never fewer than 2^20
inline int64_t sort_cap_keys(size_t ws_budget)
{
    const int64_t cap = (int64_t)(ws_budget / 24);
    return cap < ((int64_t)1 << 20) ? (int64_t)1 << 20 : cap;
}

inline Plan make_plan(const Facts &f, int64_t nq, int w)
{
    Plan p;
    p.lds = f.table_free ? lds_bytes_table_free(f.m, f.m > 0 ? f.d / f.m : f.d) : lds_bytes(f.d, f.m);
    if (p.lds > f.lds_max) { p.why = f.table_free ? "the residual exceeds the LDS of a compute unit" : "the tables of one probe exceed the LDS of a compute unit"; return p; }
    // a query's visit orders count its probed points: fewer than 2^32 when the index holds fewer (the generic path's limit)
    if ((uint64_t)f.n >= VISIT_LIMIT) { p.why = "a query may probe 2^32 points or more: visit orders are 32-bit"; return p; }
    p.chunk = f.force_chunk > 0 ? forced_chunk(f.force_chunk) : (f.table_free ? TABLE_FREE_CHUNK : default_chunk(f.d, f.m, f.ksub));
    p.maxch = (int64_t)chunks_of((uint64_t)(f.maxlen > 0 ? f.maxlen : 0), p.chunk);
    if (p.maxch < 1) p.maxch = 1;
    p.items = (int64_t)w * p.maxch;
    if (p.items > MAX_GRID_X) { p.why = "w x chunks of the longest list exceeds a launch grid: force a longer chunk"; return p; }
    // a query's share of the workspace: coarse row and its keys twice over (4 + 16), probe arrays (12), item counts and offsets (8 an
    // item), total and key offset; masked: the ingested mask number (4)
    p.per_query_bytes = (int64_t)f.kc * 20 + (int64_t)w * 12 + p.items * 8 + 64 + (f.masked ? 4 : 0);
    int64_t nb = (int64_t)(f.ws_budget / (size_t)p.per_query_bytes);
    if (nb < 1) nb = 1;
    const int64_t by_rows = (((int64_t)1 << 31) - 1) / (f.kc > 0 ? f.kc : 1);   // the coarse rows of a sub-batch are sorted in one call: fewer than 2^31 keys
    if (nb > by_rows) nb = by_rows;
    if (nb > MAX_GRID_Y) nb = MAX_GRID_Y;
    if (nq > 0 && nb > nq) nb = nq;
    if (nb < 1) nb = 1;
    p.nb = nb;
    p.cap_keys = sort_cap_keys(f.ws_budget);
    p.fits = true;
    return p;
}

// Sort groups of a sub-batch: queries g0 .. g1 - 1 whose keys fit cap_keys together (one query alone always goes) and stay below 2^32
// (the segmented sort's offsets are 32-bit).  tot: keys per query.  Returns g1 > g0, or g0 when query g0 alone has 2^32 keys or more.
inline int64_t next_group(const std::vector<uint64_t> &tot, int64_t g0, int64_t cap_keys, uint64_t *keys_out)
{
    int64_t g1 = g0;
    uint64_t keys = 0;
    const int64_t n = (int64_t)tot.size();
    while (g1 < n && g1 - g0 < MAX_GRID_Y && (g1 == g0 || keys + tot[(size_t)g1] <= (uint64_t)cap_keys) && keys + tot[(size_t)g1] < VISIT_LIMIT)
        keys += tot[(size_t)g1++];
    if (keys_out) *keys_out = keys;
    return g1;
}

// lims of a batch from its per-query totals: 64-bit throughout (a SIFT1B batch holds more than 2^32 results)
inline std::vector<int64_t> make_lims(const std::vector<uint64_t> &tot)
{
    std::vector<int64_t> lims(tot.size() + 1, 0);
    for (size_t q = 0; q < tot.size(); ++q) lims[q + 1] = lims[q] + (int64_t)tot[q];
    return lims;
}

}  // namespace range_plan
