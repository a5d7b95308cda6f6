// Planner and index arithmetic of ivfadc_rerank (rerank.hip.h holds the kernels).  Plain C++ (no HIP types), in the manner of score_plan.h,
// so that the plan and every index the kernels form compile and run without a GPU (tests/c/rerank_plan_check.cpp).
//
// A call re-scores nq x C PAIRS (query q, slot j) against a vector store of n rows of d components (Float32, or Float16 widened exactly).
// The id of pair (q, j) is ids[q * C + j]; counts[q] (clamped to [0, C]; no counts: C) cuts a row: a slot at or behind it is DEAD.  A dead
// slot and a slot whose id is at or beyond n read nothing of the store and carry the all-ones key.
//
// Distance pass: grid (tiles(C), queries of the slice), a workgroup of TILE lanes = WAVES waves, a wave owns 64 consecutive slots of one
// query.  The rows are walked in CHUNKS of CHUNK_DWORDS dwords = one 128-byte line of a row (32 Float32 or 64 Float16 components).  The wave
// fetches the chunk of its 64 rows cooperatively: LANES_PER_ROW lanes of 16 bytes cover one row's line, so one wave load brings
// ROWS_PER_LOAD whole lines and LOADS loads bring all 64.  Lane L fetches dwords gather_dword(L, 0..3) of rows gather_row(L, 0..LOADS-1).
// The chunk lands in the wave's LDS tile, [row][dword] with a row stride of ROW_STRIDE dwords (odd: lane r reading dword t of row r hits
// bank (r + t) mod 32, two lanes per bank, the rate of a wave64 read).  Then lane r runs its own row's chain over the chunk.
// LDS of a workgroup: the query (d floats, rounded up to four) and one tile per wave.
//
// Select pass: one workgroup per query.  C <= SELECT_LDS_MAX: the keys are sorted in LDS, padded to padded_keys(C); above it they go
// through the segmented radix sort of the generic search path, which needs a second key buffer.
//
// Under a workspace limit the call is cut into SLICES of whole queries whose keys fit (never fewer than one query); a slice is also at
// most MAX_SLICE_QUERIES queries, the y extent of a launch.  Key of pair (q, j) of a slice that starts at q0: key_index(q - q0, C, j).
//
// Nothing here has been measured against an alternative.  The constants below are REASONED, NOT MEASURED.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RERANK_HD __host__ __device__ __forceinline__
#else
#define RERANK_HD inline
#endif

namespace rerank {

constexpr int WAVE = 64;
// four waves: a row of 100 candidates leaves two waves without a live slot (they leave at once), a row of 1000 fills 3.9 workgroups of
// 4; the per-workgroup cost, d floats of the query into LDS, is shared by 256 rows of the same length.  (REASONED, NOT MEASURED)
constexpr int WAVES = 4;
constexpr int TILE = WAVE * WAVES;
// one 128-byte line of a row per chunk: the unit HBM and the L2 move, whatever the component type
constexpr int CHUNK_DWORDS = 32;
constexpr int CHUNK_BYTES = CHUNK_DWORDS * 4;
constexpr int LANES_PER_ROW = CHUNK_BYTES / 16;          // 8
constexpr int ROWS_PER_LOAD = WAVE / LANES_PER_ROW;      // 8
constexpr int LOADS = WAVE / ROWS_PER_LOAD;              // 8: 32 staging registers per lane
constexpr int ROW_STRIDE = CHUNK_DWORDS + 1;             // odd
constexpr int TILE_DWORDS = WAVE * ROW_STRIDE;
// the most pairs of one call (their index fits 31 bits, a slot fits the low word of a key)
constexpr int64_t MAX_PAIRS = 0x7FFFFFFF;
constexpr int64_t MAX_SLICE_QUERIES = 65535;
// the LDS sort holds padded_keys(C) keys of 8 bytes: 32 KB at 4096, two workgroups per CU beside the runtime's own use.  (REASONED, NOT MEASURED)
constexpr int64_t SELECT_LDS_MAX = 4096;
// the longest vector a store takes: the query sits in LDS beside the tiles (64 KB of query + 33 KB of tiles, inside the 160 KB of a CU)
constexpr int MAX_D = 16384;
constexpr uint64_t KEY_DEAD = 0xFFFFFFFFFFFFFFFFull;

enum StoreType : int { STORE_F32 = 0, STORE_F16 = 1 };
enum SelectForm : int { SELECT_LDS = 0, SELECT_SORT = 1 };

RERANK_HD bool pairs_fit(int64_t nq, int64_t C) { return nq <= 0 || C <= 0 || nq <= MAX_PAIRS / C; }

// ---- the store ----------------------------------------------------------------------------------------------------------------------------
RERANK_HD uint64_t elem_bytes(bool f16) { return f16 ? 2u : 4u; }
RERANK_HD uint64_t row_bytes(int d, bool f16) { return (uint64_t)d * elem_bytes(f16); }
RERANK_HD uint64_t row_offset(uint64_t v, int d, bool f16) { return v * row_bytes(d, f16); }        // bytes; v < n <= 2^32, d < 2^31
RERANK_HD uint64_t store_bytes(uint64_t n, int d, bool f16) { return n * row_bytes(d, f16); }
// 16-byte loads: row v starts at v * row_bytes, a multiple of 16 for every v exactly when row_bytes is (the store is an allocation of the
// runtime, aligned far beyond 16 bytes), and a 16-byte piece that starts inside such a row ends inside it.  d = 10 gives 40-byte rows: no.
RERANK_HD bool vec16(int d, bool f16) { return row_bytes(d, f16) % 16 == 0; }
RERANK_HD int chunk_elems(bool f16) { return f16 ? 2 * CHUNK_DWORDS : CHUNK_DWORDS; }
RERANK_HD int chunks(int d, bool f16) { return (d + chunk_elems(f16) - 1) / chunk_elems(f16); }
// components of chunk c that exist
RERANK_HD int chunk_len(int d, bool f16, int c)
{
    const int left = d - c * chunk_elems(f16);
    return left < chunk_elems(f16) ? left : chunk_elems(f16);
}

// ---- pairs, tiles, the cooperative fetch ----------------------------------------------------------------------------------------------------
RERANK_HD uint64_t id_index(int64_t q, int64_t C, int64_t j) { return (uint64_t)q * (uint64_t)C + (uint64_t)j; }
RERANK_HD uint64_t key_index(int64_t q_in_slice, int64_t C, int64_t j) { return (uint64_t)q_in_slice * (uint64_t)C + (uint64_t)j; }
RERANK_HD uint64_t out_index(int64_t q, int K, int64_t i) { return (uint64_t)q * (uint64_t)K + (uint64_t)i; }
RERANK_HD uint64_t query_row(int64_t q, int d) { return (uint64_t)q * (uint64_t)d; }
RERANK_HD int64_t live_slots(bool have_counts, int32_t count, int64_t C) { return !have_counts ? C : count < 0 ? 0 : count > C ? C : (int64_t)count; }
RERANK_HD uint32_t tiles(int64_t C) { return (uint32_t)((C + TILE - 1) / TILE); }
RERANK_HD int64_t tile_slot(uint32_t tile, uint32_t thread) { return (int64_t)tile * TILE + (int64_t)thread; }
RERANK_HD int gather_row(int lane, int i) { return (lane / LANES_PER_ROW) + ROWS_PER_LOAD * i; }    // row of the wave's 64, i < LOADS
RERANK_HD int gather_dword(int lane, int k) { return (lane % LANES_PER_ROW) * 4 + k; }               // dword of the chunk, k < 4
RERANK_HD uint64_t chunk_byte(int c, int dword) { return (uint64_t)c * CHUNK_BYTES + (uint64_t)dword * 4; }   // within the row

// ---- LDS of the distance pass, in dwords ----------------------------------------------------------------------------------------------------
RERANK_HD uint32_t query_dwords(int d) { return ((uint32_t)d + 3u) & ~3u; }
RERANK_HD uint32_t tile_base(int d, int wave) { return query_dwords(d) + (uint32_t)wave * TILE_DWORDS; }
RERANK_HD uint32_t tile_index(int row, int dword) { return (uint32_t)row * ROW_STRIDE + (uint32_t)dword; }
RERANK_HD size_t dist_lds_bytes(int d) { return ((size_t)query_dwords(d) + (size_t)WAVES * TILE_DWORDS) * 4; }

// ---- the select pass --------------------------------------------------------------------------------------------------------------------------
RERANK_HD int select_form(int64_t C) { return C <= SELECT_LDS_MAX ? SELECT_LDS : SELECT_SORT; }
// C <= SELECT_LDS_MAX: the power of two the LDS sort runs on, at least one wave's run
RERANK_HD int padded_keys(int64_t C)
{
    int p = WAVE;
    while (p < C) p <<= 1;
    return p;
}
RERANK_HD size_t select_lds_bytes(int64_t C) { return select_form(C) == SELECT_LDS ? (size_t)padded_keys(C) * 8 : 0; }
// compare-exchange p (of P / 2) of a merge network's stages: the FLIP stage of merge width k pairs i with i ^ (k - 1), a stage of stride j
// pairs i with i + j (bit j of i clear); both keep the minimum at the lower index
RERANK_HD void flip_pair(int p, int k, int &lo, int &hi)
{
    const int half = k >> 1, block = p / half, off = p % half;
    lo = block * k + off;
    hi = block * k + k - 1 - off;
}
RERANK_HD void stride_pair(int p, int j, int &lo, int &hi)
{
    lo = (p / j) * 2 * j + p % j;
    hi = lo + j;
}
// workspace per slot: the key, and in the sort form the sorted key beside it (the sort's own scratch is the generic path's buffer)
RERANK_HD uint64_t bytes_per_slot(int form) { return form == SELECT_LDS ? 8u : 16u; }

// ---- the plan -----------------------------------------------------------------------------------------------------------------------------
struct Plan {
    int64_t nq = 0, C = 0;
    bool f16 = false, vec = false;
    int form = SELECT_LDS;
    int64_t slice_nq = 0;        // queries of every slice but the last
    int64_t nslices = 0;
    int64_t slice_keys = 0;      // keys of a full slice
    uint32_t grid_x = 0;         // workgroups per query of the distance pass
    int nchunks = 0;
    size_t dist_lds = 0, select_lds = 0;
    int padded = 0;              // LDS form: keys the sort runs on
};

// nq > 0, C > 0, pairs_fit(nq, C), d > 0
inline Plan make_plan(int64_t nq, int64_t C, int d, bool f16, uint64_t ws_budget)
{
    Plan p;
    p.nq = nq;
    p.C = C;
    p.f16 = f16;
    p.vec = vec16(d, f16);
    p.form = select_form(C);
    int64_t per = MAX_SLICE_QUERIES;
    const uint64_t fit = ws_budget / (bytes_per_slot(p.form) * (uint64_t)C);
    if (fit < (uint64_t)per) per = (int64_t)fit;
    if (per < 1) per = 1;
    if (per > nq) per = nq;
    p.slice_nq = per;
    p.nslices = (nq + per - 1) / per;
    p.slice_keys = per * C;
    p.grid_x = tiles(C);
    p.nchunks = chunks(d, f16);
    p.dist_lds = dist_lds_bytes(d);
    p.select_lds = select_lds_bytes(C);
    p.padded = p.form == SELECT_LDS ? padded_keys(C) : 0;
    return p;
}

RERANK_HD int64_t slice_begin(const Plan &p, int64_t s) { return s * p.slice_nq; }
RERANK_HD int64_t slice_queries(const Plan &p, int64_t s)
{
    const int64_t left = p.nq - slice_begin(p, s);
    return left < p.slice_nq ? left : p.slice_nq;
}

}  // namespace rerank
