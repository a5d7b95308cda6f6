// Planner and index arithmetic of ivfadc_score_ids (score.hip.h holds the kernel).  Plain C++ (no HIP types), in the manner of
// reconstruct_plan.h, so that the plan and every index the kernel forms compile and run without a GPU (tests/c/score_plan_check.cpp).
//
// A call scores nq x C PAIRS (query q, slot j): pair q * C + j, the index of its distance and of its found byte.  The id of the pair is
// ids[q * ids_stride + j], and there are exactly two stride forms: ids_stride == C, one row of candidates per query, and ids_stride == 0,
// ONE shared row scored against every query.  counts[q] (clamped to [0, C]; no counts: C) cuts a row: a slot at or behind it is DEAD, is
// answered +Inf / 0 and reads nothing of the index.
//
// The ids are located by the pass of reconstruct_plan.h (sort, one pass over the stored ids, resolve to (list, position) per slot), which
// keeps LOCATE_BYTES_PER_SLOT bytes of workspace per located slot.  Under a workspace limit the call is cut into SLICES of whole queries
// whose locate workspace fits (never fewer than one query); a slice is also at most MAX_SLICE_QUERIES queries, the y extent of a launch.
// The shared row is located ONCE, C slots whatever nq is, so only the y extent cuts it.  The located (list, position) of pair (q, j) of a
// slice that starts at query q0 stands at loc_index: (q - q0) * C + j per query, j for the shared row.
//
// One workgroup of TILE lanes takes one query and TILE consecutive slots of it: grid (tiles(C), queries of the slice).  A lane owns one
// pair and runs the three sequential Float32 chains of the distance itself (score.hip.h), so nothing is reduced across lanes and the
// only LDS is the query, d floats.
//
// Nothing here has been measured against an alternative.  The constants below are REASONED, NOT MEASURED.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SCORE_HD __host__ __device__ __forceinline__
#else
#define SCORE_HD inline
#endif

namespace score {

// slots of one query per workgroup = lanes of a workgroup, two waves: a row of 100 candidates leaves 28 lanes idle (156 at four waves),
// a row of 1000 fills 7.8 workgroups of 8; the per-workgroup cost, d floats of the query into LDS, is below 1 % of what its lanes read
// (2 d floats of centre and d of codewords EACH).  (REASONED, NOT MEASURED)
constexpr int TILE = 128;
// the most pairs of one call (their index and the located slots of a slice fit 31 bits)
constexpr int64_t MAX_PAIRS = 0x7FFFFFFF;
// the most queries of one slice: the y extent of a launch
constexpr int64_t MAX_SLICE_QUERIES = 65535;
// workspace the locate pass keeps per located slot: the sorted id (4), its key (8), list (4) and position (8) of the slot, and the sort's
// double buffer (4, rounded up to 8 for its histograms).  (the sort's share: REASONED, NOT MEASURED)
constexpr uint64_t LOCATE_BYTES_PER_SLOT = 32;

enum Form : int { FORM_BAD = 0, FORM_PER_QUERY = 1, FORM_SHARED = 2 };

// ids_stride == 0 is the shared row whatever C is (C == 0 scores nothing either way)
SCORE_HD int stride_form(int64_t C, int64_t ids_stride) { return ids_stride == 0 ? FORM_SHARED : ids_stride == C ? FORM_PER_QUERY : FORM_BAD; }
SCORE_HD bool pairs_fit(int64_t nq, int64_t C) { return nq <= 0 || C <= 0 || nq <= MAX_PAIRS / C; }

// ---- pair arithmetic, 64-bit ------------------------------------------------------------------------------------------------------------
SCORE_HD uint64_t pair_index(int64_t q, int64_t C, int64_t j) { return (uint64_t)q * (uint64_t)C + (uint64_t)j; }
SCORE_HD uint64_t id_index(int64_t q, int64_t ids_stride, int64_t j) { return (uint64_t)q * (uint64_t)ids_stride + (uint64_t)j; }
SCORE_HD uint64_t loc_index(bool shared, int64_t q_in_slice, int64_t C, int64_t j) { return shared ? (uint64_t)j : pair_index(q_in_slice, C, j); }
SCORE_HD int64_t live_slots(bool have_counts, int32_t count, int64_t C) { return !have_counts ? C : count < 0 ? 0 : count > C ? C : (int64_t)count; }
SCORE_HD uint64_t query_row(int64_t q, int d) { return (uint64_t)q * (uint64_t)d; }

// ---- tiles ------------------------------------------------------------------------------------------------------------------------------
SCORE_HD uint32_t tiles(int64_t C) { return (uint32_t)((C + TILE - 1) / TILE); }
SCORE_HD int64_t tile_slot(uint32_t tile, uint32_t lane) { return (int64_t)tile * TILE + (int64_t)lane; }
SCORE_HD size_t lds_bytes(int d) { return (size_t)d * 4; }
// 16-byte loads: a centre row starts at l * d floats, a codeword at (ii * ksub + c) * dsub floats and its part of the centre row at
// ii * dsub floats behind the row's start -- every one a multiple of four floats exactly when d, and dsub, are (the arrays themselves are
// allocations of the runtime, aligned far beyond 16 bytes).  d = 10 gives 40-byte rows: scalar loads.
SCORE_HD bool centre_vec4(int d) { return d % 4 == 0; }
SCORE_HD bool codeword_vec4(int dsub) { return dsub % 4 == 0; }

// ---- the plan -----------------------------------------------------------------------------------------------------------------------------
struct Plan {
    bool shared = false;
    int64_t nq = 0, C = 0;
    int64_t slice_nq = 0;        // queries of every slice but the last
    int64_t nslices = 0;
    int64_t locate_slots = 0;    // slots one locate pass resolves: C (shared: once per call) or slice_nq * C (once per slice)
    uint32_t grid_x = 0;         // workgroups per query
    size_t lds = 0;              // dynamic LDS of a workgroup
};

// nq > 0, C > 0, a valid stride form, pairs_fit(nq, C)
inline Plan make_plan(int64_t nq, int64_t C, int64_t ids_stride, int d, uint64_t ws_budget)
{
    Plan p;
    p.shared = stride_form(C, ids_stride) == FORM_SHARED;
    p.nq = nq;
    p.C = C;
    int64_t per = MAX_SLICE_QUERIES;
    if (!p.shared) {
        const uint64_t fit = ws_budget / (LOCATE_BYTES_PER_SLOT * (uint64_t)C);
        if (fit < (uint64_t)per) per = (int64_t)fit;
        if (per < 1) per = 1;
    }
    if (per > nq) per = nq;
    p.slice_nq = per;
    p.nslices = (nq + per - 1) / per;
    p.locate_slots = p.shared ? C : per * C;
    p.grid_x = tiles(C);
    p.lds = lds_bytes(d);
    return p;
}

SCORE_HD int64_t slice_begin(const Plan &p, int64_t s) { return s * p.slice_nq; }
SCORE_HD int64_t slice_queries(const Plan &p, int64_t s)
{
    const int64_t left = p.nq - slice_begin(p, s);
    return left < p.slice_nq ? left : p.slice_nq;
}

}  // namespace score
