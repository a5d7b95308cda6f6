// Record layout and index arithmetic of the PQ vector store (store_type 2: ivfadc_vectors_create_pq, re-ranked by rerank_pq_dist_kernel in
// rerank.hip.h).  Plain C++ (no HIP types), a sibling of rerank_plan.h, so that the stride, every field offset and every address the two
// kernels form compile and run without a GPU (tests/c/vstore_pq_plan_check.cpp).
//
// Row v of the store is one RECORD: list_v (uint32, little-endian), m base codeword INDICES, m2 refinement codeword indices, one byte each,
// then zero padding up to the stride.  The stride is the power of two at or above the 4 + m + m2 bytes in use (at least 8), so a record
// never straddles a 128-byte line, nor a 32- or 64-byte sector once it fits one: m = 8, m2 = 16 is 28 bytes in a 32-byte record, one
// sector per candidate.  4 + m + m2 <= MAX_RECORD.
//
// The store owns copies of the centroids [kc][d], the base codebooks [m][ksub][dsub] and the refinement codebooks [m2][k2][dsub2].
// Component t of row v is reconstructed as (c[list][t] + B[t / dsub][code][t % dsub]) + R[t / dsub2][code2][t % dsub2].
//
// rerank_pq_dist_kernel keeps rerank_dist_kernel's decomposition (rerank_plan.h: a wave owns 64 slots, chunks of 32 components through the
// wave's [row][dword] tile).  Two things are added.  The wave first brings its 64 records into LDS in PIECES of 16 bytes (4 where the
// stride is 8): piece i of the wave is bytes piece_byte(i) .. of row piece_row(i); consecutive lanes read consecutive pieces, so the lanes
// of one record read one contiguous run.  Then, per chunk, lane L RECONSTRUCTS components gather_dword(L, 0..3) of rows gather_row(L, i):
// vec4(...) true, each of the three operands is ONE aligned 16-byte piece that stays inside its centroid row and its codeword (dsub and
// dsub2 are multiples of 4, so four components that start at a multiple of 4 share a sub-space of either quantizer); otherwise the four
// components are addressed one by one.
// LDS of a workgroup: the query and the tiles as rerank_plan.h lays them out, then one block of 64 records per wave; on the staged route
// (below) the chunk's two codebook slices behind them.
#pragma once

#include "rerank_plan.h"

namespace vspq {

constexpr int STORE_PQ = 2;          // store_type
constexpr int MAX_K2 = 256;          // a refinement code is one byte
constexpr int LIST_BYTES = 4;
// with d = rerank::MAX_D the query (64 KB), the tiles (33 KB) and 4 x 64 records of 128 bytes (32 KB) stay inside the 160 KB of a CU
constexpr uint32_t MAX_RECORD = 128;
constexpr uint32_t MIN_STRIDE = 8;

// ---- the record ---------------------------------------------------------------------------------------------------------------------------
RERANK_HD uint32_t raw_bytes(int m, int m2) { return (uint32_t)LIST_BYTES + (uint32_t)m + (uint32_t)m2; }
RERANK_HD bool record_fits(int m, int m2) { return m >= 1 && m2 >= 1 && (int64_t)m + (int64_t)m2 <= (int64_t)MAX_RECORD - LIST_BYTES; }
// record_fits(m, m2)
RERANK_HD uint32_t stride(int m, int m2)
{
    uint32_t s = MIN_STRIDE;
    while (s < raw_bytes(m, m2)) s <<= 1;
    return s;
}
RERANK_HD uint32_t off_list() { return 0u; }
RERANK_HD uint32_t off_code(int j) { return (uint32_t)LIST_BYTES + (uint32_t)j; }               // j < m
RERANK_HD uint32_t off_code2(int m, int j) { return (uint32_t)LIST_BYTES + (uint32_t)m + (uint32_t)j; }   // j < m2
RERANK_HD uint64_t record_offset(uint64_t v, uint32_t stride) { return v * (uint64_t)stride; }    // v < n <= 2^32
RERANK_HD uint64_t store_bytes(uint64_t n, uint32_t stride) { return n * (uint64_t)stride; }

// ---- the cooperative fetch of a wave's 64 records -------------------------------------------------------------------------------------------
RERANK_HD uint32_t piece_bytes(uint32_t stride) { return stride % 16u == 0u ? 16u : 4u; }
RERANK_HD uint32_t pieces(uint32_t stride) { return (uint32_t)rerank::WAVE * (stride / piece_bytes(stride)); }   // a multiple of 64
RERANK_HD int piece_row(uint32_t i, uint32_t stride) { return (int)(i / (stride / piece_bytes(stride))); }
RERANK_HD uint32_t piece_byte(uint32_t i, uint32_t stride) { return (i % (stride / piece_bytes(stride))) * piece_bytes(stride); }

// ---- the reconstruction ---------------------------------------------------------------------------------------------------------------------
RERANK_HD bool vec4(int d, int m, int m2) { return (d / m) % 4 == 0 && (d / m2) % 4 == 0; }
RERANK_HD int chunk_comp(int c, int dword) { return c * rerank::CHUNK_DWORDS + dword; }                   // component of the row
RERANK_HD int sub_of(int t, int dsub) { return t / dsub; }
RERANK_HD int sub_at(int t, int dsub) { return t % dsub; }
RERANK_HD uint64_t centroid_elem(uint32_t list, int d, int t) { return (uint64_t)list * (uint64_t)d + (uint64_t)t; }
// element `at` of codeword c of sub-space j of a codebook array [nsub][k][dsub]
RERANK_HD uint64_t codeword_elem(int j, uint32_t c, int at, int dsub, int k) { return ((uint64_t)j * (uint64_t)k + c) * (uint64_t)dsub + (uint64_t)at; }

// ---- LDS of the distance pass, in dwords ----------------------------------------------------------------------------------------------------
RERANK_HD uint32_t wave_record_dwords(uint32_t stride) { return (uint32_t)rerank::WAVE * stride / 4u; }
RERANK_HD uint32_t record_base(int d, int wave, uint32_t stride) { return rerank::tile_base(d, rerank::WAVES) + (uint32_t)wave * wave_record_dwords(stride); }
RERANK_HD size_t dist_lds_bytes(int d, uint32_t stride) { return rerank::dist_lds_bytes(d) + (size_t)rerank::WAVES * wave_record_dwords(stride) * 4; }

// ---- the staged route of the distance pass --------------------------------------------------------------------------------------------------
// ROUTE_STAGED: before a chunk is reconstructed the workgroup copies the chunk's SLICE of both codebooks into LDS -- of every codeword of
// the sub-spaces the chunk touches, the 32 components that lie in the chunk, as SLICE_PIECES pieces of four -- and the lanes take their
// codeword pieces from there; only the centroid piece still comes through the L2.  Piece g of codeword `code` stands at dword
// slice_piece(code, g) of its slice: consecutive lanes of the copy write consecutive pieces.  The base slice follows the records, the
// refinement slice follows the base slice.  vec4 shapes only, and only where the whole fits a workgroup's LDS (staged_fits).
enum Route : int { ROUTE_L2 = 0, ROUTE_STAGED = 1 };
constexpr int SLICE_PIECES = rerank::LANES_PER_ROW;      // 8 pieces of four components: one chunk of a codeword
constexpr size_t STAGED_LDS_MAX = (size_t)160 << 10;     // the LDS of a CU
RERANK_HD uint32_t slice_pieces(int k) { return (uint32_t)k * (uint32_t)SLICE_PIECES; }
RERANK_HD uint32_t slice_dwords(int k) { return slice_pieces(k) * 4u; }
RERANK_HD uint32_t slice_code(uint32_t e) { return e / (uint32_t)SLICE_PIECES; }                    // piece e of the copy: codeword
RERANK_HD int slice_g(uint32_t e) { return (int)(e % (uint32_t)SLICE_PIECES); }                     // ... and which four components
RERANK_HD uint32_t slice_piece(uint32_t code, int g) { return (code * (uint32_t)SLICE_PIECES + (uint32_t)g) * 4u; }   // dword in the slice
RERANK_HD uint32_t slice_base(int d, uint32_t stride) { return record_base(d, rerank::WAVES, stride); }               // the base slice
RERANK_HD size_t staged_lds_bytes(int d, uint32_t stride, int ksub, int k2) { return dist_lds_bytes(d, stride) + ((size_t)slice_dwords(ksub) + slice_dwords(k2)) * 4; }
RERANK_HD bool staged_fits(int d, int m, int m2, int ksub, int k2) { return vec4(d, m, m2) && staged_lds_bytes(d, stride(m, m2), ksub, k2) <= STAGED_LDS_MAX; }

// ---- creation -------------------------------------------------------------------------------------------------------------------------------
// LDS of vstore_pq_encode_kernel: the residual (d floats, rounded up to four), then one key per base and per refinement sub-space
RERANK_HD size_t encode_lds_bytes(int d, int m, int m2) { return (size_t)rerank::query_dwords(d) * 4 + ((size_t)m + (size_t)m2) * 8; }
// rows of one block of the creation: their coarse distances (kc floats), their data (d floats, host entry) and their assignment fit the
// workspace limit; never fewer than 1, never more than the 2^30 bytes of distances the encoder's own batches keep to
inline int64_t block_rows(int64_t n, int d, int kc, uint64_t ws_budget)
{
    const uint64_t per = ((uint64_t)kc + (uint64_t)d + 1u) * 4u;
    uint64_t rows = ws_budget / per;
    const uint64_t cap = ((uint64_t)1 << 30) / ((uint64_t)kc * 4u);
    if (rows > cap) rows = cap;
    if (rows < 1) rows = 1;
    if (rows > (uint64_t)n) rows = (uint64_t)n;
    return (int64_t)rows;
}
// rows the refinement codebooks are trained on
RERANK_HD int64_t train_rows(int64_t n, int64_t ntrain) { return ntrain <= 0 || ntrain > n ? n : ntrain; }

}  // namespace vspq
