// Row layout, range arithmetic and index arithmetic of the 8-bit scalar-quantised vector store (store_type 3: ivfadc_vectors_create_sq,
// re-ranked by rerank_sq_dist_kernel in rerank.hip.h).  Plain C++ (no HIP types), a sibling of rerank_plan.h and vstore_pq_plan.h, so that
// the stride, the range, the code and every address the three kernels form compile and run without a GPU (tests/c/vstore_sq_plan_check.cpp).
//
// Row v of the store is d CODES of one byte, component t at byte t, then zero padding up to the stride: d rounded up to 16 bytes.  Every
// fetch is then an aligned 16-byte load that stays inside its row, and a d = 128 row is exactly one 128-byte line.  Beside the rows the
// store owns three Float32 arrays of d entries, computed on the HOST in plain float arithmetic (the device never divides):
//   lo[t];  step[t] = (hi[t] - lo[t]) / 255;  inv[t] = 255 / (hi[t] - lo[t]);  a range of 0 gives step = inv = 0.
// Code of x:          c = min(255, max(0, rintf((x - lo[t]) * inv[t]))), round-half-to-even.
// Reconstruction:     y = lo[t] + (float)c * step[t], one rounding per operation, nothing contracted.
//
// vstore_sq_range_kernel: a workgroup of RANGE_LANES lanes is range_cols(d) columns wide and range_rows_par(d) rows deep; consecutive lanes
// sit on consecutive columns of a row.  Workgroup (bx, by) walks rows range_row_begin(by) .. of columns bx * cols ..; the minimum and the
// maximum travel as ORDER-PRESERVING unsigned images of the floats (image()), so an atomic min / max on them is exact and the result is
// the same for any grid and any arrival order.
// vstore_sq_encode_kernel: one lane per PIECE of 16 output bytes; piece e of a block of rows is piece e % pieces_per_row of row
// e / pieces_per_row.  lo / inv sit in LDS up to ENCODE_LDS_MAX_D components and are read through the L2 above it.
// rerank_sq_dist_kernel keeps rerank_dist_kernel's decomposition (rerank_plan.h): the same gather, the same [row][dword] tile -- but a
// chunk, one 128-byte line of a row, is now CHUNK_ELEMS = 128 components, and dword w of a tile row holds components 4w .. 4w + 3.
// LDS of a workgroup: the query, lo and step, each d floats rounded up to four, then one tile per wave.
//
// Nothing here has been measured against an alternative.  The constants below are REASONED, NOT MEASURED.
#pragma once

#include <cmath>

#include "rerank_plan.h"

namespace vssq {

constexpr int STORE_SQ = 3;                          // store_type
constexpr int CHUNK_ELEMS = rerank::CHUNK_BYTES;     // 128 codes: one line of a row
constexpr int PIECE = 16;                            // bytes of a fetch and of an encoder lane's store
constexpr size_t LDS_MAX = (size_t)160 << 10;        // the LDS of a CU
// the longest vector the store takes: the query, lo and step stand whole in LDS beside the tiles -- 3 x 40 KB + 33 KB = 153 KB of the
// 160 KB of a CU, one workgroup per CU at that length.  (REASONED, NOT MEASURED: the largest round d that fits, not a tuned one)
constexpr int MAX_D = 10240;

// ---- the row --------------------------------------------------------------------------------------------------------------------------------
RERANK_HD uint32_t stride(int d) { return ((uint32_t)d + (uint32_t)PIECE - 1u) & ~((uint32_t)PIECE - 1u); }
RERANK_HD uint32_t pieces_per_row(int d) { return stride(d) / (uint32_t)PIECE; }
RERANK_HD uint64_t row_offset(uint64_t v, uint32_t stride) { return v * (uint64_t)stride; }     // v < n <= 2^32
RERANK_HD uint64_t store_bytes(uint64_t n, uint32_t stride) { return n * (uint64_t)stride; }
RERANK_HD int chunks(int d) { return (d + CHUNK_ELEMS - 1) / CHUNK_ELEMS; }
RERANK_HD int chunk_len(int d, int c)
{
    const int left = d - c * CHUNK_ELEMS;
    return left < CHUNK_ELEMS ? left : CHUNK_ELEMS;
}
// component t of a tile row: dword and byte in it
RERANK_HD int comp_dword(int t) { return t >> 2; }
RERANK_HD int comp_shift(int t) { return 8 * (t & 3); }

// ---- the range and the code -------------------------------------------------------------------------------------------------------------------
// lo <= hi, both finite, hi - lo finite (the entries refuse anything else)
inline void range_arrays(float lo, float hi, float &step, float &inv)
{
    const float range = hi - lo;
    step = range == 0.0f ? 0.0f : range / 255.0f;
    inv = range == 0.0f ? 0.0f : 255.0f / range;
}
RERANK_HD uint32_t encode(float x, float lo, float inv) { return (uint32_t)fminf(255.0f, fmaxf(0.0f, rintf((x - lo) * inv))); }
RERANK_HD float decode(uint32_t c, float lo, float step) { return lo + (float)c * step; }
// a < b as floats <=> image(a) < image(b) as unsigned (neither a NaN; -0 stands below +0)
RERANK_HD uint32_t image(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
RERANK_HD uint32_t image_bits(uint32_t img) { return (img & 0x80000000u) ? img & 0x7FFFFFFFu : ~img; }
constexpr uint32_t IMAGE_MIN_INIT = 0xFFFFFFFFu, IMAGE_MAX_INIT = 0u;
RERANK_HD bool not_finite(uint32_t bits) { return (bits & 0x7F800000u) == 0x7F800000u; }

// ---- vstore_sq_range_kernel ---------------------------------------------------------------------------------------------------------------------
constexpr int RANGE_LANES = 256;
constexpr int64_t RANGE_MAX_GRID_Y = 4096;
constexpr int64_t RANGE_MIN_ROWS = 256;              // rows a workgroup walks at least, so that its atomics are few beside its reads
RERANK_HD int range_cols(int d)                      // the power of two at or above d, at most the workgroup
{
    int c = 1;
    while (c < d && c < RANGE_LANES) c <<= 1;
    return c;
}
RERANK_HD int range_rows_par(int d) { return RANGE_LANES / range_cols(d); }
RERANK_HD uint32_t range_grid_x(int d) { return (uint32_t)((d + range_cols(d) - 1) / range_cols(d)); }
RERANK_HD uint32_t range_grid_y(int64_t rows)
{
    const int64_t g = (rows + RANGE_MIN_ROWS - 1) / RANGE_MIN_ROWS;
    return (uint32_t)(g < 1 ? 1 : g > RANGE_MAX_GRID_Y ? RANGE_MAX_GRID_Y : g);
}
RERANK_HD int64_t range_rows_per_group(int64_t rows, uint32_t grid_y) { return (rows + (int64_t)grid_y - 1) / (int64_t)grid_y; }
RERANK_HD int64_t range_row_begin(int64_t rows, uint32_t grid_y, uint32_t by)
{
    const int64_t b = (int64_t)by * range_rows_per_group(rows, grid_y);
    return b < rows ? b : rows;
}

// ---- vstore_sq_encode_kernel --------------------------------------------------------------------------------------------------------------------
constexpr int ENCODE_LANES = 256;
// lo and inv in LDS: 2 x 16 KB at most.  A workgroup's turn encodes 4096 components; above this d its copy of the two arrays would read
// more than twice what it encodes per turn, and the L2 serves them as well.
constexpr int ENCODE_LDS_MAX_D = 4096;
constexpr int64_t ENCODE_MAX_GRID = 65536;
RERANK_HD bool encode_in_lds(int d) { return d <= ENCODE_LDS_MAX_D; }
RERANK_HD size_t encode_lds_bytes(int d) { return encode_in_lds(d) ? (size_t)rerank::query_dwords(d) * 8 : 0; }
RERANK_HD uint64_t encode_pieces(int64_t rows, int d) { return (uint64_t)rows * pieces_per_row(d); }
RERANK_HD uint32_t encode_grid(int64_t rows, int d)
{
    const uint64_t g = (encode_pieces(rows, d) + ENCODE_LANES - 1) / ENCODE_LANES;
    return (uint32_t)(g < 1 ? 1 : g > (uint64_t)ENCODE_MAX_GRID ? (uint64_t)ENCODE_MAX_GRID : g);
}
RERANK_HD uint64_t piece_row(uint64_t e, uint32_t ppr) { return e / ppr; }
RERANK_HD int piece_comp(uint64_t e, uint32_t ppr) { return (int)(e % ppr) * PIECE; }          // first component of the piece
// four float4 loads serve a piece whose 16 components all exist, in a source whose rows keep 16-byte alignment
RERANK_HD bool encode_vec(int d, uint64_t src_address) { return d % 4 == 0 && src_address % 16 == 0; }

// ---- LDS of the distance pass, in dwords ----------------------------------------------------------------------------------------------------
RERANK_HD uint32_t lo_base(int d) { return rerank::query_dwords(d); }
RERANK_HD uint32_t step_base(int d) { return 2u * rerank::query_dwords(d); }
RERANK_HD uint32_t tile_base(int d, int wave) { return 3u * rerank::query_dwords(d) + (uint32_t)wave * rerank::TILE_DWORDS; }
RERANK_HD size_t dist_lds_bytes(int d) { return (size_t)tile_base(d, rerank::WAVES) * 4; }

}  // namespace vssq
