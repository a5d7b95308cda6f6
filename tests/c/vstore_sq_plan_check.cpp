// Stand-alone check of csrc/vstore_sq_plan.h: the stride, the range, the code, and every address vstore_sq_range_kernel, vstore_sq_encode_kernel
// and rerank_sq_dist_kernel form, lane by lane, on arrays of exactly the size the store allocates (a wrong index is an AddressSanitizer
// report).  Build with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "../../ivfadc.jl_amd/csrc/vstore_sq_plan.h"

using namespace vssq;   // (rerank:: has a row_offset, a chunks, a tile_base and a MAX_D of its own: its names are taken one by one)
using rerank::WAVE; using rerank::WAVES; using rerank::LOADS; using rerank::TILE_DWORDS; using rerank::gather_row; using rerank::gather_dword;
using rerank::tile_index; using rerank::chunk_byte; using rerank::query_dwords;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static long long g_components = 0, g_shapes = 0;
static uint32_t bits_of(float x) { uint32_t b; memcpy(&b, &x, 4); return b; }

// the three kernels on n rows of d components: every component of every row read exactly once by each
static void check_shape(int d, int64_t n)
{
    const uint32_t s = stride(d), ppr = pieces_per_row(d);
    CHECK(s % PIECE == 0 && s >= (uint32_t)d && s < (uint32_t)d + PIECE && ppr * PIECE == s);
    CHECK(chunks(d) == (d + 127) / 128 && chunk_len(d, chunks(d) - 1) == d - 128 * (chunks(d) - 1) && (chunks(d) == 1 || chunk_len(d, 0) == 128));
    std::vector<float> src((size_t)n * d), arr(d);
    std::vector<uint8_t> store(store_bytes((uint64_t)n, s));
    // range: workgroup (bx, by), lane tid
    std::vector<int> seen((size_t)n * d, 0);
    const int cols = range_cols(d), par = range_rows_par(d);
    const uint32_t gy = range_grid_y(n);
    CHECK(cols * par == RANGE_LANES && (cols >= d || cols == RANGE_LANES) && (cols & (cols - 1)) == 0 && (int64_t)range_grid_x(d) * cols >= d);
    CHECK(gy >= 1 && gy <= RANGE_MAX_GRID_Y && range_row_begin(n, gy, 0) == 0 && range_row_begin(n, gy, gy) == n);
    for (uint32_t bx = 0; bx < range_grid_x(d); ++bx)
        for (uint32_t by = 0; by < gy; ++by)
            for (int tid = 0, t; tid < RANGE_LANES; ++tid)
                for (int64_t r = range_row_begin(n, gy, by) + tid / cols; (t = (int)bx * cols + tid % cols) < d && r < range_row_begin(n, gy, by + 1); r += par)
                    (void)src.at((size_t)r * d + t), ++seen.at((size_t)r * d + t);
    for (int c : seen) CHECK(c == 1);
    // encode: piece e of the block; every output byte written once, every component read once, the arrays inside d
    std::vector<int> wrote(store.size(), 0);
    std::fill(seen.begin(), seen.end(), 0);
    CHECK(encode_pieces(n, d) * PIECE == store.size() && encode_grid(n, d) >= 1 && encode_grid(n, d) <= ENCODE_MAX_GRID);
    CHECK(encode_lds_bytes(d) == (d <= ENCODE_LDS_MAX_D ? (size_t)query_dwords(d) * 8 : 0) && encode_lds_bytes(d) <= ((size_t)32 << 10));
    for (uint64_t e = 0; e < encode_pieces(n, d); ++e) {
        const uint64_t r = piece_row(e, ppr);
        const int t0 = piece_comp(e, ppr);
        CHECK(r < (uint64_t)n && t0 % PIECE == 0 && t0 < d);
        for (int k = 0; k < PIECE; ++k) {
            ++wrote.at(row_offset(r, s) + (uint64_t)t0 + k);
            if (t0 + k < d) { ++seen.at((size_t)r * d + t0 + k); (void)arr.at(t0 + k); }
        }
        if (encode_vec(d, 0) && t0 + PIECE <= d) CHECK((r * (uint64_t)d + t0) % 4 == 0);   // four aligned float4 loads
    }
    for (int c : wrote) CHECK(c == 1);
    for (int c : seen) CHECK(c == 1);
    // distance: LDS, then the fetch and the consumption of every chunk of the wave's 64 rows (the store's last rows: the furthest addresses)
    std::vector<uint32_t> lds(dist_lds_bytes(d) / 4);
    CHECK(dist_lds_bytes(d) <= LDS_MAX && lds.size() == 3u * query_dwords(d) + (size_t)WAVES * TILE_DWORDS);
    CHECK(lo_base(d) % 4 == 0 && step_base(d) % 4 == 0 && tile_base(d, 0) % 4 == 0 && lo_base(d) >= (uint32_t)d && step_base(d) - lo_base(d) >= (uint32_t)d &&
          tile_base(d, 0) - step_base(d) >= (uint32_t)d);
    for (int wv = 0; wv < WAVES; ++wv) (void)lds.at(tile_base(d, wv) + TILE_DWORDS - 1);
    std::vector<int> used((size_t)WAVE * d, 0);
    for (int c = 0; c < chunks(d); ++c) {
        std::vector<int> filled((size_t)TILE_DWORDS, 0), from((size_t)TILE_DWORDS, -1);
        for (int lane = 0; lane < WAVE; ++lane)
            for (int i = 0; i < LOADS; ++i) {
                const int r = gather_row(lane, i);
                const uint64_t v = (uint64_t)(n - 1 - r % n), at = chunk_byte(c, gather_dword(lane, 0));
                if (at < s) { CHECK(at % PIECE == 0 && at + PIECE <= s); (void)store.at(row_offset(v, s) + at + PIECE - 1); }
                for (int k = 0; k < 4; ++k) {
                    ++filled.at(tile_index(r, gather_dword(lane, k)));
                    from.at(tile_index(r, gather_dword(lane, k))) = at < s ? (int)(at / 4) + k : -1;   // dword of the row, or zeros
                }
            }
        for (int r = 0; r < WAVE; ++r)
            for (int t = 0; t < chunk_len(d, c); ++t, ++g_components) {
                const int T = c * CHUNK_ELEMS + t, w = tile_index(r, comp_dword(t));
                CHECK(filled.at(w) == 1 && from.at(w) * 4 + comp_shift(t) / 8 == T && comp_shift(t) < 32);
                if (t % 4 == 0 && t + 4 <= chunk_len(d, c)) CHECK(T % 4 == 0 && T + 3 < (int)query_dwords(d));   // the 16-byte reads of q, lo, step
                ++used.at((size_t)r * d + T);
            }
    }
    for (int c : used) CHECK(c == 1);
    ++g_shapes;
}

int main()
{
    // the range and the code
    const float inf = std::numeric_limits<float>::infinity();
    const float vals[] = {-inf, -3.0e38f, -1.5f, -1.0e-45f, -0.0f, 0.0f, 1.0e-45f, 1.0f, 1.0000001f, 3.0e38f, inf};
    for (size_t i = 0, nv = sizeof(vals) / 4; i < nv; ++i) {
        const uint32_t b = bits_of(vals[i]);
        CHECK(image_bits(image(b)) == b && image(b) > IMAGE_MAX_INIT && image(b) < IMAGE_MIN_INIT && not_finite(b) == (i == 0 || i + 1 == nv));
        if (i) CHECK(image(bits_of(vals[i - 1])) < image(b));
    }
    CHECK(not_finite(bits_of(std::numeric_limits<float>::quiet_NaN())));
    float step, inv;
    range_arrays(0.0f, 255.0f, step, inv);
    CHECK(step == 1.0f && inv == 1.0f);
    range_arrays(0.0f, 510.0f, step, inv);
    CHECK(step == 2.0f && inv == 0.5f);
    range_arrays(3.5f, 3.5f, step, inv);
    CHECK(step == 0.0f && inv == 0.0f && encode(3.5f, 3.5f, inv) == 0 && decode(0, 3.5f, step) == 3.5f);
    for (int c = 0; c < 256; ++c) CHECK(encode((float)c, 0.0f, 1.0f) == (uint32_t)c && decode((uint32_t)c, 0.0f, 1.0f) == (float)c);
    // halves go to the even code; values outside the range clamp
    CHECK(encode(1.0f, 0.0f, 0.5f) == 0 && encode(3.0f, 0.0f, 0.5f) == 2 && encode(5.0f, 0.0f, 0.5f) == 2 && encode(509.0f, 0.0f, 0.5f) == 254);
    CHECK(encode(-7.0f, 0.0f, 0.5f) == 0 && encode(511.0f, 0.0f, 0.5f) == 255 && encode(1.0e30f, 0.0f, 0.5f) == 255 && encode(-3.0e38f, 3.0e38f, 1.0f) == 0);
    // the row and the LDS bound
    CHECK(stride(1) == 16 && stride(16) == 16 && stride(17) == 32 && stride(128) == 128 && stride(129) == 144 && stride(vssq::MAX_D) == (uint32_t)vssq::MAX_D);
    CHECK(dist_lds_bytes(128) == 3 * 512 + 33792 && dist_lds_bytes(vssq::MAX_D) <= LDS_MAX && vssq::MAX_D % PIECE == 0 && vssq::MAX_D <= rerank::MAX_D);
    CHECK(row_offset(((uint64_t)1 << 32) - 1, stride(vssq::MAX_D)) + stride(vssq::MAX_D) == store_bytes((uint64_t)1 << 32, stride(vssq::MAX_D)));
    CHECK(range_cols(1) == 1 && range_cols(10) == 16 && range_cols(128) == 128 && range_cols(129) == 256 && range_cols(vssq::MAX_D) == 256 && range_grid_x(vssq::MAX_D) == 40);
    CHECK(range_grid_y(1) == 1 && range_grid_y(257) == 2 && range_grid_y((int64_t)1 << 32) == 4096 && range_row_begin((int64_t)1 << 32, 4096, 4096) == ((int64_t)1 << 32));
    CHECK(encode_grid(0, 8) == 1 && encode_grid((int64_t)1 << 32, vssq::MAX_D) == ENCODE_MAX_GRID && encode_vec(128, 64) && !encode_vec(10, 64) && !encode_vec(128, 68));
    for (int d = 1; d <= 600; ++d) check_shape(d, d % 7 == 0 ? 300 : 3);
    for (int d : {768, 4096, 4097, vssq::MAX_D}) check_shape(d, 2);
    check_shape(16, 5000), check_shape(10, 4097);
    printf("vstore_sq_plan_check ok: %lld components consumed once, %lld shapes\n", g_components, g_shapes);
    return 0;
}
