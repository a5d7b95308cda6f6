// Stand-alone check of csrc/vstore_pq_plan.h: the record and every address rerank_pq_dist_kernel forms, lane by lane, on arrays of exactly
// the size the store allocates (a wrong index is an AddressSanitizer report).  Build with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../ivfadc.jl_amd/csrc/vstore_pq_plan.h"

using namespace rerank;
using namespace vspq;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static long long g_components = 0, g_shapes = 0;
static void check_record(int m, int m2)
{
    CHECK(record_fits(m, m2));
    const uint32_t s = stride(m, m2), raw = raw_bytes(m, m2);
    CHECK(s >= MIN_STRIDE && s <= MAX_RECORD && (s & (s - 1)) == 0 && raw <= s && (s == MIN_STRIDE || s / 2 < raw));
    CHECK(off_list() == 0 && off_code(0) == 4 && off_code(m - 1) + 1 == off_code2(m, 0) && off_code2(m, m2 - 1) + 1 == raw);
    for (uint64_t v : {(uint64_t)0, (uint64_t)1, (uint64_t)77, ((uint64_t)1 << 32) - 1})
        CHECK(record_offset(v, s) / 128 == (record_offset(v, s) + s - 1) / 128 && record_offset(v, s) + s <= store_bytes(v + 1, s));
    // no record straddles a 128-byte line; the fetch reads every byte of the 64 records once, in aligned pieces, every lane as often
    const uint32_t pb = piece_bytes(s), np = pieces(s);
    CHECK((pb == 16 || pb == 4) && s % pb == 0 && np % WAVE == 0 && (uint64_t)np * pb == (uint64_t)WAVE * s);
    std::vector<int> seen((size_t)WAVE * s, 0);
    for (uint32_t i = 0; i < np; ++i) {
        const int r = piece_row(i, s);
        const uint32_t at = piece_byte(i, s);
        CHECK(r >= 0 && r < WAVE && at % pb == 0 && at + pb <= s);
        for (uint32_t b = 0; b < pb; ++b) ++seen.at((size_t)r * s + at + b);
    }
    for (int c : seen) CHECK(c == 1);
}

// the reconstruction of every chunk of 64 rows: each component of each row once, every operand inside its centroid row and its codeword
static void check_reconstruct(int d, int m, int m2, int ksub, int k2, int kc)
{
    const int dsub = d / m, dsub2 = d / m2;
    const bool vec = vec4(d, m, m2);
    CHECK(vec == (dsub % 4 == 0 && dsub2 % 4 == 0));
    const uint32_t s = stride(m, m2);
    std::vector<float> cent((size_t)kc * d), books((size_t)m * ksub * dsub), refine((size_t)m2 * k2 * dsub2);
    std::vector<uint8_t> lds(vspq::dist_lds_bytes(d, s));
    CHECK(lds.size() <= ((size_t)160 << 10) && lds.size() == rerank::dist_lds_bytes(d) + (size_t)WAVES * WAVE * s);
    for (int wv = 0; wv < WAVES; ++wv) CHECK(record_base(d, wv, s) % 4 == 0 && 4 * (size_t)record_base(d, wv, s) + (size_t)WAVE * s <= lds.size());
    CHECK(record_base(d, 0, s) == tile_base(d, WAVES - 1) + TILE_DWORDS);
    const uint32_t list = (uint32_t)kc - 1, c1 = (uint32_t)ksub - 1, c2 = (uint32_t)k2 - 1;   // the last of each: the furthest addresses
    for (int c = 0; c < chunks(d, false); ++c) {
        std::vector<int> filled((size_t)TILE_DWORDS, 0);
        for (int lane = 0; lane < WAVE; ++lane) {
            const int t0 = chunk_comp(c, gather_dword(lane, 0));
            for (int i = 0; i < LOADS; ++i) {
                const int r = gather_row(lane, i);
                for (int k = 0; k < 4; ++k) ++filled.at(tile_index(r, gather_dword(lane, k)));
                if (t0 >= d) continue;
                if (vec) {   // three 16-byte pieces, aligned, each inside one row / one codeword
                    const int j1 = sub_of(t0, dsub), a1 = sub_at(t0, dsub), j2 = sub_of(t0, dsub2), a2 = sub_at(t0, dsub2);
                    CHECK(t0 + 3 < d && a1 + 3 < dsub && a2 + 3 < dsub2 && j1 < m && j2 < m2);
                    CHECK(centroid_elem(list, d, t0) % 4 == 0 && codeword_elem(j1, c1, a1, dsub, ksub) % 4 == 0 && codeword_elem(j2, c2, a2, dsub2, k2) % 4 == 0);
                    (void)cent.at(centroid_elem(list, d, t0) + 3);
                    (void)books.at(codeword_elem(j1, c1, a1, dsub, ksub) + 3);
                    (void)refine.at(codeword_elem(j2, c2, a2, dsub2, k2) + 3);
                    g_components += 4;
                } else {
                    for (int k = 0; k < 4 && t0 + k < d; ++k, ++g_components) {
                        const int t = t0 + k, j1 = sub_of(t, dsub), j2 = sub_of(t, dsub2);
                        CHECK(j1 < m && j2 < m2 && off_code(j1) < off_code2(m, 0) && off_code2(m, j2) < raw_bytes(m, m2));
                        (void)cent.at(centroid_elem(list, d, t));
                        (void)books.at(codeword_elem(j1, c1, sub_at(t, dsub), dsub, ksub));
                        (void)refine.at(codeword_elem(j2, c2, sub_at(t, dsub2), dsub2, k2));
                    }
                }
            }
        }
        for (int e = 0; e < WAVE * CHUNK_DWORDS; ++e) CHECK(filled[tile_index(e / CHUNK_DWORDS, e % CHUNK_DWORDS)] == 1);
    }
    ++g_shapes;
    // the staged route: the copy writes every piece of both slices once, from inside its codeword, and a lane's reads stay inside the slices
    CHECK(staged_fits(d, m, m2, ksub, k2) == (vec && staged_lds_bytes(d, s, ksub, k2) <= STAGED_LDS_MAX));
    if (!vec) return;
    CHECK(slice_base(d, s) % 4 == 0 && (size_t)slice_base(d, s) * 4 == lds.size() && staged_lds_bytes(d, s, ksub, k2) == lds.size() + 128u * (ksub + k2));
    for (int c = 0; c < chunks(d, false); ++c) {
        std::vector<int> w(slice_dwords(ksub) + slice_dwords(k2), 0);   // both slices, the refinement's behind the base's
        for (uint32_t e = 0; e < slice_pieces(ksub) + slice_pieces(k2); ++e) {
            const bool base = e < slice_pieces(ksub);
            const uint32_t f = base ? e : e - slice_pieces(ksub), code = slice_code(f);
            const int g = slice_g(f), t0 = chunk_comp(c, 4 * g), ds = base ? dsub : dsub2, k = base ? ksub : k2;
            CHECK(code < (uint32_t)k && g < SLICE_PIECES && slice_piece(code, g) % 4 == 0);
            for (int x = 0; x < 4; ++x) ++w.at((base ? 0u : slice_dwords(ksub)) + slice_piece(code, g) + x);
            if (t0 >= d) continue;
            CHECK(sub_at(t0, ds) + 3 < ds && codeword_elem(sub_of(t0, ds), code, sub_at(t0, ds), ds, k) % 4 == 0);
            (void)(base ? books : refine).at(codeword_elem(sub_of(t0, ds), code, sub_at(t0, ds), ds, k) + 3);
        }
        for (int x : w) CHECK(x == 1);
        for (int lane = 0; lane < WAVE; ++lane)   // a lane reads the piece filled for its four components (g = its dword / 4)
            CHECK(gather_dword(lane, 0) % 4 == 0 && slice_piece(c1, gather_dword(lane, 0) / 4) + 3 < slice_dwords(ksub) && slice_piece(c2, gather_dword(lane, 0) / 4) + 3 < slice_dwords(k2));
    }
}

int main()
{
    for (int m = 1; m <= 123; ++m)
        for (int m2 = 1; m + m2 <= 124; ++m2) check_record(m, m2);
    CHECK(!record_fits(64, 61) && !record_fits(0, 4) && !record_fits(4, 0) && record_fits(62, 62));
    CHECK(stride(1, 1) == 8 && stride(8, 8) == 32 && stride(8, 16) == 32 && stride(16, 8) == 32 && stride(8, 2) == 16 && stride(2, 5) == 16 && stride(62, 62) == 128);
    const int PAIRS[][3] = {{6, 1, 1}, {10, 2, 5}, {32, 8, 8}, {32, 8, 2}, {96, 16, 8}, {128, 8, 16}};
    for (int d = 1; d <= 1024; ++d)   // every d, under the pairs above that divide it and under its finest and coarsest split
        for (const auto &p : PAIRS) {
            if (d % p[1] == 0 && d % p[2] == 0) check_reconstruct(d, p[1], p[2], 7, 3, 2);
            if (d <= 62 && &p == &PAIRS[0]) check_reconstruct(d, d, d, 2, 2, 1);
        }
    check_reconstruct(144, 2, 4, 256, 256, 2), check_reconstruct(128, 8, 16, 256, 256, 2);
    CHECK(staged_lds_bytes(128, 32, 256, 256) == 512 + 33792 + 8192 + 65536 && staged_fits(128, 8, 16, 256, 256) && !staged_fits(96, 16, 8, 256, 256) &&
          staged_fits(12288, 8, 16, 256, 256) && !staged_fits(MAX_D, 8, 16, 256, 256));   // the query itself takes d x 4 bytes of the 160 KB
    CHECK(vspq::dist_lds_bytes(MAX_D, MAX_RECORD) <= ((size_t)160 << 10) && block_rows(1000, 128, 1000, (uint64_t)8 << 30) == 1000 && block_rows(1000, 128, 1000, 1) == 1 && block_rows(5, 4, 2, 100) == 3);
    CHECK(block_rows((int64_t)1 << 32, 128, 1 << 20, ~(uint64_t)0) == 256 && encode_lds_bytes(10, 2, 5) == 48 + 56 && train_rows(10, 0) == 10 && train_rows(10, 4) == 4);
    printf("vstore_pq_plan_check ok: %lld components reconstructed once, %lld shapes\n", g_components, g_shapes);
    return 0;
}
