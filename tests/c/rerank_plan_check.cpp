// Stand-alone check of csrc/rerank_plan.h: the plan, and every index rerank_dist_kernel and rerank_select_kernel form, restated lane by lane
// in plain C++ on arrays of exactly the caller's size (a wrong index is an AddressSanitizer report).  Build with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ivfadc.jl_amd/csrc/rerank_plan.h"

using namespace rerank;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static uint32_t rnd_state = 12345;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }
static long long g_pairs = 0, g_slices = 0;

// the merge network of the select pass on P keys whose 64-key runs are sorted: must sort
static void check_network(int64_t C)
{
    const int P = padded_keys(C);
    CHECK(P >= WAVE && P >= C && (P & (P - 1)) == 0 && (P == WAVE || P / 2 < C) && select_lds_bytes(C) == (size_t)P * 8);
    std::vector<uint64_t> k((size_t)P, KEY_DEAD);
    for (int64_t i = 0; i < C; ++i) k[(size_t)i] = ((uint64_t)(rnd() % 7) << 32) | (uint64_t)i;
    std::vector<uint64_t> want = k;
    std::sort(want.begin(), want.end());
    for (int r = 0; r < P; r += WAVE) std::sort(k.begin() + r, k.begin() + r + WAVE);
    auto cmpx = [&](int lo, int hi) {
        CHECK(0 <= lo && lo < hi && hi < P);
        if (k.at((size_t)hi) < k.at((size_t)lo)) std::swap(k[(size_t)lo], k[(size_t)hi]);
    };
    for (int w = 128; w <= P; w <<= 1) {
        for (int p = 0; p < P / 2; ++p) { int lo, hi; flip_pair(p, w, lo, hi); CHECK(lo / w == hi / w); cmpx(lo, hi); }
        for (int j = w >> 2; j >= 1; j >>= 1)   // (j < 64: the register tail, the same pairs inside a run)
            for (int p = 0; p < P / 2; ++p) { int lo, hi; stride_pair(p, j, lo, hi); CHECK(j >= 64 || lo / WAVE == hi / WAVE); cmpx(lo, hi); }
    }
    CHECK(k == want);
}

// every index the host loop and rerank_dist_kernel form, on arrays of exactly the caller's size (values are not computed here)
static void simulate(int d, int64_t C, int64_t nq, bool f16, uint64_t budget, int counts_mode)
{
    const uint64_t n = 9;
    const Plan pl = make_plan(nq, C, d, f16, budget);
    CHECK(pl.vec == (row_bytes(d, f16) % 16 == 0) && pl.nchunks == chunks(d, f16) && pl.grid_x * (int64_t)TILE >= C && (pl.grid_x - 1) * (int64_t)TILE < C);
    CHECK(pl.dist_lds == ((size_t)query_dwords(d) + (size_t)WAVES * WAVE * ROW_STRIDE) * 4 && ROW_STRIDE % 2 == 1);
    CHECK(pl.slice_nq >= 1 && pl.slice_nq <= MAX_SLICE_QUERIES && (pl.slice_nq == 1 || (uint64_t)pl.slice_keys * bytes_per_slot(pl.form) <= budget));
    std::vector<uint8_t> rows(store_bytes(n, d, f16)), lds(pl.dist_lds);
    std::vector<float> queries((size_t)nq * d);
    std::vector<uint32_t> ids((size_t)nq * C);
    for (uint32_t &v : ids) v = rnd() % 5 == 0 ? (rnd() % 2 ? (uint32_t)n : 0xFFFFFFFFu) : rnd() % (uint32_t)n;
    std::vector<int32_t> counts((size_t)nq);
    for (int32_t &c : counts) c = counts_mode == 2 ? (int32_t)(rnd() % (2 * C + 3)) - 2 : (int32_t)(rnd() % (C + 1));
    std::vector<int> covered((size_t)nq, 0);
    for (int64_t s = 0; s < pl.nslices; ++s, ++g_slices) {
        const int64_t q0 = slice_begin(pl, s), nqs = slice_queries(pl, s);
        std::vector<int> written((size_t)(nqs * C), 0);
        for (int64_t qy = 0; qy < nqs; ++qy) {
            const int64_t q = q0 + qy, live = live_slots(counts_mode != 0, counts.at((size_t)q), C);
            ++covered.at((size_t)q);
            (void)queries.at(query_row(q, d) + (uint64_t)d - 1);
            (void)lds.at(4 * (size_t)query_dwords(d) - 1);
            for (uint32_t bx = 0; bx < pl.grid_x; ++bx)
                for (int wv = 0; wv < WAVES; ++wv) {
                    uint32_t v[WAVE]; bool ok[WAVE];
                    for (int lane = 0; lane < WAVE; ++lane) {
                        const int64_t j = tile_slot(bx, (uint32_t)(wv * WAVE + lane));
                        ok[lane] = false; v[lane] = 0;
                        if (j < live) { v[lane] = ids.at(id_index(q, C, j)); ok[lane] = v[lane] < n; }
                        if (j < C) { ++written.at(key_index(qy, C, j)); ++g_pairs; }
                    }
                    for (int c = 0; c < pl.nchunks; ++c) {
                        std::vector<int> filled((size_t)TILE_DWORDS, 0);
                        for (int lane = 0; lane < WAVE; ++lane)
                            for (int i = 0; i < LOADS; ++i) {
                                const int r = gather_row(lane, i);
                                const uint64_t b0 = chunk_byte(c, gather_dword(lane, 0)), at = row_offset(v[r], d, f16);
                                // VEC reads 16 bytes when they start inside the row; the scalar form one component at a time
                                if (ok[r] && pl.vec && b0 < row_bytes(d, f16)) (void)rows.at(at + b0 + 15);
                                for (uint64_t e = 0; ok[r] && !pl.vec && e < 16; e += elem_bytes(f16))
                                    if (b0 + e < row_bytes(d, f16)) (void)rows.at(at + b0 + e + elem_bytes(f16) - 1);
                                for (int k = 0; k < 4; ++k) {
                                    (void)lds.at(4 * (size_t)(tile_base(d, wv) + tile_index(r, gather_dword(lane, k))) + 3);
                                    ++filled.at(tile_index(r, gather_dword(lane, k)));
                                }
                            }
                        for (int r = 0; r < WAVE; ++r)
                            for (int dw = 0; dw < CHUNK_DWORDS; ++dw) CHECK(filled[tile_index(r, dw)] == 1);
                        const int len = chunk_len(d, f16, c);   // what lane r consumes: its tile row and the query chunk
                        CHECK(len >= 1 && len <= chunk_elems(f16) && c * chunk_elems(f16) + len <= d && (f16 ? (len + 1) / 2 : len) <= CHUNK_DWORDS);
                    }
                }
        }
        for (int w : written) CHECK(w == 1);
    }
    for (int c : covered) CHECK(c == 1);
}

int main()
{
    const int CASE_D[] = {1, 3, 10, 32, 33, 64, 65, 100, 128};
    const int64_t CASE_C[] = {1, 63, 64, 65, 255, 256, 257, 600};
    const int64_t CASE_NQ[] = {1, 3, 40};
    for (int d : CASE_D)
        for (int64_t C : CASE_C)
            for (int64_t nq : CASE_NQ)
                for (int f16 = 0; f16 < 2; ++f16)
                    simulate(d, C, nq, f16 != 0, nq == 40 ? (uint64_t)C * 8 * 7 : (uint64_t)8 << 30, (int)((d + C + nq) % 3));
    for (int64_t C = 1; C <= SELECT_LDS_MAX; C = C < 70 ? C + 1 : C * 2 - 3) check_network(C);
    check_network(SELECT_LDS_MAX);
    CHECK(select_form(SELECT_LDS_MAX) == SELECT_LDS && select_form(SELECT_LDS_MAX + 1) == SELECT_SORT && select_lds_bytes(SELECT_LDS_MAX + 1) == 0);
    // the 2^31 edge: what fits, and plans at the edge (slices cover the queries once; 64-bit indices)
    CHECK(pairs_fit(MAX_PAIRS, 1) && pairs_fit(1, MAX_PAIRS) && pairs_fit(46340, 46341) && !pairs_fit(46341, 46341) && !pairs_fit(MAX_PAIRS, 2));
    CHECK(!pairs_fit((int64_t)1 << 31, 1) && !pairs_fit(1, (int64_t)1 << 31) && pairs_fit(0, (int64_t)1 << 40));
    const int64_t EDGE[][2] = {{MAX_PAIRS, 1}, {1, MAX_PAIRS}, {46340, 46341}, {65535, 32767}, {65536, 32767}, {1000000, 2147}};
    for (const auto &e : EDGE)
        for (uint64_t budget : {(uint64_t)1 << 20, (uint64_t)8 << 30, ~(uint64_t)0})
            for (int d : {1, 10, 128, MAX_D}) {
                const Plan pl = make_plan(e[0], e[1], d, d == 10, budget);
                CHECK(pl.slice_nq >= 1 && pl.slice_nq <= MAX_SLICE_QUERIES && pl.nslices >= 1);
                CHECK(slice_begin(pl, pl.nslices - 1) < e[0] && slice_begin(pl, pl.nslices - 1) + slice_queries(pl, pl.nslices - 1) == e[0]);
                CHECK(pl.slice_keys <= MAX_PAIRS && key_index(pl.slice_nq - 1, e[1], e[1] - 1) == (uint64_t)pl.slice_keys - 1);
                CHECK(id_index(e[0] - 1, e[1], e[1] - 1) == (uint64_t)e[0] * (uint64_t)e[1] - 1);
                CHECK((int64_t)pl.grid_x * TILE >= e[1] && pl.dist_lds <= (size_t)160 << 10);
            }
    CHECK(row_offset(((uint64_t)1 << 32) - 1, MAX_D, false) + row_bytes(MAX_D, false) == store_bytes((uint64_t)1 << 32, MAX_D, false));
    printf("rerank_plan_check ok: %lld pairs written once, %lld slices\n", g_pairs, g_slices);
    return 0;
}
