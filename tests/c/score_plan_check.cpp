// Stand-alone check of csrc/score_plan.h and of the pair and row addressing score_pairs_kernel (csrc/score.hip.h) builds on it, on the CPU
// (tests/test_score_plan.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer and runs it as a child process).
//
// sim_call restates the host entry's loop over the slices and the kernel lane by lane -- grid (tiles, queries of the slice), TILE lanes,
// the query into LDS, the slot of a lane, live / dead by counts, the located (list, position) at loc_index, the centre row twice, the code
// row, the codewords, 16 bytes at a time where centre_vec4 / codeword_vec4 allow -- over arrays that are std::vectors of exactly the size
// the caller and the runtime allocate, so an index the arithmetic gets wrong is an AddressSanitizer report.  Every pair must be written
// exactly once, a dead or absent slot must read nothing of the index, and the distance the restated addressing gathers must be the one a
// plain triple loop over [list][t] and [sub-space][codeword][k] computes.
#include "../../ivfadc.jl_amd/csrc/score_plan.h"

#include "../../ivfadc.jl_amd/csrc/reconstruct_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace score;

static const int64_t CASE_C[] = {1, 63, 64, 65, 255, 256, 257};
static const int64_t CASE_NQ[] = {1, 3, 1000};

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

struct Index {
    int d, m, dsub, ksub, cs, kc, bytes;   // bytes: of one code (1 or 2)
    std::vector<float> centroids, codebooks;
    std::vector<uint8_t> label_inv;        // [m][256], 8-bit only
    std::vector<int64_t> len, codeoff;
    std::vector<uint8_t> codes;            // cs-strided rows, nothing behind the last list's capacity
};

static Index make_index(int d, int m, int ksub, int bytes, int kc, std::mt19937 &rng)
{
    Index ix;
    ix.d = d; ix.m = m; ix.dsub = d / m; ix.ksub = ksub; ix.kc = kc; ix.bytes = bytes;
    ix.cs = (m * bytes + 3) / 4 * 4;
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    ix.centroids.resize((size_t)kc * d);
    ix.codebooks.resize((size_t)m * ksub * ix.dsub);
    for (float &x : ix.centroids) x = u(rng);
    for (float &x : ix.codebooks) x = u(rng);
    if (bytes == 1) {
        ix.label_inv.resize((size_t)m * 256);
        for (uint8_t &x : ix.label_inv) x = (uint8_t)(rng() % (unsigned)std::min(ksub, 256));
    }
    int64_t off = 0;
    for (int l = 0; l < kc; ++l) {
        ix.len.push_back((int64_t)(rng() % 40));
        ix.codeoff.push_back(off);
        off += ix.len.back() * ix.cs;
    }
    ix.codes.resize((size_t)off);
    for (uint8_t &x : ix.codes) x = (uint8_t)rng();       // (16-bit codes beyond ksub: the clamp is exercised)
    return ix;
}

// the codeword index the kernel forms from a code row
static uint32_t codeword_of(const Index &ix, const uint8_t *row, uint32_t ii)
{
    uint32_t c;
    if (ix.bytes == 1) c = ix.label_inv[recon::label_slot(ii, row[ii])];
    else c = (uint32_t)row[2 * ii] | ((uint32_t)row[2 * ii + 1] << 8);
    return c < (uint32_t)ix.ksub ? c : (uint32_t)ix.ksub - 1u;
}

static float step(float acc, float x, float y)
{
    const float u = x - y;
    return acc + u * u;
}

// score_pair of score.hip.h, pointer for pointer
static float sim_pair(const Index &ix, const float *qs, int32_t l, int64_t p)
{
    const float *centre = ix.centroids.data() + (size_t)l * ix.d;
    const uint8_t *row = ix.codes.data() + recon::code_row((uint64_t)ix.codeoff[l], (uint64_t)p, (uint32_t)ix.cs);
    float dc = 0.0f;
    if (centre_vec4(ix.d)) {
        for (int t = 0; t < ix.d; t += 4) {
            CHECK(((size_t)l * ix.d + t) % 4 == 0);
            float c4[4], q4[4];
            std::memcpy(c4, centre + t, 16);
            std::memcpy(q4, qs + t, 16);
            for (int k = 0; k < 4; ++k) dc = step(dc, c4[k], q4[k]);
        }
    } else {
        for (int t = 0; t < ix.d; ++t) dc = step(dc, centre[t], qs[t]);
    }
    float dist = dc;
    for (uint32_t ii = 0; ii < (uint32_t)ix.m; ++ii) {
        const uint32_t c = codeword_of(ix, row, ii);
        const uint32_t t0 = ii * (uint32_t)ix.dsub;
        const uint64_t e0 = recon::codeword_elem(ii, c, t0, (uint32_t)ix.dsub, (uint32_t)ix.ksub);
        const float *cw = ix.codebooks.data() + e0;
        float s = 0.0f;
        if (codeword_vec4(ix.dsub)) {
            for (int k = 0; k < ix.dsub; k += 4) {
                CHECK((e0 + k) % 4 == 0 && ((size_t)l * ix.d + t0 + k) % 4 == 0 && (t0 + k) % 4 == 0);
                float w4[4], c4[4], q4[4];
                std::memcpy(w4, cw + k, 16);
                std::memcpy(c4, centre + t0 + k, 16);
                std::memcpy(q4, qs + t0 + k, 16);
                for (int j = 0; j < 4; ++j) s = step(s, w4[j], q4[j] - c4[j]);
            }
        } else {
            for (int k = 0; k < ix.dsub; ++k) s = step(s, cw[k], qs[t0 + k] - centre[t0 + k]);
        }
        dist = dist + s;
    }
    return dist;
}

// the four lines of the contract over plain [list][t] and [ii][c][k] indexing
static float plain_pair(const Index &ix, const float *q, int32_t l, int64_t p)
{
    float dc = 0.0f;
    for (int t = 0; t < ix.d; ++t) dc = step(dc, ix.centroids[(size_t)l * ix.d + t], q[t]);
    float dist = dc;
    for (int ii = 0; ii < ix.m; ++ii) {
        const uint8_t *row = &ix.codes[(size_t)(ix.codeoff[l] + p * ix.cs)];
        const uint32_t c = codeword_of(ix, row, (uint32_t)ii);
        float s = 0.0f;
        for (int k = 0; k < ix.dsub; ++k) {
            const int t = ii * ix.dsub + k;
            const float r = q[t] - ix.centroids[(size_t)l * ix.d + t];
            s = step(s, ix.codebooks[((size_t)ii * ix.ksub + c) * ix.dsub + k], r);
        }
        dist = dist + s;
    }
    return dist;
}

static uint64_t g_pairs = 0, g_live = 0, g_slices = 0;

// counts_mode: 0 none, 1 ragged in [0, C] (zeros included), 2 outside [0, C] as well (the device entry clamps)
static void sim_call(const Index &ix, int64_t nq, int64_t C, bool shared, int counts_mode, uint64_t ws_budget, std::mt19937 &rng)
{
    const int64_t stride = shared ? 0 : C;
    CHECK(stride_form(C, stride) == (shared ? FORM_SHARED : FORM_PER_QUERY) && pairs_fit(nq, C));
    const Plan pl = make_plan(nq, C, stride, ix.d, ws_budget);
    CHECK(pl.nslices >= 1 && pl.slice_nq >= 1 && pl.slice_nq <= MAX_SLICE_QUERIES && (int64_t)pl.grid_x * TILE >= C && ((int64_t)pl.grid_x - 1) * TILE < C);
    CHECK(pl.lds == (size_t)ix.d * 4);
    if (!shared && pl.slice_nq > 1) CHECK((uint64_t)pl.locate_slots * LOCATE_BYTES_PER_SLOT <= ws_budget);
    if (!shared && pl.nslices > 1) CHECK((uint64_t)(pl.slice_nq + 1) * (uint64_t)C * LOCATE_BYTES_PER_SLOT > ws_budget || pl.slice_nq == MAX_SLICE_QUERIES);
    std::vector<float> queries((size_t)nq * ix.d);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    for (float &x : queries) x = u(rng);
    // an "id" here is a (list, position) the stand-in locate decodes, or an absent one
    std::vector<uint32_t> ids((size_t)(shared ? C : nq * C));
    for (uint32_t &v : ids) v = (uint32_t)rng();
    std::vector<int32_t> counts;
    if (counts_mode) {
        counts.resize((size_t)nq);
        for (int64_t q = 0; q < nq; ++q) {
            const int pick = (int)(rng() % 6);
            counts[(size_t)q] = pick == 0 ? 0 : pick == 1 ? (int32_t)C : (int32_t)(rng() % (uint64_t)(C + 1));
            if (counts_mode == 2 && pick == 2) counts[(size_t)q] = -(int32_t)(rng() % 5) - 1;
            if (counts_mode == 2 && pick == 3) counts[(size_t)q] = (int32_t)C + 1 + (int32_t)(rng() % 5);
        }
    }
    auto locate = [&](uint32_t v, int32_t &l, int64_t &p) {
        l = -1; p = -1;
        if (v % 5 == 0) return;                                        // absent
        const int32_t cand = (int32_t)((v >> 8) % (uint32_t)ix.kc);
        if (ix.len[(size_t)cand] == 0) return;
        l = cand;
        p = (int64_t)((v >> 16) % (uint64_t)ix.len[(size_t)cand]);
    };
    std::vector<float> out((size_t)(nq * C), -1.0f);
    std::vector<uint8_t> found((size_t)(nq * C), 7);
    std::vector<uint8_t> visits((size_t)(nq * C), 0);
    std::vector<int32_t> loc_list((size_t)pl.locate_slots);
    std::vector<int64_t> loc_pos((size_t)pl.locate_slots);
    if (pl.shared)
        for (int64_t j = 0; j < C; ++j) locate(ids[(size_t)j], loc_list[(size_t)j], loc_pos[(size_t)j]);
    int64_t covered = 0;
    for (int64_t s = 0; s < pl.nslices; ++s) {
        const int64_t q0 = slice_begin(pl, s), nqs = slice_queries(pl, s);
        CHECK(q0 == covered && nqs >= 1 && nqs <= pl.slice_nq);
        covered += nqs;
        ++g_slices;
        if (!pl.shared) {
            const uint32_t *src = ids.data() + id_index(q0, stride, 0);
            std::fill(loc_list.begin(), loc_list.end(), -2);          // (what an earlier slice left is not this slice's)
            for (int64_t j = 0; j < nqs * C; ++j) locate(src[j], loc_list[(size_t)j], loc_pos[(size_t)j]);
        }
        for (int64_t by = 0; by < nqs; ++by)
            for (uint32_t bx = 0; bx < pl.grid_x; ++bx) {
                const int64_t q = q0 + by;
                std::vector<float> lds(pl.lds / 4);
                const float *qrow = queries.data() + query_row(q, ix.d);
                for (int lane = 0; lane < TILE; ++lane)
                    for (int t = lane; t < ix.d; t += TILE) lds[(size_t)t] = qrow[t];
                for (uint32_t lane = 0; lane < (uint32_t)TILE; ++lane) {
                    const int64_t j = tile_slot(bx, lane);
                    if (j >= C) continue;
                    float dist = INFINITY;
                    uint8_t f = 0;
                    if (j < live_slots(counts_mode != 0, counts_mode ? counts[(size_t)q] : 0, C)) {
                        const uint64_t li = loc_index(pl.shared, by, C, j);
                        const int32_t l = loc_list[(size_t)li];
                        const int64_t p = loc_pos[(size_t)li];
                        CHECK(l != -2);
                        if (l >= 0 && l < ix.kc && p >= 0) {
                            dist = sim_pair(ix, lds.data(), l, p);
                            f = 1;
                            ++g_live;
                        }
                    }
                    const uint64_t pair = pair_index(q, C, j);
                    out[(size_t)pair] = dist;
                    found[(size_t)pair] = f;
                    ++visits[(size_t)pair];
                }
            }
    }
    CHECK(covered == nq);
    // every pair once, and what the definition says
    for (int64_t q = 0; q < nq; ++q) {
        int64_t live = C;
        if (counts_mode) live = std::min<int64_t>(std::max<int64_t>(counts[(size_t)q], 0), C);
        for (int64_t j = 0; j < C; ++j) {
            const size_t pair = (size_t)(q * C + j);
            CHECK(visits[pair] == 1);
            int32_t l = -1;
            int64_t p = -1;
            if (j < live) locate(ids[(size_t)(shared ? j : q * C + j)], l, p);
            if (l < 0) {
                CHECK(found[pair] == 0 && std::isinf(out[pair]) && out[pair] > 0);
            } else {
                const float want = plain_pair(ix, queries.data() + (size_t)q * ix.d, l, p);
                CHECK(found[pair] == 1 && std::memcmp(&want, &out[pair], 4) == 0);
            }
            ++g_pairs;
        }
    }
}

static int plan_cases()
{
    int n = 0;
    // pair counts on both sides of 2^31 - 1
    const int64_t fits[][2] = {{MAX_PAIRS, 1}, {1, MAX_PAIRS}, {46340, 46341}, {65536, 32767}, {2, 1073741823}, {0, 1ll << 40}, {1ll << 40, 0}};
    const int64_t too_many[][2] = {{MAX_PAIRS + 1, 1}, {1, MAX_PAIRS + 1}, {46341, 46341}, {65536, 32768}, {2, 1073741824}, {1ll << 40, 1ll << 40},
                                   {INT64_MAX, 2}, {3, INT64_MAX}};
    for (auto &c : fits) { CHECK(pairs_fit(c[0], c[1])); ++n; }
    for (auto &c : too_many) { CHECK(!pairs_fit(c[0], c[1])); ++n; }
    // the stride forms
    CHECK(stride_form(5, 5) == FORM_PER_QUERY && stride_form(5, 0) == FORM_SHARED && stride_form(5, 4) == FORM_BAD && stride_form(5, 6) == FORM_BAD);
    CHECK(stride_form(5, -5) == FORM_BAD && stride_form(0, 0) == FORM_SHARED && stride_form(1, 1) == FORM_PER_QUERY);
    // plans at the size limit and under workspace limits that cut between and exactly at query boundaries
    for (auto &c : fits) {
        if (c[0] == 0 || c[1] == 0) continue;
        for (int64_t stride : {c[1], (int64_t)0})
            for (uint64_t budget : {(uint64_t)1 << 20, (uint64_t)8 << 30, (uint64_t)1 << 40}) {
                const Plan pl = make_plan(c[0], c[1], stride, 128, budget);
                CHECK(pl.slice_nq >= 1 && pl.slice_nq <= MAX_SLICE_QUERIES && pl.nslices == (c[0] + pl.slice_nq - 1) / pl.slice_nq);
                CHECK(slice_begin(pl, pl.nslices - 1) + slice_queries(pl, pl.nslices - 1) == c[0]);
                CHECK((uint64_t)pl.grid_x * TILE >= (uint64_t)c[1] && pl.locate_slots >= 1 && pl.locate_slots <= MAX_PAIRS);
                CHECK(pair_index(c[0] - 1, c[1], c[1] - 1) == (uint64_t)c[0] * (uint64_t)c[1] - 1);
                CHECK(loc_index(pl.shared, slice_queries(pl, 0) - 1, c[1], c[1] - 1) == (uint64_t)pl.locate_slots - 1);
                ++n;
            }
    }
    for (int64_t C : CASE_C)
        for (int64_t k : {1, 2, 7, 999, 1000, 1001}) {
            const uint64_t exact = LOCATE_BYTES_PER_SLOT * (uint64_t)C * (uint64_t)k;
            for (uint64_t budget : {exact - 1, exact, exact + 1, exact + LOCATE_BYTES_PER_SLOT * (uint64_t)C / 2}) {
                const Plan pl = make_plan(1000, C, C, 32, budget);
                const int64_t want = std::max<int64_t>(1, std::min<int64_t>(1000, (int64_t)(budget / (LOCATE_BYTES_PER_SLOT * (uint64_t)C))));
                CHECK(pl.slice_nq == want && pl.nslices == (1000 + want - 1) / want && pl.locate_slots == want * C);
                const Plan sh = make_plan(1000, C, 0, 32, budget);
                CHECK(sh.shared && sh.nslices == 1 && sh.slice_nq == 1000 && sh.locate_slots == C);
                ++n;
            }
        }
    // more queries than one launch's y extent: the shared row is sliced too
    const Plan big = make_plan(200000, 3, 0, 8, (uint64_t)8 << 30);
    CHECK(big.shared && big.slice_nq == MAX_SLICE_QUERIES && big.nslices == 4 && big.locate_slots == 3 && slice_queries(big, 3) == 200000 - 3 * 65535);
    // live slots: the clamp of the device entry
    CHECK(live_slots(false, -9, 7) == 7 && live_slots(true, -9, 7) == 0 && live_slots(true, 0, 7) == 0 && live_slots(true, 7, 7) == 7);
    CHECK(live_slots(true, 8, 7) == 7 && live_slots(true, INT32_MAX, 7) == 7 && live_slots(true, INT32_MIN, 7) == 0 && live_slots(true, 3, 7) == 3);
    CHECK(centre_vec4(32) && !centre_vec4(10) && !centre_vec4(6) && codeword_vec4(4) && codeword_vec4(16) && !codeword_vec4(5) && !codeword_vec4(6));
    return n + 8;
}

int main()
{
    std::mt19937 rng(20260);
    // d, m, ksub, bytes of a code, kc: 16-byte loads throughout; 40-byte rows; one sub-space; 16-byte centre rows with scalar codewords;
    // 16-bit codes at code strides 16 and 4
    const int shapes[][5] = {{32, 8, 256, 1, 7}, {10, 2, 256, 1, 5}, {6, 1, 17, 1, 3}, {24, 4, 2, 1, 4}, {32, 8, 300, 2, 7}, {10, 2, 300, 2, 5},
                             {12, 3, 256, 1, 6}, {16, 1, 40, 2, 2}};
    std::vector<Index> idx;
    for (auto &s : shapes) idx.push_back(make_index(s[0], s[1], s[2], s[3], s[4], rng));
    int calls = 0;
    size_t which = 0;
    for (int64_t C : CASE_C)
        for (int64_t nq : CASE_NQ)
            for (int shared = 0; shared < 2; ++shared)
                for (int counts_mode = 0; counts_mode < 3; ++counts_mode) {
                    const Index &ix = idx[which++ % idx.size()];
                    const uint64_t per_q = LOCATE_BYTES_PER_SLOT * (uint64_t)C;
                    // unlimited; exactly k queries; one byte short of k; between k and k + 1
                    const uint64_t budgets[] = {(uint64_t)8 << 30, per_q * 2, per_q * 3 - 1, per_q * 7 + per_q / 2, 1};
                    const size_t nb = nq == 1000 ? 2 : 5;            // (the long batches: unlimited and one cut, alternating)
                    for (size_t b = 0; b < nb; ++b) {
                        const uint64_t budget = nq == 1000 && b == 1 ? budgets[1 + (size_t)calls % 4] * 50 : budgets[b];
                        sim_call(ix, nq, C, shared != 0, counts_mode, budget, rng);
                        ++calls;
                    }
                }
    const int plans = plan_cases();
    std::printf("score_plan_check ok: %d simulated calls over %zu shapes, %llu pairs written once, %llu scored, %llu slices, %d plan cases\n", calls,
                idx.size(), (unsigned long long)g_pairs, (unsigned long long)g_live, (unsigned long long)g_slices, plans);
    return 0;
}
