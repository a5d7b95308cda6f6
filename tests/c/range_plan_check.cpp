// Stand-alone check of csrc/range_plan.h (tests/test_range_plan.py builds it with -fsanitize=address,undefined and runs it directly).
// It restates the count and the fill pass of csrc/range.hip.h lane by lane in plain C++ on top of the plan's arithmetic and checks:
// chunk lengths (default and forced), the items of a list cover its positions exactly once and nothing behind list_len, every survivor
// gets exactly one slot inside its query's row, the LDS refusal, 64-bit totals at SIFT1B-sized counts, the visit-order limit, and the
// sub-batch and sort-group splits over a grid of shapes.
#include "../../ivfadc.jl_amd/csrc/range_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

using namespace range_plan;

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            if (++g_fail > 20) exit(1);                                       \
        }                                                                     \
    } while (0)

static const int64_t CASE_LENS[] = {0, 1, 31, 32, 33, 63, 64, 65, 129, 256, 257, 1025};
constexpr size_t LDS_MAX = 160 << 10;

static uint32_t bits_of(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// a point's distance in the simulation: a hash of (list, position) as a small non-negative float
static float sim_dist(int l, uint64_t p) { return (float)((l * 7919u + p * 104729u) % 1000u) * 0.001f; }

static Facts facts(int d, int m, int ksub, int kc, int64_t n, int64_t maxlen, int force_chunk, size_t ws)
{
    Facts f;
    f.d = d; f.m = m; f.ksub = ksub; f.kc = kc; f.n = n; f.maxlen = maxlen; f.force_chunk = force_chunk; f.ws_budget = ws; f.lds_max = LDS_MAX;
    return f;
}

// count pass, scan, fill pass of one query over its w probes (the case table's lists in the given order), as the kernels walk them
static int64_t simulate(const Plan &pl, int w, const std::vector<int> &probes, float r, int64_t &checked_points)
{
    const int64_t items = pl.items;
    CHECK(items == (int64_t)w * pl.maxch);
    std::vector<uint32_t> cnt((size_t)items, 0xdeadbeefu), off((size_t)items, 0);
    std::vector<uint32_t> base((size_t)w, 0);
    for (int j = 1; j < w; ++j) base[(size_t)j] = base[(size_t)j - 1] + (uint32_t)CASE_LENS[probes[(size_t)j - 1]];
    const uint32_t rb = radius_bits(r, bits_of(r));
    auto walk = [&](bool fill, std::vector<uint64_t> *keys, std::vector<int> *writes) {
        for (int64_t item = 0; item < items; ++item) {
            const uint64_t j = probe_of((uint64_t)item, (uint64_t)pl.maxch), c = chunk_of((uint64_t)item, (uint64_t)pl.maxch);
            CHECK(item_of(j, c, (uint64_t)pl.maxch) == (uint64_t)item && j < (uint64_t)w);
            const int l = probes[(size_t)j];
            const uint64_t len = (uint64_t)CASE_LENS[l], p0 = chunk_begin(c, pl.chunk), p1 = chunk_end(len, c, pl.chunk);
            const bool live = p0 < p1 && radius_live(r);
            if (!live) { if (!fill) cnt[(size_t)item] = 0; continue; }
            CHECK(p1 <= len && p1 - p0 <= pl.chunk);
            uint32_t counter = 0;
            for (uint64_t pb = p0; pb < p1; pb += THREADS)
                for (int wave = 0; wave < THREADS / 64; ++wave) {   // one ballot per wave and round
                    uint32_t first = counter, nhit = 0;
                    for (int lane = 0; lane < 64; ++lane) {
                        const uint64_t p = pb + (uint64_t)wave * 64 + (uint64_t)lane;
                        if (p >= p1) continue;                       // nothing at or behind list_len is a candidate
                        CHECK(p < len);
                        if (!fill) ++checked_points;
                        const float dist = sim_dist(l, p);
                        if (bits_of(dist) <= rb) {
                            CHECK(dist <= r);
                            if (fill) {
                                const uint32_t slot = first + nhit;
                                CHECK(slot < cnt[(size_t)item]);
                                const size_t at = (size_t)off[(size_t)item] + slot;
                                (*keys)[at] = ((uint64_t)bits_of(dist) << 32) | (uint64_t)(base[(size_t)j] + (uint32_t)p);   // ASan: inside the row
                                (*writes)[at]++;
                            }
                            ++nhit;
                        } else {
                            CHECK(!(dist <= r));
                        }
                    }
                    counter += nhit;
                }
            if (!fill) cnt[(size_t)item] = counter;
            else CHECK(counter == cnt[(size_t)item]);
        }
    };
    walk(false, nullptr, nullptr);
    uint32_t run = 0;
    for (int64_t i = 0; i < items; ++i) { off[(size_t)i] = run; run += cnt[(size_t)i]; }
    std::vector<uint64_t> keys((size_t)run, 0);
    std::vector<int> writes((size_t)run, 0);
    walk(true, &keys, &writes);
    for (size_t i = 0; i < writes.size(); ++i) CHECK(writes[i] == 1);
    for (size_t i = 0; i < keys.size(); ++i)
        for (size_t k = i + 1; k < keys.size() && k < i + 3; ++k) CHECK(keys[i] != keys[k]);   // (keys are unique: visit orders are)
    return (int64_t)run;
}

int main()
{
    // ---- chunk lengths ----------------------------------------------------------------------------------------------------------
    int shapes = 0;
    for (int m : {1, 3, 8, 10, 16, 48, 64})
        for (int dsub : {1, 4, 6, 16, 32})
            for (int ksub : {2, 64, 256}) {
                const int d = m * dsub;
                const uint32_t c = default_chunk(d, m, ksub);
                CHECK(c % CHUNK_ALIGN == 0 && c >= (uint32_t)CHUNK_ALIGN);
                CHECK((uint64_t)8 * ksub * d <= (uint64_t)c * m);                                    // the build costs at most an eighth of the lookups
                CHECK(c == (uint32_t)CHUNK_ALIGN || (uint64_t)8 * ksub * d > (uint64_t)(c - CHUNK_ALIGN) * m);   // ... and no shorter multiple of 256 would do
                CHECK(lds_bytes(d, m) == ((size_t)((d + 3) / 4 * 4) + (size_t)m * 256) * 4 + COUNTER_BYTES);
                ++shapes;
            }
    CHECK(default_chunk(128, 8, 256) == 32768);   // the SIFT1M shape: 8 * 256 * 128 / 8
    for (int fc : {1, 63, 64, 65, 1000, 1024, 1025}) {
        CHECK(forced_chunk(fc) % FORCED_ALIGN == 0 && forced_chunk(fc) >= (uint32_t)fc && forced_chunk(fc) < (uint32_t)fc + FORCED_ALIGN);
        const Plan p = make_plan(facts(32, 8, 256, 12, 1956, 1025, fc, (size_t)8 << 30), 20, 12);
        CHECK(p.fits && p.chunk == forced_chunk(fc) && p.maxch == (int64_t)chunks_of(1025, p.chunk) && p.items == 12 * p.maxch);
    }
    CHECK(forced_chunk(1) == 64 && make_plan(facts(32, 8, 256, 12, 1956, 1025, 1024, (size_t)8 << 30), 20, 12).maxch == 2);
    CHECK(make_plan(facts(32, 8, 256, 12, 0, 0, 0, (size_t)8 << 30), 1, 1).maxch == 1);   // an empty index still has a grid

    // ---- items cover the lists; count, scan and fill agree; over the case table's lengths -------------------------------------------
    int64_t sims = 0, points = 0;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int fc : {0, 1, 64, 128, 256, 1024, 2048})
        for (int w : {1, 3, 12}) {
            std::vector<int> probes;
            for (int j = 0; j < w; ++j) probes.push_back((j * 5 + 11) % 12);   // the long list first, then a spread (5 and 12 coprime)
            const Plan pl = make_plan(facts(32, 8, 256, 12, 1956, 1025, fc, (size_t)8 << 30), 1, w);
            CHECK(pl.fits);
            int64_t probed = 0;
            for (int l : probes) probed += CASE_LENS[l];
            for (float r : {-1.0f, -0.0f, 0.0f, 0.0005f, 0.25f, 0.5f, 0.999f, 2.0f, inf, nan, -inf}) {
                int64_t pts = 0;
                const int64_t got = simulate(pl, w, probes, r, pts);
                int64_t want = 0;
                for (int l : probes)
                    for (int64_t p = 0; p < CASE_LENS[l]; ++p) want += sim_dist(l, (uint64_t)p) <= r ? 1 : 0;
                CHECK(got == want);
                CHECK(pts == (radius_live(r) ? probed : 0));   // every probed point tested exactly once, none behind a list's end
                if (r == inf) CHECK(got == probed);
                if (!(r >= 0)) CHECK(got == 0);
                ++sims;
                points += pts;
            }
        }
    // the radius test itself, value by value
    for (float d : {0.0f, 1e-30f, 0.5f, 3.0e38f})
        for (float r : {nan, -nan, -1.0f, -0.0f, 0.0f, 0.5f, 1e-30f, inf, -inf})
            CHECK((radius_live(r) && bits_of(d) <= radius_bits(r, bits_of(r))) == (d <= r));

    // ---- the LDS refusal, the visit-order limit, 64-bit totals -------------------------------------------------------------------
    CHECK(make_plan(facts(768, 48, 256, 4, 2000, 600, 0, (size_t)8 << 30), 4, 2).fits);
    CHECK(lds_bytes(768, 48) == 52240);
    {
        const Plan p = make_plan(facts(1280, 160, 256, 4, 2000, 600, 0, (size_t)8 << 30), 4, 2);
        CHECK(!p.fits && lds_bytes(1280, 160) > LDS_MAX && strstr(p.why, "LDS"));
        CHECK(make_plan(facts(4, 159, 256, 4, 2000, 600, 0, (size_t)8 << 30), 4, 2).fits == (lds_bytes(4, 159) <= LDS_MAX));
    }
    {
        const int64_t sift1b = 1000000000;
        const Plan p = make_plan(facts(128, 8, 256, 1 << 20, sift1b, 4000, 0, (size_t)8 << 30), 10000, 64);
        CHECK(p.fits && p.nb >= 1 && p.nb <= 10000);
        CHECK(!make_plan(facts(128, 8, 256, 1 << 20, (int64_t)1 << 32, 4000, 0, (size_t)8 << 30), 10, 64).fits);
        CHECK(make_plan(facts(128, 8, 256, 1 << 20, ((int64_t)1 << 32) - 1, 4000, 0, (size_t)8 << 30), 10, 64).fits);
        std::vector<uint64_t> tot(10000, 4000000);   // 4 * 10^10 results: 160 GB of ids at 4 B, more than 2^32 entries
        tot[17] = ((uint64_t)1 << 32) - 1;
        const std::vector<int64_t> lims = make_lims(tot);
        CHECK(lims.size() == 10001 && lims[0] == 0);
        CHECK(lims[10000] == (int64_t)9999 * 4000000 + (((int64_t)1 << 32) - 1) && lims[10000] > ((int64_t)1 << 35));
        for (size_t q = 0; q < tot.size(); ++q) CHECK(lims[q + 1] - lims[q] == (int64_t)tot[q]);
        // groups: below 2^32 keys each, whole queries, in order, nothing lost
        uint64_t keys = 0, sum = 0;
        int64_t g0 = 0, groups = 0;
        while (g0 < (int64_t)tot.size()) {
            const int64_t g1 = next_group(tot, g0, p.cap_keys, &keys);
            CHECK(g1 > g0 && keys < VISIT_LIMIT && g1 - g0 <= MAX_GRID_Y);
            CHECK(g1 - g0 == 1 || keys <= (uint64_t)p.cap_keys);
            sum += keys;
            g0 = g1;
            ++groups;
        }
        CHECK(sum == (uint64_t)lims[10000] && groups > 10);
        std::vector<uint64_t> huge = {5, (uint64_t)1 << 32, 5};
        CHECK(next_group(huge, 0, 1 << 20, &keys) == 1 && keys == 5);
        CHECK(next_group(huge, 1, 1 << 20, &keys) == 1);          // refused: one query with 2^32 keys
    }

    // a launch grid: w x maxch work items of 256 lanes stay below 2^32 lanes, refused by the plan (not by the launch) beyond
    CHECK(MAX_GRID_X == 16777215 && (uint64_t)(MAX_GRID_X + 1) * THREADS == ((uint64_t)1 << 32));
    // (forced chunk 64, w = 2048: 8191 chunks are 16 775 168 items, 8192 are 2^24)
    CHECK(make_plan(facts(32, 8, 256, 4096, 3000000000ll, (int64_t)64 * 8191, 1, (size_t)8 << 30), 1, 2048).fits);
    {
        const Plan p = make_plan(facts(32, 8, 256, 4096, 3000000000ll, (int64_t)64 * 8191 + 1, 1, (size_t)8 << 30), 1, 2048);
        CHECK(!p.fits && strstr(p.why, "longer chunk"));
    }

    // ---- sub-batch splits over a grid of shapes ------------------------------------------------------------------------------------
    int64_t grid = 0;
    for (int kc : {1, 4, 12, 1024, 1 << 20})
        for (int m : {1, 8, 48})
            for (int64_t maxlen : {(int64_t)0, (int64_t)1, (int64_t)1025, (int64_t)100000, (int64_t)3000000000ll})
                for (int fc : {0, 1, 1024})
                    for (int w : {1, 3, 64, 2048})
                        for (size_t ws : {(size_t)1 << 20, (size_t)64 << 20, (size_t)8 << 30})
                            for (int64_t nq : {(int64_t)0, (int64_t)1, (int64_t)7, (int64_t)1000, (int64_t)300000}) {
                                if (w > kc) continue;
                                const Plan p = make_plan(facts(m * 16, m, 256, kc, maxlen, maxlen, fc, ws), nq, w);
                                ++grid;
                                if (!p.fits) { CHECK((int64_t)w * (int64_t)chunks_of((uint64_t)maxlen, p.chunk) > MAX_GRID_X); continue; }
                                CHECK(p.nb >= 1 && (nq == 0 || p.nb <= nq) && p.nb <= MAX_GRID_Y);
                                CHECK(p.nb == 1 || p.nb * (int64_t)kc < ((int64_t)1 << 31));
                                CHECK(p.nb == 1 || (uint64_t)p.nb * (uint64_t)p.per_query_bytes <= ws);
                                CHECK(p.maxch >= 1 && (uint64_t)p.maxch * p.chunk >= (uint64_t)maxlen && p.items <= MAX_GRID_X);
                                CHECK(p.maxch == 1 || (uint64_t)(p.maxch - 1) * p.chunk < (uint64_t)maxlen);
                                CHECK(p.cap_keys >= (1 << 20) && (p.cap_keys == (1 << 20) || (uint64_t)p.cap_keys * 24 <= ws));
                                // every query lands in exactly one sub-batch
                                int64_t covered = 0;
                                for (int64_t a0 = 0; a0 < nq && covered <= nq; a0 += p.nb) covered += (p.nb < nq - a0 ? p.nb : nq - a0);
                                CHECK(covered == nq);
                            }
    if (g_fail) {
        fprintf(stderr, "range_plan_check: %d failures\n", g_fail);
        return 1;
    }
    printf("range_plan_check ok: %d shapes, %lld simulated searches over %d lengths, %lld points, %lld grid cases\n", shapes, (long long)sims,
           (int)(sizeof CASE_LENS / sizeof CASE_LENS[0]), (long long)points, (long long)grid);
    return 0;
}
