// Stand-alone check of what csrc/range_plan.h and csrc/maskset_plan.h add for the masked range search (ivfadc_range_search_masked);
// tests/test_range_masked_plan.py builds it with -fsanitize=address,undefined and runs it directly.  It checks:
//   * the table-free LDS need and chunk (16-bit codes: residual [m][dsp] and the counter, no "tables exceed LDS" refusal, 1024 points an
//     item unless a chunk is forced), and that the table form's figures are what they were;
//   * the invariant the mask test stands on: every chunk begins on a round of 64, for the default chunks over a grid of shapes and for
//     forced chunks of 64, 256 and 1024 (and the odd values that are rounded up to them) over the case table's lengths;
//   * the mask words of every item of every list, as range_scan_item<.., MASKED> addresses them: a wave's round is read through
//     maskset::round_word at words that lie inside the list's row (ASan: the row is allocated at its exact size), every position is
//     tested exactly once, with the bit maskset::slot_selected names, count and fill see the same lanes, and nothing at or behind
//     list_len is a candidate even where the row's last words have bits set there;
//   * per_query_bytes: plus the 4 bytes of the ingested mask number, and the sub-batch that follows.
#include "../../ivfadc.jl_amd/csrc/maskset_plan.h"
#include "../../ivfadc.jl_amd/csrc/range_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

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
constexpr int NLISTS = (int)(sizeof(CASE_LENS) / sizeof(CASE_LENS[0]));
constexpr size_t LDS_MAX = 160 << 10;

static Facts facts(int d, int m, int ksub, int kc, int64_t n, int64_t maxlen, int force_chunk, size_t ws, bool table_free, bool masked)
{
    Facts f;
    f.d = d; f.m = m; f.ksub = ksub; f.kc = kc; f.n = n; f.maxlen = maxlen; f.force_chunk = force_chunk; f.ws_budget = ws; f.lds_max = LDS_MAX;
    f.table_free = table_free;
    f.masked = masked;
    return f;
}

// a mask's bit for (list, position): a hash, so that words differ between lists and rounds
static bool sim_bit(int mask, int l, uint64_t p) { return ((uint64_t)(mask + 1) * 2654435761u + (uint64_t)l * 40503u + p * 2246822519u) % 7u < 3u; }

int main()
{
    // ---- table-free LDS and chunk -----------------------------------------------------------------------------------------------
    int shapes = 0;
    for (int m : {1, 2, 3, 5, 8, 48, 64})
        for (int dsub : {1, 3, 4, 6, 16, 17}) {
            const int d = m * dsub, dsp = (dsub + 3) / 4 * 4;
            CHECK(lds_bytes_table_free(m, dsub) == (size_t)m * dsp * 4 + 16);
            CHECK(lds_bytes_table_free(m, dsub) % 16 == 0);   // the counter behind the residual is aligned
            for (int ksub : {200, 300, 1024, 65536}) {
                const Plan p = make_plan(facts(d, m, ksub, 12, 1956, 1025, 0, (size_t)8 << 30, true, false), 20, 3);
                CHECK(p.fits && p.lds == lds_bytes_table_free(m, dsub) && p.chunk == TABLE_FREE_CHUNK && p.chunk == 1024);
                CHECK(p.maxch == 2 && p.items == 6);
                const Plan pf = make_plan(facts(d, m, ksub, 12, 1956, 1025, 1, (size_t)8 << 30, true, false), 20, 3);
                CHECK(pf.fits && pf.chunk == 64 && pf.maxch == 17);
                // the table form of the same shape is what it was
                const Plan pt = make_plan(facts(d, m, 256, 12, 1956, 1025, 0, (size_t)8 << 30, false, false), 20, 3);
                CHECK(pt.lds == lds_bytes(d, m) && (!pt.fits || pt.chunk == default_chunk(d, m, 256)));
                ++shapes;
            }
        }
    CHECK(lds_bytes_table_free(48, 16) == 48 * 16 * 4 + 16);   // m = 48, d = 768: 3 KB where the tables take 52 KB
    {   // no "tables exceed LDS" refusal: m = 160, d = 1280 is refused by the table form and served table-free
        CHECK(!make_plan(facts(1280, 160, 256, 4, 2000, 600, 0, (size_t)8 << 30, false, false), 4, 2).fits);
        const Plan p = make_plan(facts(1280, 160, 1024, 4, 2000, 600, 0, (size_t)8 << 30, true, false), 4, 2);
        CHECK(p.fits && p.lds == 1280 * 4 + 16);
        // every other limit is unchanged: 2^32 points
        const Plan big = make_plan(facts(32, 8, 1024, 4, (int64_t)1 << 32, 600, 0, (size_t)8 << 30, true, false), 4, 2);
        CHECK(!big.fits && strstr(big.why, "2^32"));
    }

    // ---- every chunk begins on a round --------------------------------------------------------------------------------------------
    int64_t begins = 0;
    for (int m : {1, 3, 8, 10, 48})
        for (int dsub : {1, 4, 6, 16})
            for (int ksub : {16, 64, 200, 256}) {
                const uint32_t c = default_chunk(m * dsub, m, ksub);
                CHECK(chunk_is_round_aligned(c) && c % CHUNK_ALIGN == 0);
            }
    CHECK(chunk_is_round_aligned(TABLE_FREE_CHUNK) && !chunk_is_round_aligned(0) && !chunk_is_round_aligned(96));
    for (int force : {1, 63, 64, 65, 200, 256, 1000, 1024, 1025}) {
        const uint32_t c = forced_chunk(force);
        CHECK(chunk_is_round_aligned(c) && c >= (uint32_t)force && c < (uint32_t)force + 64);
        for (int l = 0; l < NLISTS; ++l)
            for (uint64_t ch = 0; ch < chunks_of((uint64_t)CASE_LENS[l], c) + 1; ++ch) {
                CHECK(chunk_begin(ch, c) % 64 == 0);
                ++begins;
            }
    }
    CHECK(forced_chunk(64) == 64 && forced_chunk(256) == 256 && forced_chunk(1024) == 1024);

    // ---- mask words of every item of every list -----------------------------------------------------------------------------------
    std::vector<int64_t> lens(CASE_LENS, CASE_LENS + NLISTS);
    const maskset::Layout L = maskset::make_layout(lens);
    const int nmasks = 3;
    // the set, at its exact size; bits at or behind list_len inside a row's last round are SET here (hostile: the build kernel leaves
    // them 0, the scan must not depend on it)
    std::vector<uint32_t> words((size_t)nmasks * L.W, 0);
    for (int k = 0; k < nmasks; ++k)
        for (int l = 0; l < NLISTS; ++l) {
            uint32_t *row = words.data() + maskset::row_start(L.W, L.word_off[(size_t)l], (uint32_t)k);
            const uint64_t rw = maskset::row_words((uint64_t)lens[(size_t)l]);
            CHECK(L.word_off[(size_t)l + 1] - L.word_off[(size_t)l] == rw);
            for (uint64_t p = 0; p < rw * 32; ++p)
                if (p >= (uint64_t)lens[(size_t)l] || sim_bit(k, l, p)) row[maskset::word_of(p)] |= 1u << maskset::bit_of(p);
        }
    int64_t items_walked = 0, points = 0, rounds_skipped = 0;
    for (int chunk_req : {0, 64, 256, 1024}) {
        const Plan pl = make_plan(facts(32, 8, 1024, NLISTS, 1956, 1025, chunk_req, (size_t)8 << 30, true, true), 22, NLISTS);
        CHECK(pl.fits && chunk_is_round_aligned(pl.chunk));
        for (int k = -1; k < nmasks; ++k)
            for (int l = 0; l < NLISTS; ++l) {
                const uint64_t len = (uint64_t)lens[(size_t)l];
                // mask_row: null for -1; the row as a bounded view otherwise (ASan catches a word outside the set; the CHECKs below, one
                // outside the list's own row)
                const uint32_t *row = k < 0 ? nullptr : words.data() + maskset::row_start(L.W, L.word_off[(size_t)l], (uint32_t)k);
                const uint64_t rw = maskset::row_words(len);
                std::vector<int> seen((size_t)len, 0);
                for (int pass = 0; pass < 2; ++pass) {   // count, fill: the same lanes
                    std::vector<int> valid_of((size_t)len, 0);
                    for (int64_t c = 0; c < pl.maxch; ++c) {
                        const uint64_t p0 = chunk_begin((uint64_t)c, pl.chunk), p1 = chunk_end(len, (uint64_t)c, pl.chunk);
                        if (!(p0 < p1)) continue;
                        ++items_walked;
                        for (uint64_t pb = p0; pb < p1; pb += THREADS)
                            for (int wave = 0; wave < THREADS / 64; ++wave) {
                                const uint64_t pw = pb + (uint64_t)wave * 64;
                                CHECK(pw % 64 == 0);
                                uint64_t bits = ~(uint64_t)0;
                                if (row && pw < p1) {
                                    const uint64_t wd = maskset::round_word(pw);
                                    CHECK(wd + 1 < rw);   // both words inside this list's row
                                    bits = maskset::round_bits(row[wd], row[wd + 1]);
                                }
                                int nvalid = 0;
                                for (int lane = 0; lane < 64; ++lane) {
                                    const uint64_t p = pw + (uint64_t)lane;
                                    const bool valid = p < p1 && ((bits >> lane) & 1u) != 0;
                                    if (!valid) continue;
                                    CHECK(p < len);
                                    CHECK(!row || maskset::slot_selected(row, p));
                                    CHECK(k < 0 || sim_bit(k, l, p));
                                    valid_of[(size_t)p]++;
                                    ++nvalid;
                                    ++points;
                                }
                                if (nvalid == 0 && pw < p1) ++rounds_skipped;
                            }
                    }
                    for (uint64_t p = 0; p < len; ++p) {
                        CHECK(valid_of[(size_t)p] == ((k < 0 || sim_bit(k, l, p)) ? 1 : 0));   // every selected position once, no other
                        seen[(size_t)p] += valid_of[(size_t)p];
                    }
                }
                for (uint64_t p = 0; p < len; ++p) CHECK(seen[(size_t)p] == 0 || seen[(size_t)p] == 2);   // count and fill agree
            }
    }

    // ---- per_query_bytes ------------------------------------------------------------------------------------------------------------
    for (int w : {1, 3, 12})
        for (int force : {0, 1, 1024})
            for (bool tf : {false, true}) {
                const Plan a = make_plan(facts(32, 8, tf ? 1024 : 256, 12, 1956, 1025, force, (size_t)1 << 20, tf, false), 176, w);
                const Plan b = make_plan(facts(32, 8, tf ? 1024 : 256, 12, 1956, 1025, force, (size_t)1 << 20, tf, true), 176, w);
                CHECK(a.fits && b.fits && b.per_query_bytes == a.per_query_bytes + 4);
                CHECK(a.per_query_bytes == (int64_t)12 * 20 + (int64_t)w * 12 + a.items * 8 + 64);
                CHECK(b.nb <= a.nb && b.nb >= 1 && b.nb * b.per_query_bytes <= ((int64_t)1 << 20));
                CHECK(a.chunk == b.chunk && a.items == b.items && a.lds == b.lds && a.cap_keys == b.cap_keys);
            }

    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("range_masked_plan_check ok: %d shapes, %lld chunk begins, %lld items over %d lengths, %lld points, %lld empty rounds\n", shapes,
           (long long)begins, (long long)items_walked, NLISTS, (long long)points, (long long)rounds_skipped);
    return 0;
}
