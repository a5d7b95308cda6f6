// The mask-set layout (csrc/maskset_plan.h) and the masked search's planner (make_plan_masked, csrc/plan.h) on the CPU: a stand-alone
// program, built with the sanitizers by tests/test_maskset_plan.py.
//
//   maskset_plan_check TABLE
//
//   layout       rows are disjoint and whole rounds, a list of 2^32 - 1 points and one of 0 are handled, offsets are 64-bit
//   bits         word_of / bit_of / round_word / slot_selected / round_bits against a bit-by-bit restatement, for every position of the case-table
//                lengths: a build restated lane by lane (ballot of a round -> two words) is read back position by position
//   planner      make_plan_masked over the shapes of plan_grid.h x K, w, nq x forced widths and chunks
//   untouched    make_plan / make_plan_u16 still return every row of tests/plan_table.tsv (read only)
// closes with "maskset_plan_check ok: <lengths> lengths, <grid cases> grid cases, <rows> table rows"
#include "../../ivfadc.jl_amd/csrc/maskset_plan.h"
#include "../../ivfadc.jl_amd/csrc/plan.h"
#include "../../ivfadc.jl_amd/csrc/subset_plan.h"
#include "plan_grid.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace ivf;
using namespace plan_grid_ns;

static long g_bad = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond) && g_bad++ < 20) printf("FAILED %s (line %d)\n", #cond, __LINE__);    \
    } while (0)

static const int64_t CASE_LENS[] = {0, 1, 31, 32, 33, 63, 64, 65, 129, 256, 257, 1025};

static void check_layout()
{
    // the case table, and the extremes: an empty list between long ones, the longest list ids allow
    std::vector<int64_t> len(CASE_LENS, CASE_LENS + sizeof CASE_LENS / sizeof *CASE_LENS);
    len.push_back(((int64_t)1 << 32) - 1);
    len.push_back(0);
    len.push_back(64);
    const maskset::Layout L = maskset::make_layout(len);
    CHECK(L.word_off.size() == len.size() + 1 && L.word_off[0] == 0 && L.W == L.word_off.back());
    uint64_t expect = 0;
    for (size_t l = 0; l < len.size(); ++l) {
        const uint64_t words = L.word_off[l + 1] - L.word_off[l];
        CHECK(L.word_off[l] == expect);                                        // rows follow each other: disjoint, no gap
        CHECK(words % maskset::ROUND_WORDS == 0);                              // whole rounds
        CHECK(words * 32 >= (uint64_t)len[l] && words * 32 < (uint64_t)len[l] + 64);   // ... and no more of them than the list needs
        CHECK(words == maskset::row_words((uint64_t)len[l]));
        CHECK(L.word_off[l] % 2 == 0);                                         // a round is one aligned 8-byte store
        if (len[l] > 0) {
            const uint64_t last = (uint64_t)len[l] - 1;
            CHECK(maskset::word_of(last) < words && maskset::round_word(last) + 1 < words + 1 && maskset::round_word(last) + 2 <= words);
        }
        expect += words;
    }
    CHECK(maskset::row_words(((uint64_t)1 << 32) - 1) == ((uint64_t)1 << 27));   // 2^26 rounds
    CHECK(L.W > ((uint64_t)1 << 27));                                              // 64-bit offsets: mask r = 40 starts beyond 2^32 words
    CHECK(maskset::row_start(L.W, L.word_off[3], 40) == 40 * L.W + L.word_off[3] && 40 * L.W > ((uint64_t)1 << 32));
    CHECK(maskset::row_words(0) == 0);
    CHECK(maskset::clamp_mask(-5, 16) == -1 && maskset::clamp_mask(-1, 16) == -1 && maskset::clamp_mask(0, 16) == 0 &&
          maskset::clamp_mask(15, 16) == 15 && maskset::clamp_mask(16, 16) == 15 && maskset::clamp_mask(0x7fffffff, 1) == 0);
}

// maskset_build_kernel restated lane by lane on the CPU for one mask: ids -> keep (subset::subset_selected) -> ballot -> two words per round
static void build_row(const std::vector<uint32_t> &ids, const std::vector<uint32_t> &bits, uint64_t nbits, uint32_t *row, int64_t spare_behind)
{
    const int64_t len = (int64_t)ids.size() - spare_behind;   // the ids behind len are stale spare capacity: they must not show
    const std::vector<subset::Item> items = subset::make_items(std::vector<int64_t>(1, len));
    for (const subset::Item &it : items)
        for (int wv = 0; wv < 4; ++wv)
            for (int r = 0; r < subset::SUBSET_ROUNDS; ++r) {
                uint64_t ballot = 0;
                const int64_t first = subset::subset_point(it.chunk, wv, r, 0);
                for (int lane = 0; lane < 64; ++lane) {
                    const int64_t p = subset::subset_point(it.chunk, wv, r, lane);
                    const bool keep = p < len && subset::subset_selected(bits.data(), nbits, ids[(size_t)p]);
                    if (keep) ballot |= (uint64_t)1 << lane;
                }
                if (first < len) {
                    row[maskset::round_word((uint64_t)first)] = (uint32_t)ballot;
                    row[maskset::round_word((uint64_t)first) + 1] = (uint32_t)(ballot >> 32);
                }
            }
}

static long check_bits()
{
    long lens = 0;
    for (int64_t len : CASE_LENS) {
        for (int64_t spare : {(int64_t)0, (int64_t)40}) {
            const size_t slots = (size_t)(len + spare);
            // ids: a fixed scramble; the id-space bitmap selects id i iff (i * 7 + 3) % 5 < 2, cut at nbits (ids at or above: never)
            std::vector<uint32_t> ids(slots);
            for (size_t p = 0; p < slots; ++p) ids[p] = (uint32_t)((p * 2654435761u) % 4099u);
            const uint64_t nbits = 3000;
            std::vector<uint32_t> bits((size_t)((nbits + 31) / 32), 0);
            for (uint64_t i = 0; i < nbits; ++i)
                if ((i * 7 + 3) % 5 < 2) bits[(size_t)(i >> 5)] |= 1u << (i & 31);
            const uint64_t words = maskset::row_words((uint64_t)len);
            std::vector<uint32_t> row((size_t)words + 2, 0xDEADBEEFu);   // two guard words behind the row
            build_row(ids, bits, nbits, row.data(), spare);
            CHECK(row[(size_t)words] == 0xDEADBEEFu && row[(size_t)words + 1] == 0xDEADBEEFu);   // nothing written behind the row
            for (uint64_t p = 0; p < words * 32; ++p) {
                // bit by bit: position p lives in word floor(p / 32), bit p mod 32; behind len it is 0 whatever id lies there
                const bool want = p < (uint64_t)len && ids[(size_t)p] < nbits && ((ids[(size_t)p] * 7ull + 3) % 5 < 2);
                CHECK(maskset::word_of(p) == p / 32 && maskset::bit_of(p) == (uint32_t)(p % 32));
                CHECK(maskset::slot_selected(row.data(), p) == want);
                const uint64_t rw = maskset::round_word(p);
                CHECK(rw == (p / 64) * 2 && rw + 1 < words + 1);
                CHECK((((maskset::round_bits(row[(size_t)rw], row[(size_t)rw + 1])) >> (p % 64)) & 1u) == (want ? 1u : 0u));
            }
            ++lens;
        }
    }
    return lens;
}

static long check_planner()
{
    long cases = 0;
    each_context<PlanFacts>([&](const PlanFacts &base) {
        if (base.u16) return;   // every UInt16 handle takes the masked generic path
        for (int fq : {0, 1, 2, 4, 8, -1, -3})
            for (int fc : TUNE_CHUNK)
                for (int64_t nq : NQS_FIXED)
                    for (int K : KS)
                        for (int w : WS) {
                            PlanFacts f = base;
                            f.force_qg = fq;
                            f.force_chunk = fc;
                            const int wc = w < f.kc ? w : f.kc;
                            const Plan p = make_plan_masked(f, nq, K, wc);
                            ++cases;
                            CHECK(p.form == ScanForm::Masked && p.striped() == 8 && !p.query_major() && !p.fuse_topw && !p.lanes);
                            CHECK(p.qg == 1 || p.qg == 2 || p.qg == 4);
                            if ((fq == 1 || fq == 2 || fq == 4) && p.fits) CHECK(p.qg <= fq);
                            if ((fq == 1 || fq == 2 || fq == 4) && scan_lds_bytes(f.m, f.d, fq, p.cap, p.small_k, true, false) <= LDS_MAX) CHECK(p.qg == fq);
                            CHECK(!p.fits || p.lds <= LDS_MAX);
                            CHECK(!p.fits || p.lds == scan_lds_bytes(f.m, f.d, p.qg, p.cap, p.small_k, true, false));
                            if (p.fits && !(fq == 1 || fq == 2 || fq == 4)) CHECK(p.qg == 1 || p.lds <= (size_t)(80 << 10));
                            if (!p.fits) continue;
                            CHECK(p.nb >= 1 && p.nb <= nq);
                            CHECK(p.CH > 0 && p.CH % 1024 == 0);
                            CHECK(p.maxch >= 1 && p.maxch <= 64 && (f.maxlen + p.CH - 1) / p.CH <= 64);
                            CHECK(p.threads == 256 && p.cap == sel_cap(K) && p.small_k == (K <= 64));
                        }
    });
    return cases;
}

static long check_table(const char *path)
{
    FILE *fp = fopen(path, "r");
    if (!fp) { printf("cannot open %s\n", path); ++g_bad; return 0; }
    char row[2048], line[1024];
    long rows = 0;
    for (long no = 1; fgets(row, sizeof row, fp); ++no) {
        row[strcspn(row, "\r\n")] = 0;
        if (no == 1) continue;
        PlanFacts f;
        int64_t nq;
        int K, w;
        bool pre;
        if (!plan_parse(row, f, nq, K, w, pre)) { printf("%s:%ld: not a case\n", path, no); ++g_bad; break; }
        const Plan p = f.u16 ? make_plan_u16(f, nq, K, w, pre) : make_plan(f, nq, K, w, pre);
        plan_line(line, sizeof line, f, nq, K, w, pre, p);
        if (strcmp(row, line) != 0 && g_bad++ < 20) printf("%s:%ld: an existing plan changed\n  pinned  %s\n  planned %s\n", path, no, row, line);
        CHECK(p.form != ScanForm::Masked);
        ++rows;
    }
    fclose(fp);
    return rows;
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: maskset_plan_check TABLE\n"); return 2; }
    check_layout();
    const long lens = check_bits();
    const long cases = check_planner();
    const long rows = check_table(argv[1]);
    if (g_bad) { printf("%ld failures\n", g_bad); return 1; }
    printf("maskset_plan_check ok: %ld lengths, %ld grid cases, %ld table rows\n", lens, cases, rows);
    return 0;
}
