// Stand-alone check of csrc/search_call.h (tests/test_search_call.py builds it with -fsanitize=address,undefined and runs it directly).
//
// 1. SearchCall::slice and ProbeRows::slice.  Host arrays of exactly the batch's size are laid out for nq = 1, 2, 5, 64, 65, d = 1, 50,
//    K = 1, 10, w = 1, 3 and every combination of present and absent optional rows; nested slices -- sub-batch, then sort group, then
//    grid-y block, as search_dev / search_generic / range_dev take them -- are checked at every (b0, n): every pointer lands on the element
//    a flat index computes (and the slice's first and last element are read, so an overrun is the sanitizer's to report), null stays null,
//    slices compose (slice(a, n).slice(b, k) == slice(a + b, k)) and whole_batch survives only the identity slice.
// 2. The sort groups of search_generic.  Its stage B used to cut groups with an inline loop; it now calls range_plan::next_group, as the
//    range search does.  The old loop is restated here literally and compared with next_group, (g1, keys) group by group, over totals at
//    the edges: sums on, one above and one below cap_keys, a single total above it, runs of zeros, sums reaching 2^32 - 1 and 2^32, and
//    batches of 1, 2, 65 534 and 65 535 queries (the generic path never passes more: its nba clamp, range_plan::MAX_GRID_Y).
#include "../../ivfadc.jl_amd/csrc/range_plan.h"
#include "../../ivfadc.jl_amd/csrc/search_call.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>
#include <vector>

using ivf::ProbeRows;
using ivf::SearchCall;

static_assert(std::is_trivially_copyable<SearchCall>::value && std::is_trivially_copyable<ProbeRows>::value, "passed by value, no ownership");

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            if (++g_fail > 20) exit(1);                                       \
        }                                                                     \
    } while (0)

// ---- 1. slices ------------------------------------------------------------------------------------------------------------------
enum Row { IDS = 1, DISTS = 2, COUNTS = 4, RADII = 8, PRE = 16, OUT = 32, MASK = 64, ROWS_ALL = 128 };

struct Arrays {
    std::vector<float> q, dists, radii, pre_dc, out_dc;
    std::vector<uint32_t> ids, words;
    std::vector<int32_t> counts, out_list, moq;
    std::vector<int> pre_list;
    std::vector<uint64_t> word_off;
};

static long long g_slices = 0;
static volatile float g_sink_f;
static volatile uint32_t g_sink_u;

// s is queries [b0, b0 + n) of the call c0 laid over `a`
static void check_slice(const Arrays &a, const SearchCall &c0, const SearchCall &s, int64_t b0, int64_t n)
{
    const size_t o = (size_t)b0, d = (size_t)c0.d, K = (size_t)c0.K, w = (size_t)c0.w;
    CHECK(s.nq == n && s.d == c0.d && s.K == c0.K && s.w == c0.w);
    CHECK(s.q == a.q.data() + o * d);
    CHECK(s.ids == (c0.ids ? a.ids.data() + o * K : nullptr));
    CHECK(s.dists == (c0.dists ? a.dists.data() + o * K : nullptr));
    CHECK(s.counts == (c0.counts ? a.counts.data() + o : nullptr));
    CHECK(s.radii == (c0.radii ? a.radii.data() + o : nullptr));
    CHECK(s.pre_list == (c0.pre_list ? a.pre_list.data() + o * w : nullptr));
    CHECK(s.pre_dc == (c0.pre_dc ? a.pre_dc.data() + o * w : nullptr));
    CHECK(s.out_list == (c0.out_list ? a.out_list.data() + o * w : nullptr));
    CHECK(s.out_dc == (c0.out_dc ? a.out_dc.data() + o * w : nullptr));
    CHECK(s.mask_of_query == (c0.mask_of_query ? a.moq.data() + o : nullptr));
    // the set's constant part does not move
    CHECK(s.mask_words == c0.mask_words && s.mask_word_off == c0.mask_word_off && s.mask_W == c0.mask_W);
    CHECK(s.pre() == c0.pre() && s.masked() == c0.masked());
    CHECK(s.whole_batch == (b0 == 0 && n == c0.nq));
    if (n > 0) {   // first and last element of every row of the slice: inside the arrays
        const size_t l = (size_t)n - 1;
        g_sink_f = s.q[0] + s.q[l * d + d - 1];
        if (s.ids) g_sink_u = s.ids[0] + s.ids[l * K + K - 1];
        if (s.dists) g_sink_f = s.dists[0] + s.dists[l * K + K - 1];
        if (s.counts) g_sink_u = (uint32_t)(s.counts[0] + s.counts[l]);
        if (s.radii) g_sink_f = s.radii[0] + s.radii[l];
        if (s.pre_list) g_sink_u = (uint32_t)(s.pre_list[0] + s.pre_list[l * w + w - 1]);
        if (s.pre_dc) g_sink_f = s.pre_dc[0] + s.pre_dc[l * w + w - 1];
        if (s.out_list) g_sink_u = (uint32_t)(s.out_list[0] + s.out_list[l * w + w - 1]);
        if (s.out_dc) g_sink_f = s.out_dc[0] + s.out_dc[l * w + w - 1];
        if (s.mask_of_query) g_sink_u = (uint32_t)(s.mask_of_query[0] + s.mask_of_query[l]);
    }
}

// field by field (the struct has padding: no memcmp)
static bool same(const SearchCall &x, const SearchCall &y)
{
    return x.nq == y.nq && x.d == y.d && x.K == y.K && x.w == y.w && x.q == y.q && x.ids == y.ids && x.dists == y.dists && x.counts == y.counts &&
           x.radii == y.radii && x.pre_list == y.pre_list && x.pre_dc == y.pre_dc && x.out_list == y.out_list && x.out_dc == y.out_dc &&
           x.mask_words == y.mask_words && x.mask_word_off == y.mask_word_off && x.mask_W == y.mask_W && x.mask_of_query == y.mask_of_query;
}

// the (x0, k) pairs inside a range of n queries: all of them for a handful (n <= 5: 15 pairs), else the edges
struct Pairs {
    int count = 0;
    int64_t x0[16], k[16];
    void add(int64_t a, int64_t b) { x0[count] = a; k[count] = b; ++count; }
};

static Pairs inner(int64_t n, bool all)
{
    Pairs r;
    if (all) {
        for (int64_t x0 = 0; x0 < n; ++x0)
            for (int64_t k = 1; x0 + k <= n; ++k) r.add(x0, k);
        return r;
    }
    r.add(0, n);
    r.add(0, 1);
    r.add(n - 1, 1);
    if (n > 1) r.add(1, n - 1);
    if (n > 2) r.add(n / 2, n - n / 2 - 1);
    return r;
}

static void check_shape(int64_t nq, int d, int K, int w, int rows)
{
    Arrays a;
    a.q.assign((size_t)nq * d, 1.0f);
    a.ids.assign((size_t)nq * K, 2u);
    a.dists.assign((size_t)nq * K, 3.0f);
    a.counts.assign((size_t)nq, 4);
    a.radii.assign((size_t)nq, 5.0f);
    a.pre_list.assign((size_t)nq * w, 6);
    a.pre_dc.assign((size_t)nq * w, 7.0f);
    a.out_list.assign((size_t)nq * w, 8);
    a.out_dc.assign((size_t)nq * w, 9.0f);
    a.moq.assign((size_t)nq, -1);
    a.words.assign(4, 0u);
    a.word_off.assign(2, 0u);
    SearchCall c{nq, d, K, w, a.q.data(), (rows & IDS) ? a.ids.data() : nullptr, (rows & DISTS) ? a.dists.data() : nullptr,
                 (rows & COUNTS) ? a.counts.data() : nullptr};
    CHECK(c.whole_batch && !c.pre() && !c.masked() && !c.radii && !c.out_list && !c.out_dc && !c.mask_of_query);
    if (rows & RADII) c.radii = a.radii.data();
    if (rows & PRE) { c.pre_list = a.pre_list.data(); c.pre_dc = a.pre_dc.data(); }
    if (rows & OUT) { c.out_list = a.out_list.data(); c.out_dc = a.out_dc.data(); }
    if (rows & MASK) { c.mask_words = a.words.data(); c.mask_word_off = a.word_off.data(); c.mask_W = 2; c.mask_of_query = a.moq.data(); }
    const bool small = nq <= 5;
    for (int64_t b0 = 0; b0 < nq; ++b0)
        for (int64_t n = 1; b0 + n <= nq; ++n) {
            const SearchCall s1 = c.slice(b0, n);                  // a sub-batch
            ++g_slices;
            check_slice(a, c, s1, b0, n);
            const Pairs gs = inner(n, small);
            for (int gi = 0; gi < gs.count; ++gi) {
                const std::pair<int64_t, int64_t> g{gs.x0[gi], gs.k[gi]};
                // a sort group of it: the slice of the call at the summed offset, which this loop checks against the flat index in its turn
                const SearchCall s2 = s1.slice(g.first, g.second);
                ++g_slices;
                CHECK(same(s2, c.slice(b0 + g.first, g.second)));
                CHECK(s2.whole_batch == (s1.whole_batch && g.first == 0 && g.second == n));
                const Pairs ys = inner(g.second, small);
                for (int yi = 0; yi < ys.count; ++yi) {
                    const std::pair<int64_t, int64_t> y{ys.x0[yi], ys.k[yi]};
                    const SearchCall s3 = s2.slice(y.first, y.second);   // a grid-y block of that
                    ++g_slices;
                    CHECK(same(s3, c.slice(b0 + g.first + y.first, y.second)));
                    CHECK(s3.whole_batch == (s2.whole_batch && y.first == 0 && y.second == g.second));
                }
            }
        }
    // a slice of a slice that was not the whole call never becomes "whole" again, even where it is all of its parent
    if (nq > 1) CHECK(!c.slice(0, nq - 1).slice(0, nq - 1).whole_batch && !c.slice(1, nq - 1).slice(0, nq - 1).whole_batch);
    CHECK(c.slice(0, nq).slice(0, nq).whole_batch);
    // the probe rows of a batch: [queries][w] each, from query g0 on; absent rows stay absent
    std::vector<int> pl((size_t)nq * w, 1);
    std::vector<float> pd((size_t)nq * w, 2.0f);
    std::vector<uint32_t> pb((size_t)nq * w, 3u);
    ProbeRows r;
    r.list = pl.data(); r.dc = (rows & PRE) ? pd.data() : nullptr; r.base = pb.data(); r.w = w;
    for (int64_t g0 = 0; g0 < nq; ++g0) {
        const ProbeRows s = r.slice(g0);
        CHECK(s.w == w && s.list == pl.data() + (size_t)g0 * w && s.base == pb.data() + (size_t)g0 * w);
        CHECK(s.dc == (r.dc ? pd.data() + (size_t)g0 * w : nullptr));
        g_sink_u = (uint32_t)s.list[0] + s.base[(size_t)(nq - g0) * w - 1];
        for (int64_t y0 = 0; g0 + y0 < nq; y0 += (small ? 1 : 17)) {
            const ProbeRows t = s.slice(y0), u = r.slice(g0 + y0);
            CHECK(t.list == u.list && t.dc == u.dc && t.base == u.base && t.w == u.w);
        }
    }
}

// ---- 2. sort groups: search_generic's old inline loop against range_plan::next_group ---------------------------------------------
// (tot: the u32 totals the device left; cap_keys and keys in int64_t, as the old code had them)
static int64_t old_next_group(const std::vector<uint32_t> &tot, int64_t g0, int64_t cap_keys, int64_t *keys_out)
{
    const int64_t na = (int64_t)tot.size();
    int64_t g1 = g0, keys = 0;
    while (g1 < na && (g1 == g0 || keys + tot[g1] <= cap_keys) && keys + tot[g1] < ((int64_t)1 << 32)) keys += tot[g1++];
    *keys_out = keys;
    return g1;
}

static long long g_groups = 0, g_tables = 0;

static void check_groups(const std::vector<uint32_t> &tot, int64_t cap_keys)
{
    ++g_tables;
    CHECK((int64_t)tot.size() <= range_plan::MAX_GRID_Y);   // the bound for_sort_groups asserts
    const std::vector<uint64_t> t64(tot.begin(), tot.end());
    for (int64_t g0 = 0; g0 < (int64_t)tot.size();) {
        int64_t ko = -1;
        uint64_t kn = ~(uint64_t)0;
        const int64_t go = old_next_group(tot, g0, cap_keys, &ko);
        const int64_t gn = range_plan::next_group(t64, g0, cap_keys, &kn);
        CHECK(go == gn && (uint64_t)ko == kn);
        ++g_groups;
        if (go == g0 || go != gn) break;   // (a query too large for one sort: both refuse it)
        g0 = go;
    }
}

static void check_group_tables()
{
    const uint32_t U = 0xFFFFFFFFu;
    const int64_t caps[] = {(int64_t)1 << 20, ((int64_t)1 << 20) + 7, (int64_t)1 << 33};   // (the last: only the 2^32 limit binds)
    for (int64_t cap : caps) {
        const uint32_t c = (uint32_t)std::min<int64_t>(cap, U);
        const uint32_t h = c / 2;
        std::vector<std::vector<uint32_t>> tables = {
            {0}, {1}, {c}, {c - 1}, {U},                                           // one query; U: sorted alone (2^32 - 1 keys)
            {h, c - h}, {h, c - h + 1}, {h, c - h - 1},                            // a pair on, above and below the cap
            {h, c - h, 0}, {h, c - h, 0, 0, 1}, {0, 0, h, 0, c - h, 0}, {0, 0, 0}, // runs of zeros before, inside, behind
            {c + 1}, {1, c + 1, 1}, {c + 1, c + 1}, {0, c + 1, 0},                 // a single total above the cap goes alone
            {c, 1}, {1, c}, {c - 1, 1, 1}, {1, 1, c - 2, 1},
            {U, 0}, {0, U}, {U - 1, 1}, {U - 1, 1, 0}, {U - 1, 2}, {1, U - 1}, {1, U},   // sums of 2^32 - 1 and of 2^32
            {0x80000000u, 0x7FFFFFFFu}, {0x80000000u, 0x80000000u}, {0x80000000u, 0x7FFFFFFFu, 1},
            {U, U, U}, {0, 0, U, 0, 0, 1, U},
        };
        for (const auto &t : tables) check_groups(t, cap);
        for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)65534, (int64_t)65535}) {
            check_groups(std::vector<uint32_t>((size_t)n, 0u), cap);                // one group of n queries without keys
            check_groups(std::vector<uint32_t>((size_t)n, 1u), cap);
            check_groups(std::vector<uint32_t>((size_t)n, 17u), cap);               // n * 17 passes 2^20: cut by the cap
            check_groups(std::vector<uint32_t>((size_t)n, c), cap);                 // every query a group of its own
            check_groups(std::vector<uint32_t>((size_t)n, 0x10000u), cap);          // 65 535 * 2^16 < 2^32 <= 65 536 * 2^16
            std::vector<uint32_t> t((size_t)n);
            uint64_t x = 88172645463325252ull;
            for (auto &v : t) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; v = (x & 7) ? (uint32_t)(x >> 40) % (c / 3 + 1) : 0u; }
            check_groups(t, cap);
            t.assign((size_t)n, 0u);
            t.back() = c;                                                           // zeros, then the cap exactly
            check_groups(t, cap);
            t.front() = 1;                                                          // ... and one above it
            check_groups(t, cap);
        }
    }
    // the one expression both paths take cap_keys from (what search_generic computed inline: max(2^20, ws_budget / 24))
    for (size_t ws : {(size_t)0, (size_t)1 << 20, (size_t)24 << 20, ((size_t)24 << 20) + 23, ((size_t)24 << 20) + 24, (size_t)8 << 30}) {
        const int64_t old_cap = std::max<int64_t>(1 << 20, (int64_t)(ws / 24));
        CHECK(range_plan::sort_cap_keys(ws) == old_cap);
        range_plan::Facts f;
        f.d = 8; f.m = 2; f.ksub = 256; f.kc = 16; f.n = 100; f.maxlen = 10; f.ws_budget = ws; f.lds_max = 160 << 10;
        CHECK(range_plan::make_plan(f, 4, 2).cap_keys == old_cap);
    }
}

int main()
{
    long long shapes = 0;
    for (int64_t nq : {1, 2, 5, 64, 65})
        for (int d : {1, 50})
            for (int K : {1, 10})
                for (int w : {1, 3})
                    for (int rows = 0; rows < ROWS_ALL; ++rows) {
                        check_shape(nq, d, K, w, rows);
                        ++shapes;
                    }
    check_group_tables();
    if (g_fail) {
        fprintf(stderr, "search_call_check: %d failures\n", g_fail);
        return 1;
    }
    printf("search_call_check ok: %lld shapes, %lld slices, %lld group tables, %lld groups\n", shapes, g_slices, g_tables, g_groups);
    return 0;
}
