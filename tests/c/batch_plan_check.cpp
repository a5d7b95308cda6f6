// Stand-alone check of csrc/batch_plan.h (tests/test_batch_plan.py builds it with -fsanitize=address,undefined and runs it directly).
//
// The schedule of ivfadc_search_batches used to be written out inside that function: which batches are non-empty, the upload groups, a
// group's byte range, the token numbering, the lookahead of the copy lane and the lane_done / ev_seen bookkeeping behind pending_event.
// Those loops are restated here literally ("old_*") and compared with the header over stride 1 and 2, nbat = 1 .. 60 and the counts
// around every change of the group width (252 k), with ragged batch sizes that put empty batches at the front, at the back and between
// groups, plus the all-zero and the empty run.  On top of the comparison: groups tile the batches and stay within MAX_GROUPS, byte ranges
// tile the run, the lookahead covers what a step reads, tokens are non-zero / bit 63 / distinct and a successor's token is that step's
// own, the tracker never names a group to a lane twice, the result block's offsets are the flat-index arithmetic in bytes and in words
// (rows * K above 2^31 included), and the device split tiles a batch in blocks whose sizes differ by at most one.
#include "../../ivfadc.jl_amd/csrc/batch_plan.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            if (++g_fail > 20) exit(1);                                       \
        }                                                                     \
    } while (0)

// ---- the old statement: the loops of ivfadc_search_batches as they stood -----------------------------------------------------------
static void old_batches(int nbatches, const int64_t *batch_nq, std::vector<int64_t> &start, std::vector<int64_t> &cnt, int64_t &total)
{
    total = 0;
    for (int b = 0; b < nbatches; ++b) total += batch_nq[b];
    start.clear();
    cnt.clear();
    int64_t run = 0;
    for (int b = 0; b < nbatches; ++b) {
        if (batch_nq[b] > 0) { start.push_back(run); cnt.push_back(batch_nq[b]); }
        run += batch_nq[b];
    }
}

static void old_groups(size_t nbat, size_t stride, std::vector<size_t> &gb, std::vector<size_t> &group_of)
{
    gb.clear();
    {
        const size_t per = std::max<size_t>(stride, (nbat + 251) / 252);
        size_t at = 0;
        while (at < nbat) {
            gb.push_back(at);
            at += (at < stride) ? 1 : per;
        }
        gb.push_back(nbat);
    }
    const size_t ngroups = gb.size() - 1;
    group_of.assign(nbat, 0);
    for (size_t g = 0; g < ngroups; ++g)
        for (size_t i = gb[g]; i < gb[g + 1]; ++i) group_of[i] = g;
}

static uint64_t old_token_of(uint64_t base, size_t i) { return (base + i + 1) | ((uint64_t)1 << 63); }

// the answers hipEventQuery gives, one bit per query, in the order the queries are made
struct Answers {
    uint64_t bits;
    int used = 0;
    bool next() { const bool f = (bits >> (used & 63)) & 1; ++used; return f; }
};

// pending_event and its two vectors: the group whose event the lane still has to wait for, or -1
struct OldPending {
    std::vector<size_t> group_of;
    std::vector<char> ev_seen;
    std::vector<size_t> lane_done = std::vector<size_t>(2, 0);
    size_t nbat;
    long pending_event(size_t lane_ix, size_t batch, Answers &ans)
    {
        long ev = -1;
        const size_t g = group_of[std::min(batch, nbat - 1)];
        if (lane_done[lane_ix] > g) return ev;
        if (!ev_seen[g]) {
            if (ans.next()) { for (size_t x = 0; x <= g; ++x) ev_seen[x] = 1; }
        }
        if (!ev_seen[g]) ev = (long)g;
        lane_done[lane_ix] = g + 1;
        return ev;
    }
};

// ... and the same question put to the header's tracker, as the host runtime puts it
static long new_pending(batch_plan::IngestTracker &tr, size_t lane, size_t batch, Answers &ans)
{
    const size_t g = tr.needs(lane, batch);
    if (g == batch_plan::IngestTracker::NOTHING) return -1;
    if (!tr.seen(g) && ans.next()) tr.fired(g);
    return tr.seen(g) ? -1 : (long)g;
}

// ---- inputs ------------------------------------------------------------------------------------------------------------------------
static std::vector<size_t> batch_counts()
{
    std::vector<size_t> v;
    for (size_t n = 1; n <= 60; ++n) v.push_back(n);
    for (size_t n : {251, 252, 253, 503, 504, 505, 755, 756, 757, 2000, 65536}) v.push_back(n);
    return v;
}

// ragged sizes with nbat non-empty batches.  form 0: no empty batch; 1: the cycle (1, 0, 2, 3, 0, 0, 1); 2: empty batches in front and
// behind; 3: an empty batch (two, every third time) behind the last batch of every upload group of `stride` lanes
static std::vector<int64_t> ragged(size_t nbat, size_t stride, int form)
{
    static const int64_t cyc[7] = {1, 0, 2, 3, 0, 0, 1};
    std::vector<int64_t> v;
    size_t have = 0;
    if (form == 2) v.assign(3, 0);
    if (form == 3) {
        std::vector<size_t> gb, group_of;   // (the old loop's groups: the input does not depend on the header under test)
        old_groups(nbat, stride, gb, group_of);
        for (size_t g = 0; g + 1 < gb.size(); ++g) {
            for (size_t i = gb[g]; i < gb[g + 1]; ++i) v.push_back(1 + (int64_t)(i % 5));
            v.push_back(0);
            if (g % 3 == 2) v.push_back(0);
        }
        return v;
    }
    for (size_t k = 0; have < nbat; ++k) {
        const int64_t s = form == 1 ? cyc[k % 7] : 1 + (int64_t)(k % 4);
        v.push_back(s);
        have += s > 0;
    }
    if (form == 2) v.insert(v.end(), 2, 0);
    return v;
}

static long long g_schedules = 0, g_groups = 0, g_steps = 0, g_tracker_runs = 0, g_blocks = 0, g_splits = 0;
static size_t g_max_groups = 0;

// ---- one run: batches, groups, byte ranges, lookahead, tokens ------------------------------------------------------------------------
static void check_schedule(const std::vector<int64_t> &sizes, size_t want_nbat, size_t stride, uint64_t base)
{
    std::vector<int64_t> ostart, ocnt;
    int64_t ototal;
    old_batches((int)sizes.size(), sizes.data(), ostart, ocnt, ototal);
    batch_plan::Batches bt;
    CHECK(batch_plan::non_empty_batches(sizes.data(), (int)sizes.size(), bt) == -1);
    CHECK(bt.start == ostart && bt.cnt == ocnt && bt.total == ototal && bt.size() == want_nbat);
    const size_t nbat = bt.size();

    std::vector<size_t> gb, group_of;
    old_groups(nbat, stride, gb, group_of);
    const batch_plan::Groups gr = batch_plan::upload_groups(nbat, stride);
    CHECK(gr.first == gb && gr.of == group_of && gr.size() == gb.size() - 1);
    const size_t ngroups = gr.size();
    CHECK(ngroups <= batch_plan::MAX_GROUPS);
    g_max_groups = std::max(g_max_groups, ngroups);
    g_groups += (long long)ngroups;
    // non-empty, contiguous, tiling [0, nbat); the first `stride` groups are single batches
    CHECK(gr.first.front() == 0 && gr.first.back() == nbat);
    for (size_t g = 0; g < ngroups; ++g) {
        CHECK(gr.first[g] < gr.first[g + 1]);
        if (g < stride) CHECK(gr.first[g + 1] - gr.first[g] == 1);
        for (size_t i = gr.first[g]; i < gr.first[g + 1]; ++i) CHECK(gr.of[i] == g);
    }
    // byte ranges: the old expressions, and consecutive groups tile the run with no gap and no overlap
    for (size_t d : {(size_t)1, (size_t)128}) {
        size_t at = 0;
        for (size_t g = 0; g < ngroups; ++g) {
            const size_t b0 = gb[g], b1 = gb[g + 1];
            const size_t off = (size_t)ostart[b0] * d * 4;
            const size_t bytes = ((size_t)ostart[b1 - 1] + (size_t)ocnt[b1 - 1] - (size_t)ostart[b0]) * d * 4;
            const batch_plan::ByteRange r = batch_plan::group_bytes(bt, gr, g, d * 4);
            CHECK(r.off == off && r.bytes == bytes);
            CHECK(r.off == at && r.bytes > 0);
            at = r.off + r.bytes;
        }
        CHECK(at == (size_t)bt.total * d * 4);
    }
    // the steps
    size_t up_next = 0;   // the upload mark, as upload_until moves it
    std::vector<uint64_t> tokens;
    for (size_t i = 0; i < nbat; ++i) {
        const batch_plan::Step st = batch_plan::step_of(i, nbat, stride, base);
        ++g_steps;
        CHECK(st.lane == ((stride == 2 && (i & 1)) ? 1u : 0u));
        CHECK(st.token == old_token_of(base, i) && st.token != 0 && (st.token >> 63) == 1);
        CHECK(st.has_next == (i + stride < nbat));
        if (st.has_next) {
            CHECK(st.next == i + stride && st.next_token == old_token_of(base, i + stride));
            CHECK(st.next_token == batch_plan::step_of(st.next, nbat, stride, base).token);
            CHECK(batch_plan::step_of(st.next, nbat, stride, base).lane == st.lane);
        } else {
            CHECK(i + stride >= nbat);
        }
        CHECK(st.on_their_way == i + 2 * stride + 1);
        const size_t last = std::min(st.on_their_way, nbat);
        while (up_next < ngroups && gb[up_next] < last) ++up_next;
        CHECK(group_of[i] < up_next && group_of[std::min(i + stride, nbat - 1)] < up_next);
        tokens.push_back(st.token);
    }
    CHECK(nbat == 0 || up_next == ngroups);
    std::sort(tokens.begin(), tokens.end());
    CHECK(std::adjacent_find(tokens.begin(), tokens.end()) == tokens.end());
    ++g_schedules;
}

// ---- the tracker against lane_done / ev_seen, under one pattern of answers ------------------------------------------------------------
// returns the number of event queries the run made
static int check_tracker(size_t nbat, size_t stride, uint64_t pattern)
{
    OldPending old;
    std::vector<size_t> gb;
    old_groups(nbat, stride, gb, old.group_of);
    old.ev_seen.assign(gb.size() - 1, 0);
    old.nbat = nbat;
    const batch_plan::Groups gr = batch_plan::upload_groups(nbat, stride);
    batch_plan::IngestTracker tr(gr);
    Answers ao{pattern}, an{pattern};
    long told[2] = {-1, -1};   // the newest group each lane was named
    for (size_t i = 0; i < nbat; ++i) {
        const batch_plan::Step st = batch_plan::step_of(i, nbat, stride, 0);
        const size_t asks[2] = {i, st.next};
        for (int k = 0; k < (st.has_next ? 2 : 1); ++k) {
            const long o = old.pending_event(st.lane, asks[k], ao), n = new_pending(tr, st.lane, asks[k], an);
            CHECK(o == n && ao.used == an.used);
            if (n >= 0) {
                CHECK(n > told[st.lane]);   // never a group the lane was named before (nor one it covers)
                told[st.lane] = n;
            }
        }
    }
    // a batch past the end is clamped to the last one
    {
        const long o = old.pending_event(0, nbat + 5, ao), n = new_pending(tr, 0, nbat + 5, an);
        CHECK(o == n);
    }
    for (size_t g = 0; g < gr.size(); ++g) CHECK(tr.seen(g) == (old.ev_seen[g] != 0));
    ++g_tracker_runs;
    return an.used;
}

// ---- the result block ---------------------------------------------------------------------------------------------------------------
static void check_block(uint64_t rows, uint64_t K)
{
    const batch_plan::ResultBlock w = batch_plan::result_words((size_t)rows, (size_t)K), b = batch_plan::result_bytes((size_t)rows, (size_t)K);
    // flat indices: ids[r][k] at r * K + k, dists behind the rows * K ids, counts behind both
    CHECK(w.ids == 0 && (uint64_t)w.dists == rows * K && (uint64_t)w.counts == 2 * rows * K && (uint64_t)w.total == 2 * rows * K + rows);
    CHECK(b.ids == 4 * w.ids && b.dists == 4 * w.dists && b.counts == 4 * w.counts && b.total == 4 * w.total);
    CHECK((uint64_t)w.ids_len() == rows * K && (uint64_t)w.counts_len() == rows);
    CHECK((uint64_t)b.ids_len() == 4 * rows * K && (uint64_t)b.counts_len() == 4 * rows);
    ++g_blocks;
}

int main()
{
    static_assert(sizeof(size_t) == 8, "offsets are 64 bits wide");
    const uint64_t bases[] = {0, 1, 699, ((uint64_t)1 << 63) - 1, UINT64_MAX - 2};
    for (size_t stride : {(size_t)1, (size_t)2})
        for (size_t nbat : batch_counts())
            for (int form = 0; form < 4; ++form) check_schedule(ragged(nbat, stride, form), nbat, stride, bases[(nbat + (size_t)form) % 5]);
    // the all-zero run and the empty run
    for (size_t stride : {(size_t)1, (size_t)2}) {
        check_schedule(std::vector<int64_t>(9, 0), 0, stride, 0);
        check_schedule(std::vector<int64_t>(), 0, stride, 0);
    }
    // a negative size is reported, the first one
    {
        const int64_t bad[5] = {3, 0, -1, 2, -7};
        batch_plan::Batches bt;
        CHECK(batch_plan::non_empty_batches(bad, 5, bt) == 2);
    }
    CHECK(g_max_groups == 254);   // what the old loop peaks at over these counts

    // every pattern of answers over small runs, pseudo-random ones over runs whose groups hold several batches
    for (size_t stride : {(size_t)1, (size_t)2})
        for (size_t nbat = 1; nbat <= 7; ++nbat) {
            const int queries = check_tracker(nbat, stride, 0);   // nothing ever fires: the most queries a run can make
            CHECK(queries <= 14);
            for (uint64_t p = 1; p < ((uint64_t)1 << queries); ++p) check_tracker(nbat, stride, p);
        }
    for (size_t stride : {(size_t)1, (size_t)2})
        for (size_t nbat : {505, 757, 2000}) {
            uint64_t x = 0x9E3779B97F4A7C15ull * (nbat + stride);
            for (int t = 0; t < 64; ++t) {
                x = x * 6364136223846793005ull + 1442695040888963407ull;
                check_tracker(nbat, stride, t == 0 ? 0 : t == 1 ? ~(uint64_t)0 : x & ((x >> 7) | (x << 3)));
            }
        }

    for (uint64_t rows : {0, 1, 5, 1024, 65537})
        for (uint64_t K : {1, 10, 128, 2048}) check_block(rows, K);
    // rows * K just above 2^31: an int product would show
    const uint64_t big[3][2] = {{214748365, 10}, {((uint64_t)1 << 20) + 1, 2048}, {((uint64_t)1 << 31) + 1, 1}};
    for (const auto &rk : big) {
        const uint64_t rows = rk[0], K = rk[1];
        CHECK(rows * K > (uint64_t)INT_MAX && rows * K < ((uint64_t)1 << 31) + 4096);
        check_block(rows, K);
        CHECK(batch_plan::result_words((size_t)rows, (size_t)K).dists > (size_t)INT_MAX);
    }

    for (int64_t nq = 0; nq <= 70; ++nq)
        for (int64_t G = 1; G <= 9; ++G) {
            CHECK(batch_plan::mg_lo(0, nq, G) == 0 && batch_plan::mg_lo(G, nq, G) == nq);
            int64_t lo = INT64_MAX, hi = 0;
            for (int64_t r = 0; r < G; ++r) {
                const int64_t a = batch_plan::mg_lo(r, nq, G), b = batch_plan::mg_lo(r + 1, nq, G);
                CHECK(a <= b);   // (contiguous by construction: block r ends where block r + 1 begins)
                lo = std::min(lo, b - a);
                hi = std::max(hi, b - a);
            }
            CHECK(hi - lo <= 1 && (lo == 0) == (nq < G));
            ++g_splits;
        }

    if (g_fail) {
        fprintf(stderr, "batch_plan_check: %d checks failed\n", g_fail);
        return 1;
    }
    printf("batch_plan_check ok: %lld schedules, %lld groups, %lld steps, %lld tracker runs, %lld blocks, %lld splits\n", g_schedules,
           g_groups, g_steps, g_tracker_runs, g_blocks, g_splits);
    return 0;
}
