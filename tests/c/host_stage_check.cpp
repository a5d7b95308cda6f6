// Stand-alone check of csrc/host_stage.h: the arena's layout, the counts check, the id span of a score call and the row compaction of the
// re-rank host entries, each against a naive restatement on arrays of exactly the size the entries hand over (a wrong index is an
// AddressSanitizer report).  Build with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../ivfadc.jl_amd/csrc/host_stage.h"

using namespace host_stage;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static long long g_cases = 0;

// ---- layout: every sequence of 1 .. 8 parts with lengths from LENS ---------------------------------------------------------------------
static const size_t LENS[] = {0, 1, 15, 255, 256, 257, ((size_t)1 << 20) + 3};
static void check_layout(const size_t *len, int n)
{
    Layout lay;
    size_t sum = 0;
    for (int i = 0; i < n; ++i) {
        CHECK(lay.add(len[i]) == i);
        sum += len[i];
    }
    CHECK(!lay.overflow && lay.parts == n && lay.total >= sum && lay.total <= sum + ALIGN * (size_t)n);
    for (int i = 0; i < n; ++i) {
        CHECK(lay.len[i] == len[i] && lay.off[i] % ALIGN == 0 && lay.off[i] + len[i] <= lay.total);
        if (i > 0) CHECK(lay.off[i] >= lay.off[i - 1] + len[i - 1]);   // in order, disjoint (a part of no bytes shares its offset with nobody's bytes)
    }
    ++g_cases;
}
static void layouts(size_t *len, int at, int n)
{
    if (at == n) return check_layout(len, n);
    for (size_t l : LENS) {
        len[at] = l;
        layouts(len, at + 1, n);
    }
}
static void check_layout_refusals()
{
    const size_t top = ~(size_t)0;
    for (size_t big : {top, top - 1, top - 254, top - 255, top - 256}) {
        Layout a;   // alone: fits exactly when its rounded length does
        a.add(big);
        CHECK(a.overflow == (big > top - 255));
        Layout b;   // behind a part: the sum never fits
        b.add(1);
        b.add(big);
        CHECK(b.overflow && b.parts == 1 && b.total == ALIGN);
        Layout c;   // two halves
        c.add(top / 2 + 1);
        CHECK(!c.overflow);
        c.add(top / 2 + 1);
        CHECK(c.overflow);
        g_cases += 3;
    }
    Layout d;   // a ninth part
    for (int i = 0; i < MAX_PARTS; ++i) d.add(4);
    CHECK(!d.overflow && d.parts == MAX_PARTS);
    const int at = d.add(4);
    CHECK(d.overflow && d.parts == MAX_PARTS && at >= 0 && at < MAX_PARTS);
    ++g_cases;
}

// ---- counts ------------------------------------------------------------------------------------------------------------------------------
static int64_t naive_bad_count(const std::vector<int32_t> &c, int64_t C)
{
    for (size_t q = 0; q < c.size(); ++q)
        if (c[q] < 0 || c[q] > C) return (int64_t)q;
    return -1;
}
static void check_counts()
{
    for (int64_t C : {(int64_t)0, (int64_t)1, (int64_t)7, (int64_t)0x7FFFFFFF})
        for (int nq : {1, 2, 9, 64}) {
            std::vector<int32_t> good((size_t)nq);
            for (int q = 0; q < nq; ++q) good[(size_t)q] = (int32_t)((int64_t)(q * 5) % (C + 1));
            good[0] = (int32_t)C;   // the largest legal count
            CHECK(first_bad_count(good.data(), nq, C) == -1 && naive_bad_count(good, C) == -1);
            CHECK(first_bad_count(nullptr, nq, C) == -1 && first_bad_count(good.data(), 0, C) == -1);
            g_cases += 2;
            for (int at : {0, nq / 2, nq - 1})
                for (int64_t bad : {(int64_t)-1, (int64_t)-0x80000000LL, C + 1}) {
                    if (bad > 0x7FFFFFFF) continue;   // (C = 2^31 - 1: no count lies above)
                    std::vector<int32_t> c = good;
                    c[(size_t)at] = (int32_t)bad;
                    if (at + 1 < nq) c[(size_t)nq - 1] = -7;   // a later offender is not the one named
                    CHECK(first_bad_count(c.data(), nq, C) == at && naive_bad_count(c, C) == at);
                    ++g_cases;
                }
        }
}

// ---- id span ---------------------------------------------------------------------------------------------------------------------------
// the restatement: every (query, slot) pair the kernel would read an id for
static IdSpan naive_span(int64_t nq, int64_t C, bool shared, const std::vector<uint32_t> &ids, const int32_t *counts)
{
    IdSpan s{false, 0u, 0u};
    for (int64_t q = 0; q < nq; ++q)
        for (int64_t j = 0; j < C; ++j) {
            if (counts && j >= counts[q]) continue;
            const uint32_t id = ids.at((size_t)(shared ? j : q * C + j));
            if (!s.any) s = IdSpan{true, id, id};
            if (id < s.lo) s.lo = id;
            if (id > s.hi) s.hi = id;
        }
    return s;
}
static void check_span()
{
    uint32_t x = 12345u;
    const auto next = [&]() { x = x * 1664525u + 1013904223u; return x; };
    for (int shared = 0; shared < 2; ++shared)
        for (int64_t nq : {(int64_t)1, (int64_t)3, (int64_t)17})
            for (int64_t C : {(int64_t)1, (int64_t)5, (int64_t)33})
                for (int fill = 0; fill < 4; ++fill) {
                    std::vector<uint32_t> ids((size_t)(shared ? C : nq * C));   // exactly what the caller hands over
                    for (uint32_t &v : ids) v = fill == 0 ? next() : 1000u + next() % 50u;
                    if (fill == 2) ids.front() = 0u, ids.back() = 0xFFFFFFFFu;   // the ends of the id space, in the first and the last slot
                    if (fill == 3) ids[ids.size() / 2] = 0xFFFFFFFFu, ids.back() = 0u;
                    std::vector<int32_t> zero((size_t)nq, 0), mixed((size_t)nq), full((size_t)nq, (int32_t)C);
                    for (int64_t q = 0; q < nq; ++q) mixed[(size_t)q] = (int32_t)(next() % (uint32_t)(C + 1));
                    for (const int32_t *counts : {(const int32_t *)nullptr, (const int32_t *)zero.data(), (const int32_t *)mixed.data(), (const int32_t *)full.data()}) {
                        const IdSpan got = live_id_span(nq, C, shared != 0, ids.data(), counts), want = naive_span(nq, C, shared != 0, ids, counts);
                        CHECK(got.any == want.any && got.lo == want.lo && got.hi == want.hi);
                        if (counts == zero.data()) CHECK(!got.any && got.lo == 0u && got.hi == 0u);   // no live slot: a span of one id
                        if (!counts && fill >= 2 && ids.size() > 2) CHECK(got.lo == 0u && got.hi == 0xFFFFFFFFu);
                        ++g_cases;
                    }
                }
}

// ---- compaction --------------------------------------------------------------------------------------------------------------------------
static void check_compact()
{
    const uint32_t CANARY = 0xDEADBEEFu;
    for (int K : {1, 3, 10})
        for (int Kw : {1, K - 1, K}) {
            if (Kw < 1) continue;
            const int32_t CNT[] = {0, Kw, Kw + 1, 0x7FFFFFFF, -1, (int32_t)-0x80000000LL, Kw / 2, 1};
            const int64_t nq = (int64_t)(sizeof(CNT) / sizeof(CNT[0]));
            std::vector<int32_t> counts(CNT, CNT + nq);
            std::vector<uint32_t> src((size_t)nq * (size_t)Kw), dst((size_t)nq * (size_t)K, CANARY);
            for (size_t i = 0; i < src.size(); ++i) src[i] = (uint32_t)i + 1u;
            compact_rows(nq, Kw, K, counts.data(), src.data(), dst.data());
            for (int64_t q = 0; q < nq; ++q) {
                const int cnt = counts[(size_t)q] < 0 ? 0 : counts[(size_t)q] > Kw ? Kw : counts[(size_t)q];
                for (int j = 0; j < K; ++j)
                    CHECK(dst[(size_t)q * (size_t)K + (size_t)j] == (j < cnt ? src[(size_t)q * (size_t)Kw + (size_t)j] : CANARY));
                ++g_cases;
            }
            compact_rows(0, Kw, K, nullptr, nullptr, nullptr);   // no query: nothing is read
        }
}

int main()
{
    size_t len[MAX_PARTS];
    for (int n = 1; n <= 8; ++n) layouts(len, 0, n);
    check_layout_refusals();
    check_counts();
    check_span();
    check_compact();
    printf("host_stage_check ok: %lld cases\n", g_cases);
    return 0;
}
