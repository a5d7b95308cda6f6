// The cases the search planner is checked on, and the one line a case is printed as.  Templated on the facts and plan types and free of
// any include of the library's, so that the very same grid and printer can be compiled against another revision's planner (a scratch
// program around an older ivfadc_hip.hip, whose make_plan takes a handle) and the two outputs compared byte for byte: that is how
// tests/plan_table.tsv was produced and how a pull request that moves planner code proves it changed no plan.
//
//   plan_grid<F>(visit)    every case: visit(const F &facts, int64_t nq, int K, int w, bool pre)
//   plan_pairs<F>(visit)   the curated part alone: the BASELINE shapes at bench.py's batch sizes and both sides of every threshold
//   plan_line(buf, ...)    the TSV line of a case and its plan (PLAN_COLUMNS names the fields)
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

namespace plan_grid_ns {

#define PLAN_COLUMNS                                                                                                                       \
    "u16\td\tkc\tm\tdsub\tksub\tn\tmaxlen\tnum_cu\tallow_filt\tallow_lb\tforce_lb\tallow_nf\tallow_prune\tallow_mfma\tmfma_min_kc\twg8_mode\t" \
    "wg8_wide\tu16_tables\tpart_n\tforce_qg\tforce_chunk\tws_budget\ttl_use\ttl_G\tprune_est\thave_lb\thave_nf\tlanes_active\tnq\tK\tw\tpre\t"  \
    "form\tstripe\tq8\twide\tthreads\tcoarse_mfma\tfuse_topw\tlanes\ttwolevel\tsmall_k\tsmall_w\tqg\tcap\tcapw\tmaxch\tCH\tlds\tnb\tfits\t"     \
    "striped\tquery_major"
constexpr int PLAN_INPUT_FIELDS = 33;

// the inputs of a case, then every Plan field but fn, striped() and query_major()
template <class F, class P> int plan_line(char *buf, size_t cap, const F &f, int64_t nq, int K, int w, bool pre, const P &p)
{
    return snprintf(buf, cap,
                    "%d\t%d\t%d\t%d\t%d\t%d\t%lld\t%lld\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%llu\t%d\t%d\t%g\t%d\t%d\t%d\t%lld\t%d\t%d\t%d\t"
                    "%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%u\t%llu\t%lld\t%d\t%d\t%d",
                    (int)f.u16, f.d, f.kc, f.m, f.dsub, f.ksub, (long long)f.n, (long long)f.maxlen, f.num_cu, (int)f.allow_filt, (int)f.allow_lb,
                    (int)f.force_lb, (int)f.allow_nf, (int)f.allow_prune, (int)f.allow_mfma, f.mfma_min_kc, f.wg8_mode, (int)f.wg8_wide, f.u16_tables,
                    f.part_n, f.force_qg, f.force_chunk, (unsigned long long)f.ws_budget, (int)f.tl_use, f.tl_G, (double)f.prune_est,
                    (int)f.have_lb_operands, (int)f.have_nf_operands, (int)f.lanes_active, (long long)nq, K, w, (int)pre,
                    (int)p.form, (int)p.stripe, (int)p.q8, (int)p.wide, p.threads, (int)p.coarse_mfma, (int)p.fuse_topw, (int)p.lanes, (int)p.twolevel,
                    (int)p.small_k, (int)p.small_w, p.qg, p.cap, p.capw, p.maxch, (unsigned)p.CH, (unsigned long long)p.lds, (long long)p.nb,
                    (int)p.fits, p.striped(), (int)p.query_major());
}

// the inputs of a line back into a case (the first PLAN_INPUT_FIELDS fields); false: not such a line
template <class F> bool plan_parse(const char *line, F &f, int64_t &nq, int &K, int &w, bool &pre)
{
    const char *fld[PLAN_INPUT_FIELDS];
    const char *s = line;
    for (int i = 0; i < PLAN_INPUT_FIELDS; ++i) {
        fld[i] = s;
        s = strchr(s, '\t');
        if (!s) return false;
        ++s;
    }
    int i = 0;
    auto I = [&] { return atoi(fld[i++]); };
    auto L = [&] { return (int64_t)atoll(fld[i++]); };
    f = F{};
    f.u16 = I(); f.d = I(); f.kc = I(); f.m = I(); f.dsub = I(); f.ksub = I();
    f.n = L(); f.maxlen = L(); f.num_cu = I();
    f.allow_filt = I(); f.allow_lb = I(); f.force_lb = I(); f.allow_nf = I(); f.allow_prune = I();
    f.allow_mfma = I(); f.mfma_min_kc = I(); f.wg8_mode = I(); f.wg8_wide = I(); f.u16_tables = I();
    f.part_n = I(); f.force_qg = I(); f.force_chunk = I();
    f.ws_budget = (size_t)strtoull(fld[i++], nullptr, 10);
    f.tl_use = I(); f.tl_G = I(); f.prune_est = strtof(fld[i++], nullptr);
    f.have_lb_operands = I(); f.have_nf_operands = I(); f.lanes_active = I();
    nq = L(); K = I(); w = I(); pre = I();
    return i == PLAN_INPUT_FIELDS;
}

// ---- the setters of include/ivfadc_hip.h, as they write the facts ---------------------------------------------------------------------
template <class F> void set_table_mode(F &f, int mode)   // ivfadc_set_table_mode
{
    f.allow_filt = mode != 1;
    f.force_lb = mode == 2 || mode == 4;
    f.wg8_mode = mode == 5 ? -1 : (mode == 6 || mode == 8 ? 1 : (mode == 7 || mode == 9 ? 2 : 0));
    f.wg8_wide = mode == 8 || mode == 9;
}
template <class F> void set_coarse_mode(F &f, int mode)   // ivfadc_set_coarse_mode: what of it the planner sees
{
    f.allow_mfma = mode != 1;
    f.mfma_min_kc = mode == 2 ? 128 : 2048;
}

// ---- shapes ------------------------------------------------------------------------------------------------------------------------
struct Shape { bool u16; int d, kc, m, dsub, ksub; int64_t n, maxlen; };
template <class F> F facts_of(const Shape &s)
{
    F f{};
    f.u16 = s.u16; f.d = s.d; f.kc = s.kc; f.m = s.m; f.dsub = s.dsub; f.ksub = s.ksub; f.n = s.n; f.maxlen = s.maxlen;
    f.num_cu = 256;
    // the operands ivfadc_create builds for the shapes that have the kernels
    f.have_lb_operands = !s.u16 && ((s.m == 48 && s.dsub == 16) || (s.m == 16 && s.dsub == 6));
    f.have_nf_operands = !s.u16 && s.m == 8 && s.dsub == 16;
    return f;
}
// the five BASELINE shapes of bench.py (n, kc as there; the longest list as its synthetic sizes come out, to a few points)
constexpr Shape BASELINE[5] = {
    {false, 50, 100, 10, 5, 256, 1000, 25},                    // toy
    {false, 128, 1024, 8, 16, 256, 1000000, 2600},             // sift1m
    {false, 96, 65536, 16, 6, 256, 100000000, 1700},           // deep1b
    {false, 128, 8192, 8, 16, 256, 1000000000, 123600},        // sift1b
    {false, 768, 4096, 48, 16, 256, 10000000, 2650},           // hd
};
// every other (m, dsub) a kernel is specialised on, shapes only the generic kernels serve, UInt16 handles; n and maxlen come from LENGTHS
constexpr Shape OTHERS[] = {
    {false, 32, 8192, 8, 4, 256, 0, 0},    {false, 64, 8192, 8, 8, 256, 0, 0},     {false, 96, 1024, 8, 12, 256, 0, 0},
    {false, 128, 512, 8, 16, 256, 0, 0},   {false, 64, 8192, 16, 4, 256, 0, 0},    {false, 96, 4096, 16, 6, 256, 0, 0},
    {false, 128, 8192, 16, 8, 256, 0, 0},  {false, 768, 16384, 48, 16, 256, 0, 0}, {false, 15, 1024, 5, 3, 256, 0, 0},
    {false, 20, 300, 5, 4, 256, 0, 0},     {false, 8, 2048, 1, 8, 256, 0, 0},      {false, 130, 1024, 10, 13, 200, 0, 0},
    {true, 32, 1024, 4, 8, 1024, 0, 0},    {true, 2048, 512, 64, 32, 1024, 0, 0},  {true, 32, 4096, 4, 8, 65536, 0, 0},
    {true, 3072, 256, 64, 48, 65536, 0, 0}, {true, 1024, 1024, 32, 32, 4096, 0, 0},
};
// average list lengths: both sides of 3072 (shared), 8192 (eight-wave), 1024 and 1025 (UInt16 table-free rule at ksub = 1024, a pass),
// short lists; 64 KiB / m and 256 KiB / m are added per shape
constexpr int64_t LENGTHS[] = {40, 1024, 1025, 3071, 3072, 8191, 8192, 70000};
constexpr int64_t NQS_FIXED[] = {1, 32, 64, 65, 16384, 65536, ((int64_t)1 << 22) + 1};
constexpr int KS[] = {1, 10, 64, 65, 100, 128, 129, 1000, 1984, 2048};
constexpr int WS[] = {1, 2, 3, 7, 8, 32, 33, 48, 49, 64, 65, 128};
constexpr int TUNE_QG[] = {0, -1, -2, -3, 1, 2, 4, 8};
constexpr int TUNE_CHUNK[] = {0, 1024, 2048};

template <class T, size_t N> constexpr size_t count_of(const T (&)[N]) { return N; }

// the shapes with their list lengths: `visit(facts)`
template <class F, class V> void each_context(V visit)
{
    for (const Shape &s : BASELINE) visit(facts_of<F>(s));
    for (const Shape &s : OTHERS) {
        int64_t lens[count_of(LENGTHS) + 4];
        size_t nl = 0;
        for (int64_t l : LENGTHS) lens[nl++] = l;
        lens[nl++] = 65536 / s.m - 1; lens[nl++] = 65536 / s.m;       // few_heavy: avg_len * m >= 64 KiB
        lens[nl++] = 262144 / s.m;    lens[nl++] = 262144 / s.m + 1;  // long_lists: avg_len * m > 256 KiB
        for (size_t i = 0; i < nl; ++i) {
            Shape t = s;
            t.n = lens[i] * s.kc;
            t.maxlen = lens[i] + lens[i] / 8 + 8;
            visit(facts_of<F>(t));
        }
        // the eight-wave kernel's 28- and 27-bit list positions: the longest list on both sides of each
        for (int64_t ml : {((int64_t)1 << 27) - 1, (int64_t)1 << 27, ((int64_t)1 << 28) - 1, (int64_t)1 << 28}) {
            Shape t = s;
            t.n = 70000 * (int64_t)s.kc;
            t.maxlen = ml;
            visit(facts_of<F>(t));
        }
    }
}

// one switch group at a time off the defaults: `visit(facts)`
template <class F, class V> void each_config(const F &base, V visit)
{
    visit(base);
    for (int qg : TUNE_QG)
        for (int ch : TUNE_CHUNK) {
            if (qg == 0 && ch == 0) continue;
            F f = base; f.force_qg = qg; f.force_chunk = ch; visit(f);
        }
    for (int mode = 1; mode <= 10; ++mode) { F f = base; set_table_mode(f, mode); visit(f); }
    for (int mode : {1, 2}) { F f = base; set_coarse_mode(f, mode); visit(f); }
    for (int t : {1, 2}) { F f = base; f.u16_tables = t; visit(f); }
    { F f = base; f.part_n = 2; visit(f); }
    { F f = base; f.part_n = 2; set_table_mode(f, 6); visit(f); }
    for (float pe : {0.59f, 0.6f}) { F f = base; f.prune_est = pe; visit(f); }
    { F f = base; f.prune_est = 0.6f; f.allow_prune = false; visit(f); }
    { F f = base; f.lanes_active = true; visit(f); }
    for (int G : {64, 4096}) { F f = base; f.tl_use = true; f.tl_G = G; visit(f); }
    { F f = base; f.tl_use = false; f.tl_G = 256; visit(f); }
    { F f = base; f.ws_budget = (size_t)1 << 20; visit(f); }
    { F f = base; f.allow_lb = false; visit(f); }
    { F f = base; f.allow_nf = false; f.force_qg = 8; visit(f); }
    { F f = base; f.have_lb_operands = false; f.have_nf_operands = false; f.force_qg = 8; set_table_mode(f, 2); visit(f); }
}

template <class V> void each_nq(int num_cu, V visit)
{
    for (int64_t nq : NQS_FIXED) visit(nq);
    for (int64_t nq : {(int64_t)num_cu / 4, (int64_t)num_cu, (int64_t)4 * num_cu}) visit(nq);
}

struct Rng {   // splitmix64: the same sequence wherever it is compiled
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    size_t below(size_t n) { return (size_t)(next() % n); }
    template <class T, size_t N> T pick(const T (&a)[N]) { return a[below(N)]; }
};

// The curated part: the BASELINE shapes at the batch sizes bench.py runs, and a pair of cases on both sides of each threshold of the rules.
template <class F, class V> void plan_pairs(V visit)
{
    const F toy = facts_of<F>(BASELINE[0]), sift1m = facts_of<F>(BASELINE[1]), deep1b = facts_of<F>(BASELINE[2]), sift1b = facts_of<F>(BASELINE[3]),
            hd = facts_of<F>(BASELINE[4]);
    for (int K : {1, 10, 100}) {
        visit(toy, 64, K, 1, false);
        visit(sift1m, 1024, K, 8, false);
        visit(deep1b, 10000, K, 32, false);
        visit(sift1b, 16384, K, 8, false);
        visit(sift1b, 16384, K, 1, false);
        visit(sift1b, 2048, K, 8, false);
        visit(hd, 4096, K, 8, false);
    }
    for (const F &b : {sift1m, deep1b, sift1b, hd}) {   // the second lane, the caller's probes, the two-level search, the feedback on both sides of 0.6
        { F f = b; f.lanes_active = true; visit(f, b.kc == 1024 ? 1024 : 4096, 10, 8, false); visit(f, 1023, 10, 8, false); }
        visit(b, 4096, 10, 8, true);
        { F f = b; f.tl_use = true; f.tl_G = 512; visit(f, 4096, 10, 32, false); visit(f, 4096, 10, 64, false); visit(f, 4096, 10, 65, false); }
        for (float pe : {0.59f, 0.6f}) { F f = b; f.prune_est = pe; visit(f, 1024, 10, 8, false); }
    }
    // K at the selectors' and the pools' edges, w at the matrix-core rounds' (2 / 3, 32 / 33), the filter's (48 / 49) and the registers' (64 / 65)
    for (int K : {64, 65, 128, 129, 1984, 2048})
    {
        for (int mode : {0, 8, 9}) {
            if (mode == 9 && K != 128) continue;
            F f = sift1b; set_table_mode(f, mode); visit(f, 16384, K, 8, false);
        }
        visit(hd, 4096, K, 8, false);   // (no eight-wave kernel at m = 48: the table mode cannot matter)
    }
    for (int w : {1, 2, 3, 7, 8, 32, 33, 48, 49, 64, 65, 128}) visit(hd, 4096, 10, w, false);
    for (int w : {7, 8}) { visit(hd, 64, 10, w, false); visit(sift1m, 1, 10, w, false); }   // few heavy probes / a few queries with many
    for (int w : {2, 3, 32, 33}) { F f = deep1b; set_table_mode(f, 2); visit(f, 10000, 10, w, false); }   // the matrix-core rounds on request
    for (int w : {48, 49})
        for (int mode : {0, 1, 2}) { F f = sift1m; set_coarse_mode(f, mode); visit(f, 1024, 10, w, false); visit(hd, 4096, 10, w, false); }
    // batch sizes around a quarter of the chip, the chip, four times the chip
    for (int64_t nq : {63, 64, 65, 255, 256, 257, 1023, 1024}) {
        visit(hd, nq, 10, 8, false);
        visit(sift1m, nq, 10, 16, false);
        if (nq >= 1023) { F f = hd; f.lanes_active = true; visit(f, nq, 10, 8, false); }
    }
    // list lengths: shared (3072), the eight-wave kernel (8192), long lists (256 KiB / m), heavy probes (64 KiB / m); its longest lists
    for (int64_t len : {3071, 3072, 8191, 8192, 32768, 32769}) {
        F f = facts_of<F>(Shape{false, 128, 8192, 8, 16, 256, len * 8192, len + len / 8});
        visit(f, 16384, 10, 8, false);
        visit(f, 2048, 10, 8, false);
        { F g = f; set_table_mode(g, 6); visit(g, 16384, 10, 8, false); }
        { F g = f; g.part_n = 2; visit(g, 16384, 10, 8, false); }
    }
    for (int64_t ml : {((int64_t)1 << 27) - 1, (int64_t)1 << 27, ((int64_t)1 << 28) - 1, (int64_t)1 << 28})
        for (int m : {8, 16}) {
            F f = facts_of<F>(Shape{false, 128, 8192, m, 128 / m, 256, (int64_t)70000 * 8192, ml});
            set_table_mode(f, 7);
            visit(f, 16384, 10, 8, false);
        }
    // every tuning value and table mode on the shapes they matter for
    for (int qg : TUNE_QG)
        for (int ch : TUNE_CHUNK) {
            if (qg < 0 && ch != 0) continue;   // (a chunk size means nothing to the query-major and the generic requests)
            { F f = sift1b; f.force_qg = qg; f.force_chunk = ch; visit(f, 16384, 10, 8, false); }
            if (ch == 0) { F f = sift1m; f.force_qg = qg; visit(f, 1024, 10, 8, false); }
        }
    for (int mode = 0; mode <= 10; ++mode)
        for (const F &b : {sift1m, sift1b, hd}) {
            if (b.m == 48 && mode > 4) continue;   // (modes 5 ... 10 are about kernels that m = 48 does not have)
            F f = b; set_table_mode(f, mode);
            visit(f, 16384, 10, 8, false);
        }
    for (const Shape &s : OTHERS) {
        Shape t = s; t.n = 9000 * (int64_t)s.kc; t.maxlen = 10000;
        F f = facts_of<F>(t);
        visit(f, 16384, 10, 8, false);
        if (s.m == 8 || s.m == 16 || s.m == 5) { F g = f; set_table_mode(g, 7); visit(g, 16384, 10, 8, false); }
        // the eight-wave kernel's four-query form on request (m = 16: its own LDS layout), and its wide pool (m = 8 only)
        if (!s.u16 && (s.m == 8 || s.m == 16))
            for (int mode : {6, 8}) { F g = f; set_table_mode(g, mode); visit(g, 16384, mode == 6 ? 10 : 100, 8, false); }
        if (s.u16 || s.m == 48) { F g = f; g.ws_budget = (size_t)1 << 20; visit(g, 65536, 100, 32, false); }
        if (!s.u16) continue;
        for (int64_t len : {1024, 1025})   // UInt16 table-free where it is expected to win: min(avg_len, 1024) <= ksub
            for (int ut : {0, 2}) {
                Shape u = s; u.n = len * s.kc; u.maxlen = len + 50;
                F g = facts_of<F>(u); g.u16_tables = ut;
                visit(g, 4096, 10, 8, false);
                if (len == 1024) visit(g, 4096, 1984, 8, false);
            }
        { F g = f; g.u16_tables = 1; visit(g, 4096, 10, 8, false); visit(g, 4096, 2048, 8, false); }
    }
    // what bounds a sub-batch (plan_subbatch): the batch itself, the workspace budget, the kernels' 32-bit arguments (2^22 queries: a
    // cheap query-major search of a huge batch), and 2^30 partial-result slots (w x maxch large, under a raised workspace limit)
    const int64_t huge = ((int64_t)1 << 22) + 1;
    for (const F &b : {toy, sift1m, hd}) {
        visit(b, huge, 10, 1, false);
        visit(b, huge, 10, 8, false);
        { F f = b; f.ws_budget = (size_t)1 << 20; visit(f, huge, 10, 8, false); visit(f, 64, 10, 8, false); visit(f, 65, 10, 8, false); }
    }
    for (int64_t nq : {(int64_t)65536, huge})
        for (int w : {8, 128}) {
            F f = sift1b; f.ws_budget = (size_t)64 << 30; f.force_chunk = 2048;   // (64 chunks per list)
            visit(f, nq, 1, w, false);
            visit(f, nq, 100, w, false);
            f.ws_budget = (size_t)8 << 30;
            visit(f, nq, 1, w, false);
        }
}

// Every case.  Part A: every shape and list length x every nq, K, w at the default switches.  Part B: the BASELINE shapes and the long-list
// forms of the specialised shapes x one switch group at a time x every nq and the K, w that switch a branch.  Part C: 200 000 draws
// over everything at once (seed 2024), switches in combination and impossible combinations included.  Part D: plan_pairs.
template <class F, class V> long plan_grid(V visit)
{
    long cases = 0;
    auto emit = [&](const F &f, int64_t nq, int K, int w, bool pre) { visit(f, nq, K, w, pre); ++cases; };
    each_context<F>([&](const F &f) {
        each_nq(f.num_cu, [&](int64_t nq) {
            for (int K : KS)
                for (int w : WS) emit(f, nq, K, w, false);
        });
    });
    int ctx = 0;
    each_context<F>([&](const F &c) {
        const int i = ctx++;
        const bool baseline = i < 5;
        const bool long_list = !baseline && c.n / c.kc == 70000 && c.maxlen < ((int64_t)1 << 27) - 1;
        if (!baseline && !long_list) return;
        each_config<F>(c, [&](const F &f) {
            each_nq(f.num_cu, [&](int64_t nq) {
                for (int K : {1, 64, 65, 128, 129, 2048})
                    for (int w : {1, 2, 3, 8, 32, 33, 48, 49, 64, 65}) emit(f, nq, K, w, (nq + K + w) % 5 == 0);
            });
        });
    });
    Rng r{2024};
    F pool[512];
    size_t np = 0;
    each_context<F>([&](const F &c) { if (np < 512) pool[np++] = c; });
    for (int i = 0; i < 200000; ++i) {
        F f = pool[r.below(np)];
        set_table_mode(f, (int)r.below(11));
        set_coarse_mode(f, (int)r.below(3));
        if (r.below(3) == 0) { f.force_qg = r.pick(TUNE_QG); f.force_chunk = r.pick(TUNE_CHUNK); }
        f.u16_tables = (int)r.below(3);
        f.part_n = r.below(4) == 0 ? 2 : 1;
        f.prune_est = r.below(3) == 0 ? -1.0f : (r.below(2) ? 0.59f : 0.6f);
        f.allow_prune = r.below(8) != 0;
        f.allow_lb = r.below(8) != 0;
        f.allow_nf = r.below(8) != 0;
        f.lanes_active = r.below(3) == 0;
        f.tl_use = r.below(3) == 0;
        f.tl_G = r.below(2) ? (r.below(2) ? 64 : 4096) : 0;
        f.ws_budget = r.below(4) == 0 ? (size_t)1 << 20 : (size_t)8 << 30;
        if (r.below(8) == 0) f.have_lb_operands = !f.have_lb_operands;
        if (r.below(8) == 0) f.have_nf_operands = !f.have_nf_operands;
        int64_t nqs[10];
        size_t nn = 0;
        each_nq(f.num_cu, [&](int64_t nq) { nqs[nn++] = nq; });
        const int64_t nq = nqs[r.below(nn)];   // (one draw per statement: the order of evaluation of arguments is the compiler's)
        const int K = r.pick(KS);
        const int w = r.pick(WS);
        const bool pre = r.below(4) == 0;
        emit(f, nq, K, w, pre);
    }
    plan_pairs<F>(emit);
    return cases;
}

}  // namespace plan_grid_ns
