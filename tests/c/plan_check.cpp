// The search planner (csrc/plan.h) on the CPU: a stand-alone program, built with the sanitizers by tests/test_plan.py.
//
//   plan_check TABLE         every row of tests/plan_table.tsv replayed (the first differing row ends the run), then the invariants below
//                            over the whole grid of plan_grid.h; closes with "plan_check ok: <grid cases> grid cases, <rows> table rows"
//   plan_check --print-grid  one line per grid case (what a revision that moves planner code compares with its parent's)
//   plan_check --print-table the table: header, the curated pairs of plan_grid.h, and the first grid case of every outcome
//
// The table pins what the planner decides today; the invariants say what must hold of ANY rule, which a table cannot.
#include "../../ivfadc.jl_amd/csrc/plan.h"
#include "plan_grid.h"

#include <set>
#include <string>

using namespace ivf;
using namespace plan_grid_ns;

static Plan plan_of(const PlanFacts &f, int64_t nq, int K, int w, bool pre)   // as search_dev chooses
{
    return f.u16 ? make_plan_u16(f, nq, K, w, pre) : make_plan(f, nq, K, w, pre);
}

static long g_bad = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond) && g_bad++ < 20) {                                               \
            char line[1024];                                                         \
            plan_line(line, sizeof line, f, nq, K, w, pre, p);                       \
            printf("INVARIANT %s\n  %s\n", #cond, line);                             \
        }                                                                            \
    } while (0)

static void invariants(const PlanFacts &f, int64_t nq, int K, int w, bool pre, const Plan &p)
{
    const bool u16_form = p.form == ScanForm::U16 || p.form == ScanForm::U16Wide || p.form == ScanForm::U16Direct || p.form == ScanForm::U16DirectWide;
    CHECK(!p.fits || p.lds <= LDS_MAX);
    CHECK(!p.fits || (p.nb >= 1 && p.nb <= nq));
    CHECK(!p.fits || (p.qg >= 1 && p.qg <= 8));
    if (p.fits && !p.query_major()) {
        const int64_t chunks = (f.maxlen + p.CH - 1) / p.CH;
        CHECK(p.CH > 0 && chunks <= 64);
        CHECK(p.maxch == (chunks > 1 ? chunks : 1));
        if (f.force_chunk > 0) CHECK(p.CH % (u16_form ? (uint32_t)U16_PASS : 1024u) == 0);
    }
    if (p.fits && (p.form == ScanForm::EightWave || p.form == ScanForm::NarrowField)) CHECK(p.lds <= (size_t)(80 << 10));
    // a form only where its kernels are instantiated
    CHECK(u16_form == f.u16);
    CHECK(p.form != ScanForm::QueryMajorLb || (lb_shape(f.m, f.dsub) && f.have_lb_operands && p.small_k && w <= 32));
    CHECK(p.form != ScanForm::NarrowField || (nf_shape(f.m, f.dsub) && f.have_nf_operands && p.small_k && p.qg == 8));
    CHECK(p.form != ScanForm::EightWave || (f.m == 8 && w8_dsub(f.dsub)) || (f.m == 16 && w8_m16_dsub(f.dsub) && !p.wide));
    CHECK(p.form != ScanForm::EightWave || (p.threads == W8_THREADS && p.qg == (p.q8 ? 8 : 4) && K <= (p.wide ? W8_WIDE_MAX_K : 64)));
    CHECK(p.form != ScanForm::EightWave || f.maxlen < ((int64_t)1 << (f.m == 16 ? 27 : 28)));
    CHECK(!p.stripe || (p.form == ScanForm::FourWave && filt_shape(f.m, f.dsub) && p.qg == 4));
    CHECK((!p.q8 && !p.wide) || p.form == ScanForm::EightWave);
    // the coarse stage
    CHECK(!(p.coarse_mfma && p.twolevel));
    CHECK(!pre || (!p.coarse_mfma && !p.twolevel && !p.fuse_topw));
    CHECK(!p.lanes || !p.fuse_topw);
    CHECK(!p.fuse_topw || p.query_major());
}

static int replay_table(const char *path, long &rows)
{
    FILE *fp = fopen(path, "r");
    if (!fp) { printf("cannot open %s\n", path); return 1; }
    char row[2048], line[1024];
    rows = 0;
    for (long no = 1; fgets(row, sizeof row, fp); ++no) {
        row[strcspn(row, "\r\n")] = 0;
        if (no == 1) {
            if (strcmp(row, PLAN_COLUMNS) != 0) { printf("%s: the header names other columns than plan_grid.h prints\n", path); fclose(fp); return 1; }
            continue;
        }
        PlanFacts f;
        int64_t nq;
        int K, w;
        bool pre;
        if (!plan_parse(row, f, nq, K, w, pre)) { printf("%s:%ld: not a case\n", path, no); fclose(fp); return 1; }
        plan_line(line, sizeof line, f, nq, K, w, pre, plan_of(f, nq, K, w, pre));
        if (strcmp(row, line) != 0) {
            printf("%s:%ld: the plan differs from the pinned one (fields: %s)\n  pinned  %s\n  planned %s\n", path, no, PLAN_COLUMNS, row, line);
            fclose(fp);
            return 1;
        }
        ++rows;
    }
    fclose(fp);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    char line[1024];
    if (mode == "--print-grid") {
        plan_grid<PlanFacts>([&](const PlanFacts &f, int64_t nq, int K, int w, bool pre) {
            plan_line(line, sizeof line, f, nq, K, w, pre, plan_of(f, nq, K, w, pre));
            puts(line);
        });
        return 0;
    }
    if (mode == "--print-table") {
        std::set<std::string> printed, outcomes;
        puts(PLAN_COLUMNS);
        auto row = [&](const PlanFacts &f, int64_t nq, int K, int w, bool pre, bool always) {
            const Plan p = plan_of(f, nq, K, w, pre);
            char sig[128], sig2[128];
            // an outcome of the scan and coarse choice: the form, its flags and width ...
            snprintf(sig, sizeof sig, "A %d %d%d%d %d %d %d%d%d%d %d", (int)p.form, (int)p.stripe, (int)p.q8, (int)p.wide, p.qg, (int)p.fits, (int)p.coarse_mfma,
                     (int)p.fuse_topw, (int)p.lanes, (int)p.twolevel, (int)p.small_k);
            // ... and of the sizes, per form: the LDS layout where a form has several (the eight-wave kernel's: m = 8 / 16, four / eight
            // queries, wide pool), what bounded the sub-batch (0 the batch, 1 the workspace budget, 2 the 32-bit arguments, 3 the 2^30
            // partial-result slots), one chunk per list or several
            const int64_t slots = std::max<int64_t>(64, ((int64_t)1 << 30) / std::max(1, w * p.maxch));
            const int bound = !p.fits || p.nb == nq ? 0 : (p.nb == (int64_t)1 << 22 ? 2 : (p.nb == slots ? 3 : 1));
            snprintf(sig2, sizeof sig2, "B %d %llu %d %d", (int)p.form, p.form == ScanForm::EightWave ? (unsigned long long)p.lds : 0ull, bound,
                     (int)(p.fits && p.maxch > 1));
            const bool fresh_a = outcomes.insert(sig).second, fresh_b = outcomes.insert(sig2).second;
            if (!always && !fresh_a && !fresh_b) return;
            plan_line(line, sizeof line, f, nq, K, w, pre, p);
            if (printed.insert(line).second) puts(line);
        };
        plan_pairs<PlanFacts>([&](const PlanFacts &f, int64_t nq, int K, int w, bool pre) { row(f, nq, K, w, pre, true); });
        plan_grid<PlanFacts>([&](const PlanFacts &f, int64_t nq, int K, int w, bool pre) { row(f, nq, K, w, pre, false); });
        return 0;
    }
    if (argc != 2) { printf("usage: plan_check TABLE | --print-grid | --print-table\n"); return 2; }
    long rows = 0;
    if (replay_table(argv[1], rows) != 0) return 1;
    const long cases = plan_grid<PlanFacts>([&](const PlanFacts &f, int64_t nq, int K, int w, bool pre) { invariants(f, nq, K, w, pre, plan_of(f, nq, K, w, pre)); });
    if (g_bad) { printf("%ld invariant violations\n", g_bad); return 1; }
    printf("plan_check ok: %ld grid cases, %ld table rows\n", cases, rows);
    return 0;
}
