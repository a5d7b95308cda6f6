// Stand-alone check of csrc/selscan_plan.h (tests/test_selscan_plan.py builds it with -fsanitize=address,undefined and runs it directly).
// Over a grid of (d, m, K, forced capacity): the LDS regions of the layout are disjoint, aligned and end within a compute unit's
// 160 KB; a served plan's buffer holds 2 pow2ceil(K) keys and two steps of the workgroup; served is false exactly where no such buffer
// fits; the byte count the host passes to the launch is the layout's end; the sub-batch stays inside the workspace.
#include "../../ivfadc.jl_amd/csrc/selscan_plan.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

using namespace selscan;

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            if (++g_fail > 20) exit(1);                                       \
        }                                                                     \
    } while (0)

constexpr size_t LDS_MAX = 160 << 10;
constexpr int MAX_K = 2048, MAX_W = 2048;

int main()
{
    const int ds[] = {1, 6, 10, 96, 128, 768, 2048}, ms[] = {1, 2, 8, 16, 48, 64, 96, 104, 128, 160};
    const int ks[] = {1, 2, 64, 65, 100, 128, 1000, 1024, 1025, 2047, 2048, 2049}, caps[] = {0, 1, 1024, 1025, 4096, 8192, 20000, 1 << 30};
    long cases = 0, served = 0;
    for (int d : ds)
        for (int m : ms)
            for (int K : ks)
                for (int fc : caps)
                    for (bool u16 : {false, true}) {
                        Facts f;
                        f.d = d; f.kc = 1024; f.m = m; f.u16 = u16; f.max_k = MAX_K; f.max_w = MAX_W; f.force_cap = fc;
                        f.ws_budget = (size_t)1 << 20; f.lds_max = LDS_MAX;
                        const Plan p = make_plan(f, 5000, K, 8);
                        ++cases;
                        // what the issue's rule says, restated: a buffer of `need` keys next to everything else
                        const int64_t p2 = pow2ceil(K);
                        const int64_t need = 2 * p2 > 2 * STEP_MAX ? 2 * p2 : 2 * STEP_MAX;
                        const size_t fixed = (size_t)((d + 3) / 4 * 4) * 4 + (size_t)m * 1024 + (size_t)((p2 * 8 + 15) / 16 * 16) + HIST_BYTES + CTL_BYTES;
                        const bool fits = fixed + (size_t)need * 8 <= LDS_MAX;
                        CHECK(p.served == (!u16 && K <= MAX_K && fits));
                        if (!p.served) continue;
                        ++served;
                        const Layout &l = p.lay;
                        CHECK(p.cap % CAP_ALIGN == 0 && p.cap >= 2 * p2 && p.cap >= K + STEP_MAX);
                        CHECK(l.resid == 0 && l.tab >= (size_t)d * 4 && l.tab % 16 == 0);
                        CHECK(l.keys >= l.tab + (size_t)m * 1024 && l.keys % 16 == 0);
                        CHECK(l.scratch >= l.keys + (size_t)p.cap * 8 && l.scratch % 8 == 0);
                        CHECK(l.hist >= l.scratch + (size_t)p2 * 8 && l.hist % 16 == 0);
                        CHECK(l.ctl >= l.hist + HIST_BYTES && l.ctl % 8 == 0 && l.end >= l.ctl + CTL_BYTES);
                        CHECK(l.end <= LDS_MAX && p.lds == l.end && p.lds == layout(d, m, K, p.cap).end);
                        // automatic: the largest buffer; forced: rounded up to 1024 keys, clamped between what is needed and what fits
                        const int64_t most = cap_max(d, m, K, LDS_MAX);
                        CHECK(layout(d, m, K, most + CAP_ALIGN).end > LDS_MAX);
                        int64_t want = fc > 0 ? ((int64_t)fc + 1023) / 1024 * 1024 : most;
                        want = want > most ? most : (want < need ? need : want);
                        CHECK(p.cap == want);
                        CHECK(p.nb >= 1 && p.nb <= 5000 && (size_t)p.nb * (1024 * 4 + 8 * 12 + 64) <= f.ws_budget);
                    }
    CHECK(served > 0 && served < cases);
    Facts f;
    f.d = 128; f.kc = 1024; f.m = 8; f.max_k = MAX_K; f.max_w = MAX_W; f.ws_budget = (size_t)8 << 30; f.lds_max = LDS_MAX;
    CHECK(!make_plan(f, 10, 0, 8).served && !make_plan(f, 10, 10, MAX_W + 1).served && make_plan(f, 10, 10, MAX_W).served);
    CHECK(make_plan(f, 10, 1000, 8).cap == 16384 && make_plan(f, 10, 1000, 8).nb == 10);
    if (g_fail) return 1;
    printf("selscan_plan_check ok: %ld cases, %ld served\n", cases, served);
    return 0;
}
