// Stand-alone check of the four-wave kernels' LDS layout in csrc/scan_layouts.h (tests/test_scan_lds.py builds it with
// -fsanitize=address,undefined and runs it directly).  FwLds / FwTail / SqLds are what carve_lds and sq_kernel fill their pointers from
// and what the plan's scan_lds_bytes, sq_lds_bytes and lb_lds_bytes take their ends from; this program sweeps
//   m in {1, 2, 3, 8, 16, 48, 64} x dsub in {1, 2, 4, 6, 8, 16} (m dsub <= 1024), qg in {1, 2, 4}, K in {1, 64, 65, 100, 128, 1984} through
//   sel_cap, small / list_major / stripe on and off; for sq_kernel kc in {4, 2045, 2048}, inside on and off; the eight LB instantiations
// and checks that (a) the regions stand in order and are pairwise disjoint, the exchange area over the tables included, (b) u64 regions
// start at 8 bytes, the filter table, the residuals and sq_kernel's row at 16, parked entries at 4, (c) the short-row scratch lies inside the
// probe area behind five 32-entry arrays and three 64-entry arrays end at the area's last byte, (d) the four waves' parking buffers end at
// the layout's end (m = 16; the area is sized for five-dword entries, so at m = 8 the last wave's ends 512 B short of it), (e) every end is
// the figure the plan reported before the layout existed: the formulas of that time are kept below, verbatim, as the frozen figures.
// The region check is then fed two wrong layouts -- parking buffers 128 dwords (not 192) behind the probes, a tail without the 8-byte
// round-up -- and has to report both.
#include "../../ivfadc.jl_amd/csrc/scan_layouts.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

using namespace ivf;

static int g_fail = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            if (++g_fail > 20) exit(1);                                       \
        }                                                                     \
    } while (0)

// ---- the frozen figures: scan_lds_bytes, lb_lds_bytes and the small-batch sum as they stood, literals and all ------------------------
static size_t old_scan_lds_bytes(int m, int d, int qg, int cap, bool small, bool list_major = false, bool stripe = false)
{
    size_t b = (size_t)(m > 2 ? m : 2) * 256 * qg * 4;
    b += align_up((size_t)d * qg, 4) * 4;
    if (!small) b += (size_t)4 * (list_major ? qg : 1) * cap * 8;
    b += (size_t)4 * qg * 4 + 16;
    b = align_up(b, 8) + (size_t)qg * 40;
    b += 3 * 256;
    if (list_major && qg == 4 && (m == 8 || m == 16))
        b += 4 * 16 * 5 * 4;
    if (stripe && m == 8)
        b += 256 * 64;
    return b;
}

static size_t old_lb_lds_bytes(int m, int dsub, int pg)
{
    size_t b = align_up((size_t)pg * ((size_t)m * 256 + 32), 16);
    b += (size_t)m * pg * ((dsub + 3) & ~3) * 4;
    b += 2 * (size_t)m * pg * 4 + 128 + 256;
    b += (size_t)m * dsub * 4;
    b += (size_t)4 * (pg >= 4 ? 54 : 16) * (m / 4 + 2) * 4;
    b += 4 * 64 * 8;
    b += (size_t)4 * pg * 4 + 16 + (size_t)pg * 40 + 3 * 256;
    return b;
}

static size_t old_sq_lds_bytes(int m, int d, int kc, bool inside)
{
    return old_scan_lds_bytes(m, d, 1, 64, true) + 64 + (inside ? (size_t)kc * 4 : 0);
}

// ---- regions ----------------------------------------------------------------------------------------------------------------------
struct Region {
    const char *name;
    size_t begin, bytes, align;
};

// violations among regions given in layout order: a start off its alignment, a region reaching into the next, the last one past `end`
static int region_faults(const Region *r, int n, size_t end, bool say)
{
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        const size_t stop = r[i].begin + r[i].bytes, next = i + 1 < n ? r[i + 1].begin : end;
        if (r[i].begin % r[i].align != 0) {
            ++bad;
            if (say) fprintf(stderr, "  %s at %zu is not %zu-byte aligned\n", r[i].name, r[i].begin, r[i].align);
        }
        if (stop > next) {
            ++bad;
            if (say) fprintf(stderr, "  %s [%zu, %zu) reaches past %zu\n", r[i].name, r[i].begin, stop, next);
        }
    }
    return bad;
}

// the tail's regions, as the kernels use them: park_m = 0 (no parking buffers), 8 or 16
static int tail_faults(const FwTail &t, int qg, int park_m, bool say)
{
    const size_t park_bytes = park_m ? (size_t)4 * CAND_CAP * cand_stride(park_m) * 4 : 0;
    const Region r[] = {
        {"scnt", t.scnt, (size_t)4 * qg * 4, 4},
        {"swi", t.swi, 16, 4},
        {"sthr", t.sthr, (size_t)qg * STHR_WORDS * 8, 8},
        {"probes", t.probes, FW_PROBE_BYTES, 4},
        {"park", t.park, park_bytes, 4},
    };
    int bad = region_faults(r, 5, t.end, say);
    // (c) the scratch words: behind five 32-entry arrays, inside the probe area, in order
    const Region s[] = {
        {"probe arrays (32 entries)", t.probes, 5 * 32 * 4, 4},
        {"wbound", t.wbound, 4 * 8, 8},
        {"ccnt", t.ccnt, 2 * 4, 4},
        {"flag", t.flag, 4, 4},
    };
    bad += region_faults(s, 4, t.probes + FW_PROBE_BYTES, say);
    return bad;
}

static int layout_faults(const FwLds &l, int m, int d, int qg, int nsel, int cap, bool small, size_t extra, int park_m, bool say)
{
    const Region r[] = {
        {"tab", l.tab, (size_t)m * 256 * qg * 4, 16},
        {"qf", l.qf, extra, 16},
        {"resid", l.resid, (size_t)d * qg * 4, 16},
        {"selbuf", l.selbuf, small ? 0 : (size_t)4 * nsel * cap * 8, 8},
    };
    int bad = region_faults(r, 4, l.t.scnt, say) + tail_faults(l.t, qg, park_m, say);
    // the exchange area of the register selectors lies over the tables: 4 waves x qg slots x 64 keys
    if (small && l.tab + (size_t)4 * qg * 64 * 8 > l.qf) {
        ++bad;
        if (say) fprintf(stderr, "  the exchange area reaches past the tables\n");
    }
    return bad;
}

// the second planted error: fw_tail without the round-up in front of the u64 words
static FwTail tail_without_roundup(size_t base, int qg, bool park)
{
    FwTail t = fw_tail(base, qg, park);
    const size_t back = t.sthr - (t.swi + 16);
    t.sthr -= back; t.probes -= back; t.wbound -= back; t.ccnt -= back; t.flag -= back; t.park -= back; t.end -= back;
    return t;
}

template <int M, int DS, int PG> static int check_lb()
{
    const size_t cfg_end = LbCfg<M, DS, PG>::END;
    const FwTail t = fw_tail(cfg_end, PG);
    CHECK(tail_faults(t, PG, 0, true) == 0 && t.scnt == cfg_end);
    CHECK(t.end == lb_lds_bytes(M, DS, PG) && t.end == old_lb_lds_bytes(M, DS, PG));
    return 1;
}

int main()
{
    const int ms[] = {1, 2, 3, 8, 16, 48, 64}, dsubs[] = {1, 2, 4, 6, 8, 16}, qgs[] = {1, 2, 4}, Ks[] = {1, 64, 65, 100, 128, 1984};
    const int kcs[] = {4, 2045, 2048};
    long layouts = 0, sqs = 0, lbs = 0, planted = 0;

    for (int m : ms) for (int dsub : dsubs) {
        if (m * dsub > 1024) continue;
        const int d = m * dsub;
        for (int qg : qgs) for (int K : Ks) for (int sm = 0; sm < 2; ++sm) for (int lm = 0; lm < 2; ++lm) for (int st = 0; st < 2; ++st) {
            const int cap = sel_cap(K), nsel = lm ? qg : 1;
            const bool small = sm != 0, list_major = lm != 0, stripe = st != 0;
            const size_t extra = stripe && m == 8 ? QF_BYTES : 0;
            const int park_m = list_major && qg == 4 && (m == 8 || m == 16) ? m : 0;
            const FwLds l = fw_lds(m, d, qg, nsel, cap, small, extra, park_m != 0);
            ++layouts;
            const int bad = layout_faults(l, m, d, qg, nsel, cap, small, extra, park_m, true);   // (a), (b), (c)
            if (bad) fprintf(stderr, "m %d dsub %d qg %d K %d small %d list_major %d stripe %d: %d faults\n", m, dsub, qg, K, sm, lm, st, bad);
            CHECK(bad == 0);
            {   // the kernels carve the tail by fw_tail(0, QG)'s offsets from its start: it must not matter where the tail stands
                const FwTail t = l.t, r = fw_tail(0, qg, park_m != 0);
                CHECK(t.scnt % 16 == 0 && t.swi == t.scnt + r.swi && t.sthr == t.scnt + r.sthr && t.probes == t.scnt + r.probes);
                CHECK(t.wbound == t.scnt + r.wbound && t.ccnt == t.scnt + r.ccnt && t.flag == t.scnt + r.flag && t.park == t.scnt + r.park);
                CHECK(t.end == t.scnt + r.end);
                // ... and the regions in front follow each other at the lengths the carve adds up
                CHECK(l.qf == fw_tab_floats(m, qg) * 4 && l.selbuf == l.resid + fw_resid_floats(d, qg) * 4);
                CHECK(t.scnt == l.selbuf + (small ? 0 : fw_selbuf_keys(nsel, cap) * 8));
            }
            CHECK(l.t.probes + (size_t)3 * fw_probe_entries(33) * 4 == l.t.probes + FW_PROBE_BYTES && l.t.park == l.t.probes + FW_PROBE_BYTES);
            CHECK(fw_probe_entries(1) == 32 && fw_probe_entries(32) == 32 && fw_probe_entries(33) == 64 && fw_probe_entries(64) == 64);
            if (park_m) {   // (d)
                const size_t last = l.t.park + (size_t)4 * CAND_CAP * cand_stride(park_m) * 4;
                CHECK(last + (park_m == 8 ? 512 : 0) == l.t.end);
            } else {
                CHECK(l.t.park == l.t.end);
            }
            CHECK(l.t.end == scan_lds_bytes(m, d, qg, cap, small, list_major, stripe));          // (e)
            CHECK(l.t.end == old_scan_lds_bytes(m, d, qg, cap, small, list_major, stripe));
        }
        for (int kc : kcs) for (int in = 0; in < 2; ++in) {
            const SqLds s = sq_lds(m, d, in ? kc : 0);
            const FwLds l = fw_lds(m, d, 1, 1, 64, true);
            ++sqs;
            const Region r[] = {
                {"sthr", l.t.sthr, (size_t)STHR_WORDS * 8, 8},
                {"s_list", s.s_list, 64 * 4, 4},
                {"s_dc", s.s_dc, 64 * 4, 4},
                {"s_base", s.s_base, 64 * 4, 4},
                {"wbound", s.wbound, 4 * 8, 8},
                {"ccnt", s.ccnt, 4 * 4, 4},
                {"s_row", s.s_row, in ? (size_t)kc * 4 : 0, 16},
            };
            CHECK(region_faults(r, 7, s.end, true) == 0);
            {   // sq_kernel's constant offsets from the tail's start, and the row where the rounded-up pointer lands
                const SqLds rel = sq_tail(0, in ? kc : 0);
                const size_t base = l.t.scnt;
                CHECK(base % 16 == 0 && s.s_list == base + rel.s_list && s.s_dc == base + rel.s_dc && s.s_base == base + rel.s_base);
                CHECK(s.wbound == base + rel.wbound && s.ccnt == base + rel.ccnt && s.row_lo == base + rel.row_lo && s.end == base + rel.end);
                CHECK(s.s_row == (s.row_lo + 15) / 16 * 16 && s.row_lo == s.ccnt + 16);
            }
            CHECK(layout_faults(l, m, d, 1, 1, 64, true, 0, 0, true) == 0);
            CHECK(s.end == sq_lds_bytes(m, d, in ? kc : 0) && s.end == old_sq_lds_bytes(m, d, kc, in != 0));
        }
    }

    // the matrix-core rounds: LbCfg's regions, then the same tail
#define X(M_, D_, P_) lbs += check_lb<M_, D_, P_>();
    IVF_LB_SHAPES(X)
#undef X
    CHECK(lb_lds_bytes(8, 16, 2) > LDS_MAX);   // no such kernel: nothing fits

    // ---- teeth: two wrong layouts, each of which the region check must report --------------------------------------------------
    for (int m : {8, 16}) {
        FwLds l = fw_lds(m, m * 8, 4, 4, 64, true, 0, true);
        CHECK(layout_faults(l, m, m * 8, 4, 4, 64, true, 0, m, false) == 0);
        l.t.park = l.t.probes + 128 * 4;   // 128 dwords behind the probes' start: inside the 64-entry arrays
        ++planted;
        CHECK(layout_faults(l, m, m * 8, 4, 4, 64, true, 0, m, false) > 0);
    }
    for (int qg : qgs) {
        // a base 4 bytes off the 8-byte grid: fw_tail rounds the u64 words up, the wrong one does not
        const size_t base = 1024 + 4;
        CHECK(tail_faults(fw_tail(base, qg, true), qg, 16, false) == 0);
        ++planted;
        CHECK(tail_faults(tail_without_roundup(base, qg, true), qg, 16, false) > 0);
    }

    if (g_fail) {
        fprintf(stderr, "scan_lds_check: %d checks failed\n", g_fail);
        return 1;
    }
    printf("scan_lds_check ok: %ld layouts, %ld sq layouts, %ld lb layouts, %ld planted errors reported\n", layouts, sqs, lbs, planted);
    return 0;
}
