// plan.h -- the search planner: which scan kernel a search runs, how many queries share a code stream, the chunk size, the dynamic LDS
// it asks for, the sub-batch size and the coarse stage.  A PURE function of PlanFacts and (nq, K, w, pre): plain C++ on scan_layouts.h
// and the standard library, no handle, no HIP call, no environment, no error path -- so every rule below runs without a GPU
// (tests/c/plan_check.cpp: invariants over a grid, and tests/plan_table.tsv, the decisions pinned row by row).  ivfadc_hip.hip reads the
// handle into a PlanFacts in ONE place (plan_facts) and resolves the planned form to a kernel in one (plan_kernel).
#pragma once

#include "scan_layouts.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace ivf {

// everything the planner reads, by value
struct PlanFacts {
    // shape and lists (Dims, Lists)
    int d = 0, kc = 0, m = 0, dsub = 0, ksub = 0;
    int64_t n = 0, maxlen = 0;
    int num_cu = 256;
    bool u16 = false;
    // switches (SearchConfig: the setters of include/ivfadc_hip.h)
    bool allow_filt = true, allow_lb = true, force_lb = false, allow_nf = true, allow_prune = true, allow_mfma = true;
    int mfma_min_kc = 2048;
    int wg8_mode = 0;
    bool wg8_wide = false;
    int u16_tables = 0;
    int part_n = 1;
    int force_qg = 0, force_chunk = 0;
    size_t ws_budget = (size_t)8 << 30;
    // the two-level coarse search as the handle's first search left it
    bool tl_use = false;
    int tl_G = 0;
    float prune_est = -1.0f;         // smoothed pruned fraction of the probed points (< 0: not known yet; fb_poll in ivfadc_hip.hip)
    bool have_lb_operands = false;   // the matrix-core table operands are on the device (lb_split)
    bool have_nf_operands = false;   // ... the narrow-field kernel's (nf_n2)
    bool lanes_active = false;       // a device-pointer entry while several lanes of this replica search side by side
};

// The scan a search runs.  Query-major: one workgroup per query (qscan_kernel), Lb with 8-bit lower-bound tables from the matrix cores
// (lbscan.hip.h).  List-major: FourWave scan_kernel (striped tables: Plan::stripe); NarrowField nf_scan_kernel, eight queries per code
// stream behind the 4-bit filter (nfscan.hip.h); EightWave wg8scan.hip.h, eight waves per workgroup on four conflict-free copies of
// the integer filter table (Plan::q8: eight queries per stream; Plan::wide: the wide pool of 64 < K <= 128, the merge behind it is
// the one of K > 64); U16 / U16Wide u16scan.hip.h on register / LDS selectors, U16Direct / U16DirectWide its table-free entries.
// Masked: masked_scan_kernel (maskset.hip.h), the list scan of ivfadc_search_masked -- planned by make_plan_masked alone, never by make_plan.
enum class ScanForm { QueryMajor, QueryMajorLb, FourWave, NarrowField, EightWave, U16, U16Wide, U16Direct, U16DirectWide, Masked };

struct Plan {
    ScanForm form = ScanForm::QueryMajor;
    bool stripe = false, q8 = false, wide = false;   // FourWave / EightWave only (see ScanForm)
    const void *fn = nullptr;   // the scan kernel of the form: scan_fn_t, qscan_fn_t, wg8_fn_t, nf_fn_t or u16_fn_t (plan_kernel in ivfadc_hip.hip)
    int threads = 256;          // ... and its workgroup size
    bool coarse_mfma = false;   // coarse scores on the matrix cores + certified exact refine (w <= 48)
    bool fuse_topw = false;   // query-major only: top-w selection runs inside the scan kernel
    bool lanes = false;         // several batches in flight on this replica: stand-alone top-w, a wave per query (see make_plan)
    bool twolevel = false;      // coarse stage: certified two-level search (twolevel.hip.h) instead of the exhaustive kernels + top-w
    bool small_k = true, small_w = true;
    int qg = 0, cap = 64, capw = 64, maxch = 1;
    uint32_t CH = 0;
    size_t lds = 0;
    int64_t nb = 0;   // queries per sub-batch
    bool fits = true;    // false: the selection kernels' LDS need exceeds the CU's 160 KB -> the caller takes the generic path
    bool query_major() const { return form == ScanForm::QueryMajor || form == ScanForm::QueryMajorLb; }
    // ivfadc_stats.last_striped of a list-major form: 1 striped four-wave tables; 2 / 3 eight-wave, four / eight queries; 4 / 5 its wide pool;
    // 6 / 7 the table-free UInt16 scan on register / LDS selectors; 8 the masked scan
    int striped() const
    {
        if (form == ScanForm::Masked) return 8;
        if (form == ScanForm::U16Direct) return 6;
        if (form == ScanForm::U16DirectWide) return 7;
        return form == ScanForm::EightWave ? (wide ? 4 : 2) + (q8 ? 1 : 0) : (stripe ? 1 : 0);
    }
};

// the shapes (m, dsub) the handle's table mode admits to the eight-wave kernel, and the longest list the kernel's 28-bit positions and
// 31-bit byte offsets hold
inline bool w8_md(const PlanFacts &f) { return (f.m == 8 && w8_dsub(f.dsub)) || (f.m == 16 && w8_m16_dsub(f.dsub) && f.wg8_mode > 0); }
inline int64_t w8_maxlen(const PlanFacts &f) { return (int64_t)1 << (f.m == 16 ? 27 : 28); }
// ... and where the plan takes the kernel unasked (wg8_mode == 0; table modes 6 / 7 take it wherever it is instantiated): see make_plan
inline bool w8_default(const PlanFacts &f) { return f.m == 8 && f.dsub == 16 && f.part_n <= 1; }

// Coarse stage: the certified two-level search (twolevel.hip.h: its four waves keep their queries in LDS), or the matrix-core filter
// -- which pays when the coarse search is large: below ~2k centroids the extra selection + refine work in the scan prologue costs
// more than the VALU kernel it replaces (SIFT1M-shape: 92 -> 121 us per batch) -- or, with neither, the exact VALU kernels.
// own: the search has a coarse stage of these kernels at all (not the caller's probes, not the generic path's sort); tl_batch: the
// batch is one the two-level kernel's 32-bit indices hold
struct CoarseForm { bool twolevel, mfma; };
inline CoarseForm coarse_form(const PlanFacts &f, int w, bool own, bool tl_batch)
{
    CoarseForm c;
    c.twolevel = own && tl_batch && f.tl_use && f.tl_G > 0 && w <= 64 && (f.d & 3) == 0 && (size_t)4 * f.d * 4 + 4 * 64 * 8 <= (size_t)(96 << 10);
    c.mfma = own && !c.twolevel && f.allow_mfma && w <= 48 && f.kc >= f.mfma_min_kc && (f.d & 3) == 0;
    return c;
}

// what both planners start from ...
inline Plan plan_begin(const PlanFacts &f, int64_t nq, int K, int w, bool pre)
{
    Plan pl;
    pl.small_k = K <= 64;
    pl.small_w = w <= 64;
    pl.cap = sel_cap(K);
    pl.capw = sel_cap(w);
    const CoarseForm c = coarse_form(f, w, !pre, nq <= ((int64_t)1 << 30) / std::max(1, f.tl_G));
    pl.twolevel = c.twolevel;
    pl.coarse_mfma = c.mfma;
    return pl;
}

// ... the list-major ones go on, once pl.qg stands, with the chunk size (from ch0 points up; a forced one in multiples of align): enough
// work items to fill the chip, as few table rebuilds as possible.  Two items per CU is the measured optimum on billion-scale lists
// (SIFT1B-shape, 16..1024 queries, w = 1 and 8: every case at or within 5 % of its best chunk size; sixteen per CU rebuilt tables up
// to 15 times per probe)
inline Plan plan_chunks(const PlanFacts &f, int64_t nq, int w, double avg_len, uint32_t ch0, uint32_t align, Plan pl)
{
    const double ch = (double)nq * w * avg_len / pl.qg / (2.0 * f.num_cu);
    uint32_t CH = ch0;
    // (cap 2^18 points: on the billion-scale shapes a chunk then covers a whole list -- one table build and one selector
    // warm-up per (list, query group) instead of two: SIFT1B-shape scan 8.64 -> 7.45 ms at w = 8, 1.87 -> 1.69 ms at w = 1)
    while ((double)CH < ch && CH < (1u << 18)) CH <<= 1;
    if (f.force_chunk > 0) CH = (uint32_t)align_up((size_t)f.force_chunk, align);
    while ((f.maxlen + CH - 1) / CH > 64) CH <<= 1;   // bound the partial-result slots per probe
    pl.CH = CH;
    pl.maxch = (int)std::max<int64_t>(1, (f.maxlen + CH - 1) / CH);
    return pl;
}

// ... and both end with: sub-batches so the workspace stays inside the budget (partials: the list-major plans' partial results per probe and chunk)
inline Plan plan_subbatch(const PlanFacts &f, int64_t nq, int K, int w, bool partials, Plan pl)
{
    const size_t per_q = (pl.twolevel ? (size_t)f.tl_G : (size_t)f.kc) * 4 + (partials ? (size_t)w * pl.maxch * ((size_t)K * 8 + 4) : 0) +
                         (size_t)w * 20 + (size_t)K * 8 + 64;
    int64_t nb = (int64_t)std::max<size_t>(64, f.ws_budget / per_q);
    nb = std::min<int64_t>(nb, (int64_t)1 << 22);                                   // kernel arguments are 32-bit
    nb = std::min<int64_t>(nb, std::max<int64_t>(64, ((int64_t)1 << 30) / std::max(1, w * pl.maxch)));
    pl.nb = std::min<int64_t>(nq, nb);
    return pl;
}

// ---- how many probes a query-major round takes is a question about the DATA ---------------------------------------------------------
// Two probes per round share every codeword fetch between two tables -- right when most probes are scanned; one probe per round lets
// exact pruning look at the bound after EVERY list -- right when the bound the closest cells leave prunes most of the rest.  SIFT1M
// shape, two batches in flight (profiles/r05_pg12_matrix.txt): clustered data (93 % of the probed points pruned) 49.6 M q/s with one
// probe per round against 44.8 M with two, w = 32 41.5 against 31.5 M; data where nothing prunes 19.5 against 22.5 M.  The scan kernels
// count probed and pruned points anyway (ivfadc_stats); every few searches a 4 KB snapshot of the counters follows the scan on the
// stream into pinned memory, and a later search that finds it arrived (hipEventQuery: no wait, ever) folds the pruned fraction into
// the handle's prune_est (fb_poll / fb_snapshot in ivfadc_hip.hip).  Plans change with it, results cannot (every plan returns the reference's bytes).
constexpr float PG1_MIN_PRUNED = 0.6f;

// U = UInt16 (u16scan.hip.h): always list-major; K <= 64 on register selectors, 64 < K on LDS selectors where table mode 10 asks for
// them (search_dev sends larger K to the generic path otherwise).  Pairs per work item from the expected probes per list (a codeword
// read serves every pair of the item), halved for K > 64 until the selector buffers fit; chunks of whole passes, about two items per CU.
// Table-free (ivfadc_set_u16_tables): 1 always; 2 where a pass holds fewer points, weighted by what a gather costs, than a table has
// entries: min(avg_len, U16_PASS) * U16_DIRECT_COST <= ksub.
inline Plan make_plan_u16(const PlanFacts &f, int64_t nq, int K, int w, bool pre = false)
{
    Plan pl = plan_begin(f, nq, K, w, pre);
    const double avg_len = (double)f.n / std::max(1, f.kc);
    const bool tfree = f.u16_tables == 1 || (f.u16_tables == 2 && std::min(avg_len, (double)U16_PASS) * (double)U16_DIRECT_COST <= (double)f.ksub);
    pl.form = tfree ? (pl.small_k ? ScanForm::U16Direct : ScanForm::U16DirectWide) : (pl.small_k ? ScanForm::U16 : ScanForm::U16Wide);
    auto lds_of = [&](int g) {
        if (tfree) return pl.small_k ? u16_direct_lds_bytes(f.m, f.dsub) : u16_direct_wide_lds_bytes(f.m, f.dsub, g, pl.cap);
        return pl.small_k ? u16_lds_bytes(f.m, f.dsub) : u16_wide_lds_bytes(f.m, f.dsub, g, pl.cap);
    };
    const double ppl = (double)nq * w / std::max(1, f.kc);
    int qg = ppl >= 6.0 ? 8 : (ppl >= 2.5 ? 4 : (ppl >= 1.25 ? 2 : 1));
    if (f.force_qg == 1 || f.force_qg == 2 || f.force_qg == 4 || f.force_qg == 8) qg = f.force_qg;
    if (!pl.small_k)   // 4 x qg x cap keys beside the tables: m dsp + qg cap <= 4091, table-free <= 5115 (u16scan.hip.h)
        while (qg > 1 && lds_of(qg) > LDS_MAX) qg >>= 1;
    pl.qg = qg;
    pl.lds = lds_of(qg);
    if (pl.lds > LDS_MAX) { pl.fits = false; return pl; }
    pl = plan_chunks(f, nq, w, avg_len, U16_PASS, U16_PASS, pl);
    return plan_subbatch(f, nq, K, w, true, pl);
}

// query-major: one workgroup per query, no grouping, no partial results
inline Plan plan_query_major(const PlanFacts &f, int64_t nq, int w, bool pre, Plan pl)
{
    // large kc: the selection is a 4*kc-byte stream per query, better done by the lean stand-alone kernel
    pl.fuse_topw = pl.small_w && f.kc <= 8192 && f.force_qg != -3 && !pl.twolevel && !pre;
    // Several batches in flight on this replica (the index has views, or this IS a view: ivfadc_search_batches' second lane, a serving
    // loop's lanes): what bounds the chip then is register-file time, not one launch's latency -- and the fused selection holds a scan
    // workgroup's four waves and 126 VGPRs each for the 10 k cycles (28 % of its life on the SIFT1M shape, by phase stamps) in which
    // wave 0 selects and the others wait.  A stand-alone selection, one lean wave per query, costs a launch and gives the scan its
    // registers back: 42.5 -> 44.7 M q/s with two batches in flight (profiles/r05_topw_probe.txt); one batch at a time keeps the fused form.
    // (device-pointer entries only, and only while the lanes really run side by side -- PlanFacts::lanes_active, from the handle's dev_entry,
    // set by the entry from the root index's tickets: the host entries are bound by the host's enqueue time, where one more launch per batch costs
    // ivfadc_search_batches 27.8 -> 25.8 M q/s, and a caller who owns views but searches one batch at a time would pay a launch for nothing)
    pl.lanes = f.lanes_active && nq >= 4 * (int64_t)f.num_cu && f.kc >= 512;
    if (pl.lanes) pl.fuse_topw = false;
    // probes per round: share each codeword fetch between PG tables, keep >= 4 workgroups per CU when possible
    int pg = w >= 2 ? 2 : 1;   // measured: PG=2 beats PG=4 (register pressure halves the occupancy at 4)
    if (pl.small_k && f.allow_prune && f.prune_est >= PG1_MIN_PRUNED) pg = 1;   // (fb_poll: most of what is probed gets pruned)
    while (pg > 1 && scan_lds_bytes(f.m, f.d, pg, pl.cap, pl.small_k) > (size_t)(40 << 10)) pg >>= 1;
    pl.qg = pg;
    pl.lds = scan_lds_bytes(f.m, f.d, pg, pl.cap, pl.small_k);
    // lower-bound tables on the matrix cores: four probes per round share one pass over the codebook (a quarter of the exact
    // build's L1 traffic, a fraction of its vector-ALU work); register selectors and the LDS probe copy only
    // (measured: m = 48, where the exact build re-reads 768 KB of codewords per probe, +20 % on the HD shape; m = 16 with 1.5 k-point
    // lists -- the Deep1B shape -- loses 12 %: four barriers and the round's setup per four 24 KB lists cost what the cheaper tables
    // save, so there the rounds run only on request, ivfadc_set_table_mode(h, 2))
    const bool lb = f.allow_lb && f.allow_filt && f.have_lb_operands && lb_shape(f.m, f.dsub) && pl.small_k && w <= 32 &&
                    f.ksub == 256 && (f.m >= 32 || f.force_lb);
    pl.form = lb ? ScanForm::QueryMajorLb : ScanForm::QueryMajor;
    if (lb) {
        // the top-w selection of a large batch runs as its own launch, one wave per query at full occupancy (per-tile records,
        // no score matrix); inside this kernel -- two workgroups per CU, three waves idle -- it was a sixth of the launch
        if (nq >= 4 * (int64_t)f.num_cu || pl.twolevel) pl.fuse_topw = false;
        pl.qg = w >= 3 ? 4 : w;
        pl.lds = lb_lds_bytes(f.m, f.dsub, pl.qg);
    }
    if (pl.lds > LDS_MAX) pl.fits = false;   // e.g. m = 48 with K near 2048: tables + selector buffers
    return pl;
}

// list-major: work items of (list, group of qg queries that probe it, chunk of CH points), partial results merged behind the scan
inline Plan plan_list_major(const PlanFacts &f, int64_t nq, int K, int w, double avg_len, bool long_lists, bool forced, Plan pl)
{
    // query-group width from the expected number of probes per list
    const double ppl = (double)nq * w / std::max(1, f.kc);
    int qg = ppl >= 2.5 ? 4 : (ppl >= 1.25 ? 2 : 1);
    // billion-scale lists (a list is megabytes: the stream, not the per-item work, is what a group shares): wider groups pay
    // much earlier.  SIFT1B shape, step in ms at QG = 1 / 2 / 4 (profiles/r03_a_sift1b_plan_sweep.txt): probes per list 0.125:
    // 0.26 / 0.30 / 0.38; 0.25: 0.45 / 0.42 / 0.54; 0.5: 0.90 / 0.70 / 0.81; 1.0: 1.55 / 1.07 / 1.15; 2.0: 2.93 / 1.81 / 1.57
    // -- the regime of one rank of an 8-GPU run on a 16 384-query batch (2048 queries, w = 8)
    if (long_lists) qg = ppl >= 1.5 ? 4 : (ppl >= 0.2 ? 2 : 1);
    // ... and where the eight-wave kernel exists (it is planned below for groups of four) it pays from half a probe per list: scan ms of
    // the SIFT1B shape at 0.25 / 0.5 / 1 probes per list, eight-wave kernel against scan_kernel<QG=2>: 0.355 / 0.525 / 0.70-0.75 against
    // 0.316 / 0.544 / 0.92-0.93 (round 6)
    // (K the kernel's pool holds: 64, or 128 where table mode 8 / 9 asks for the wide pool -- a request, so wg8_mode > 0 there)
    const bool w8_k = pl.small_k || (K <= W8_WIDE_MAX_K && f.wg8_wide && f.wg8_mode > 0 && f.m == 8);
    // ... the kernel exists for the index and may run: every admission below is this and a reason to take it
    // (positions and byte offsets of a list are 28- / 31-bit quantities in the kernel: lists of fewer than 2^28 points; m = 16: 27-bit
    // lists -- a point is 16 bytes -- and on request only: w8_md)
    const bool w8_base = w8_k && f.allow_filt && f.wg8_mode >= 0 && w8_md(f) && f.ksub == 256 && f.maxlen < w8_maxlen(f);
    const bool w8_shape = w8_base && (f.wg8_mode > 0 || w8_default(f)) && avg_len >= 8192.0;
    if (long_lists && w8_shape && ppl >= 0.5) qg = 4;
    if (forced) qg = f.force_qg;
    // eight queries per code stream behind the 4-bit narrow-field filter (nfscan.hip.h): conflict-free gathers, a third of the vector
    // instructions per (query, point), every list streamed once per eight queries -- where the shape has the kernel, K fits the
    // register selectors and the lists are probed often enough to fill the groups
    // (measured, SIFT1B shape, 16 384 x w = 8: 7.76 ms against 7.44 ms for the 16-bit four-query kernel -- DESIGN.md 4.11 -- so the kernel
    // runs on request only: ivfadc_set_tuning(h, 8, 0))
    const bool nf_ok = f.allow_nf && f.allow_filt && f.have_nf_operands && nf_shape(f.m, f.dsub) && f.ksub == 256 && pl.small_k;
    if (f.force_qg == 8 && !nf_ok) qg = 4;
    if (nf_ok && f.force_qg == 8) {
        pl.form = ScanForm::NarrowField;   // (nf_scan_kernel<4>: plan_kernel)
        pl.qg = qg = 8;
        pl.lds = (size_t)NfLds::END;
    } else {
        // keep two workgroups per CU when possible (a forced width only yields to the hard LDS limit)
        // (groups of four that the wide-pool kernel takes below need none of the four-wave kernel's LDS selectors: its budget does not narrow them)
        // (... nor do the groups of four of an m = 16 index that the kernel takes on request: the four-wave kernel's 64 KB of f32 tables are not built)
        const bool w8_wide_ok = w8_base && f.wg8_mode > 0 && (!pl.small_k || f.m == 16);
        // the four-wave kernel's striped form (and at m = 8 its 16-bit integer filter), and its LDS need, at a width
        auto stripe_at = [&](int g) { return f.allow_filt && filt_shape(f.m, f.dsub) && g == 4 && f.ksub == 256; };
        auto lds_at = [&](int g) { return scan_lds_bytes(f.m, f.d, g, pl.cap, pl.small_k, true, stripe_at(g)); };
        while (qg > 1 && !(qg == 4 && w8_wide_ok) && lds_at(qg) > (forced ? LDS_MAX : (size_t)(80 << 10))) qg >>= 1;
        if (!(qg == 4 && w8_wide_ok) && lds_at(qg) > LDS_MAX) { pl.fits = false; return pl; }
        // four queries per code stream on long lists of the m = 8 / dsub = 16 shape: the eight-wave kernel (a work item must feed
        // eight waves: lists of at least 8 K points).  Measured on the SIFT1B shape against the four-wave kernel (profiles/r06_w8_sweep.txt,
        // the eight-wave kernel with its workgroup pool): 16 384 queries, scan ms at w = 1 / 8: 1.36 / 5.73 against 1.68 / 7.46;
        // 2048 x w = 8: 1.06 against 1.47.
        // (The list-partitioned mode needs nothing of the kernel: the partition is applied in front of it -- the top-w kernel counts this rank's
        // lists only into list_cnt, which bucket_scan_kernel turns into work items and item_list, bucket_scatter_kernel drops the other
        // ranks' probes -- and behind it, in merge_kernel; a rank's work items are ordinary ones)
        // (w = 1 too since the workgroup pool: 1.36 against the four-wave kernel's 1.67 ms)
        if (qg == 4 && w8_base && (f.wg8_mode > 0 || (w8_default(f) && avg_len >= 8192.0))) {
            pl.form = ScanForm::EightWave;
            pl.wide = !pl.small_k;
            // ... and EIGHT queries per code stream (wg8_scan_kernel<8>: 16-byte entries, 32 instead of 48 instructions per point and eight queries)
            // where the lists are probed often enough to fill groups of eight (table mode 7: wherever the kernel exists)
            pl.q8 = f.wg8_mode == 2 || (f.wg8_mode == 0 && !forced && ppl >= W8_Q8_MIN_PPL);
            if (pl.q8) qg = 8;
            pl.lds = f.m == 16 ? (pl.q8 ? (size_t)W8Lds<8, 1, 16>::END : (size_t)W8Lds<4, 1, 16>::END)
                   : pl.wide   ? (pl.q8 ? (size_t)W8Lds<8, 2>::END : (size_t)W8Lds<4, 2>::END)
                               : (pl.q8 ? (size_t)W8Lds<8>::END : (size_t)W8Lds<4>::END);
            pl.threads = W8_THREADS;
        } else {
            pl.form = ScanForm::FourWave;
            pl.stripe = stripe_at(qg);
            pl.lds = lds_at(qg);
        }
        pl.qg = qg;
    }
    return plan_chunks(f, nq, w, avg_len, 4096, 1024, pl);
}

inline Plan make_plan(const PlanFacts &f, int64_t nq, int K, int w, bool pre = false)   // pre: the probes are the caller's (SearchCall::pre_list): no coarse stage of any kind
{
    Plan pl = plan_begin(f, nq, K, w, pre);
    const double avg_len = (double)f.n / std::max(1, f.kc);
    // list-major (queries that probe a list share its code stream; per-item grouping/merge overhead) wins when
    // the lists are very long (a query's probe must be split over workgroups anyway), or when a list is probed by
    // enough queries to fill the groups AND the batch makes enough work items to fill the chip; otherwise
    // query-major (one workgroup per query, no grouping, no partial results).  Measured crossovers, m = 8,
    // kc = 8192, 16 probes/list: list-major ahead from 10 KB lists on (1.74 vs 1.90 ms); SIFT1M-shape (8
    // probes/list but only 2048 work items): query-major 92 vs 190 us; Deep1B-shape (4.9 probes/list): query-major.
    const double ppl_ = (double)nq * w / std::max(1, f.kc);
    const bool long_lists = avg_len * f.m > 256.0 * 1024.0;
    // ... and the lists are long enough to amortise a fresh selection per (query, list): kc = 8192, 16 probes/list:
    // 3.7k-point lists 1.88 vs 2.01 ms, 12k 2.70 vs 3.28 ms for list-major; SIFT1M-shape (1k-point lists) with 16k-64k
    // queries: query-major 18-20 M q/s vs 12 M
    const bool shared = ppl_ >= 6.0 && (double)nq * w / 4.0 >= 64.0 * f.num_cu && avg_len >= 3072.0;
    // ... or when a handful of queries with heavy probes would leave most CUs idle at one workgroup per query: list-major
    // spreads a query's probes over workgroups (HD-shape, 64 queries: w = 8 0.39 vs 0.31 M q/s, w = 32 0.21 vs 0.10;
    // SIFT1M- and Deep1B-shape probes are too light for it: 1.4 vs 3.0 M and 0.2 vs 0.7 M q/s)
    const bool few_heavy = nq <= f.num_cu && w >= 8 && avg_len * f.m >= 64.0 * 1024.0;   // 256 queries: +10 % (w = 8), +60 % (w = 32); 512: even
    // ... or a very small batch with several probes each: one workgroup per query walks its w probes in sequence, list-major
    // (ungrouped: one work item per (query, probe), no bucket kernels) runs them side by side.  SIFT1M-shape, measured
    // query-major vs list-major per batch: 1 query w = 8 42 vs 35 us, w = 16 64 vs 42 us, w = 32 118 vs 56 us; even at
    // 64 queries for w = 8 / 16; w <= 4 stays query-major (30 vs 33 us).  Not with a large kc, where the per-list
    // bookkeeping of the list-major plan costs more than it buys (Deep1B-shape 380 vs 234 us)
    const bool few_many = w >= 8 && nq <= 32 + (int64_t)w && nq <= f.num_cu / 4 && f.kc <= 8192;
    bool query_major = !(long_lists || shared || few_heavy || few_many);
    if (f.force_qg == -1 || f.force_qg == -3) query_major = true;
    if (f.part_n > 1) query_major = false;   // list-partitioned mode: the list-major plan is the one that skips other ranks' lists
    const bool forced = (f.force_qg == 1 || f.force_qg == 2 || f.force_qg == 4 || f.force_qg == 8);
    if (forced) query_major = false;
    pl = query_major ? plan_query_major(f, nq, w, pre, pl) : plan_list_major(f, nq, K, w, avg_len, long_lists, forced, pl);
    return pl.fits ? plan_subbatch(f, nq, K, w, !query_major, pl) : pl;
}

// The masked search of an 8-bit handle (ivfadc_search_masked; masked_scan_kernel<QG, SMALL> in maskset.hip.h: any m, dsub, ksub <= 256):
// always list-major -- the mask rows are per list, and the queries that probe a list share its code stream whatever their masks.  Width
// from the probes-per-list rule of plan_list_major, narrowed until the four-wave layout without stripes fits two workgroups per CU (a
// forced width yields to the hard limit only); !fits sends the search to the masked generic path.  No latency path, no fused top-w.
inline Plan make_plan_masked(const PlanFacts &f, int64_t nq, int K, int w)
{
    Plan pl = plan_begin(f, nq, K, w, false);
    pl.form = ScanForm::Masked;
    const double avg_len = (double)f.n / std::max(1, f.kc);
    const double ppl = (double)nq * w / std::max(1, f.kc);
    int qg = ppl >= 2.5 ? 4 : (ppl >= 1.25 ? 2 : 1);
    const bool forced = f.force_qg == 1 || f.force_qg == 2 || f.force_qg == 4;
    if (forced) qg = f.force_qg;
    auto lds_at = [&](int g) { return scan_lds_bytes(f.m, f.d, g, pl.cap, pl.small_k, true, false); };
    while (qg > 1 && lds_at(qg) > (forced ? LDS_MAX : (size_t)(80 << 10))) qg >>= 1;
    pl.qg = qg;
    pl.lds = lds_at(qg);
    if (pl.lds > LDS_MAX) { pl.fits = false; return pl; }
    pl = plan_chunks(f, nq, w, avg_len, 4096, 1024, pl);
    return plan_subbatch(f, nq, K, w, true, pl);
}

}  // namespace ivf
