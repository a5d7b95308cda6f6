// scan_layouts.h -- what the search plan (plan.h) has to know about the scan kernels: their dynamic-LDS layouts and sizes, the shapes
// they are instantiated for, the limits their index arithmetic sets.  Plain C++ (no HIP type), so the plan compiles and runs without
// a GPU (tests/c/plan_check.cpp); the kernel headers include this file and read the very same names, namespace ivf:
//   wg8scan.hip.h   W8_*, W8Lds, w8_ds_ok           nfscan.hip.h    NF_*, NfLds
//   u16scan.hip.h   U16_*, u16_*_lds_bytes          lbscan.hip.h    LbCfg (lb_lds_bytes: its END and the four-wave tail)
//   kernels.hip.h   carve_lds: FwLds / FwTail, whose end scan_lds_bytes returns (the carve adds up the lengths FwLds is made of and takes
//                   the tail's offsets from fw_tail)                   smallq.hip.h    SqLds (sq_lds_bytes)
#pragma once

#include <cstddef>
#include <cstdint>

typedef unsigned int u32;   // (as kernels.hip.h and wave_sort.hip.h have it)

namespace ivf {

constexpr size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
constexpr int pow2ceil(int x) { int p = 1; while (p < x) p <<= 1; return p; }

// ---- the eight-wave list-major kernel (wg8scan.hip.h) --------------------------------------------------------------------------------
// Waves per workgroup.  Measured with more (round 6; the table build is laid out for 512 threads, further waves repeat the first ones' share --
// the same values to the same places): TEN (640 threads at <= 96 registers) run one workgroup per CU -- a workgroup's waves spread 3-3-2-2
// over the SIMDs, two of them would need six register sets on a SIMD -- 9.6 ms; TWELVE (<= 80 registers: the scan loop still holds no
// spilled register, the candidate path 150) run two per CU and take 9.1 ms, 8.5 without candidates against 5.0: six waves per SIMD on the
// same LDS are slower than four, whatever the guide's 2 cycles per ds_read_b64 leave free on paper.
constexpr int W8_NW = 8;
constexpr int W8_THREADS = 64 * W8_NW;
constexpr int W8_ES = 3;                      // dwords per parked point: code bytes (2), list position (m = 16: W8Lds::ES = 5, four dwords of code bytes)
constexpr u32 W8_TAB_BYTES = 256u * 256u;     // 256 codes x (32 / NQ copies x 8 sub-quantizers x 2 NQ bytes; m = 16: 16 / NQ copies x 16 sub-quantizers)

// KP: the pool's entries per lane (1: K <= 64, the layout of every measurement so far; 2: K <= 128, the wide pool -- see w8_pool_offer)
// M: sub-quantizers (8, or 16: SIXTEEN SUB-QUANTIZERS in wg8scan.hip.h).  Two sizes depend on it, both behind the pool, so everything the helpers
// there read at fixed addresses stands where it stood: a parked point takes five dwords instead of three (16 code bytes), and the residuals
// -- 16 x (DS + 1) x NQ x 4 B, 576 NQ bytes at DS = 8, which the block sized for m = 8 / DS = 16 (544 NQ bytes) does NOT hold -- are built
// where the rings are: the rings are empty from the end of a work item's scan to the start of the next one's, the residuals live from
// the top of a work item to the barrier behind its table build, and barriers separate the two (RESB; at m = 16 the block at RES is unused).
template <int NQ, int KP = 1, int M = 8> struct W8Lds {
    static_assert(NQ == 4 || NQ == 8, "four or eight queries per code stream");
    static_assert(KP == 1 || KP == 2, "one or two pool entries per lane");
    static_assert(M == 8 || (M == 16 && KP == 1), "eight sub-quantizers, or sixteen with the one-entry-per-lane pool");
    static constexpr u32 ES = M == 8 ? (u32)W8_ES : 5u;      // dwords per parked point: M / 4 of code bytes, list position
    static constexpr u32 RES = W8_TAB_BYTES;                  // f32 residuals [ii][t][s]: 8 x (DS x NQ + NQ of padding) x 4 B, sized for DS = 16 (W8_RES_STRIDE)
    static constexpr u32 SMAX = RES + 8u * (16u * NQ + NQ) * 4u;   // u32 [NQ]: bits of the per-query largest entry (atomicMax); f32 inv[NQ] behind
    static constexpr u32 QC = SMAX + 8u * NQ;                 // f32 dc[NQ]; u32 visit-order base[NQ]; u32 probe index[NQ]; u32 query[NQ]
    static constexpr u32 HARD = QC + 16u * NQ;                // u64 [NQ]: the bounds the item started from
    static constexpr u32 STHR = HARD + 8u * NQ;               // u64 [NQ]: workgroup-shared bounds
    static constexpr u32 SWI = STHR + 8u * NQ;                // u32 [4]
    static constexpr u32 POOL = SWI + 16u;                    // u64 [NQ][64 KP]: the workgroup's K smallest keys per slot, unordered (w8_pool_offer)
    static constexpr u32 POOL_SLOT = 64u * KP * 8u;           // bytes of a slot's pool
    static constexpr u32 PARK = POOL + NQ * POOL_SLOT;        // u32 [8][32][W8_ES]: the waves' rings of parked points (W8_RING)
    static constexpr u32 COLD = PARK + (u32)W8_NW * 32u * ES * 4u;     // u32 [NQ][16]: a cold work item's first step, every wave's ceil(K / 8)-th smallest integer sum per slot
    // (KP = 1: up to sixteen waves; the wide pool's 8 NQ more entries leave the eight-query form room for the eight waves there are: u32 [NQ][8])
    static constexpr u32 COLD_SLOT = KP == 1 ? 64u : 4u * (u32)W8_NW;
    static constexpr u32 END = COLD + COLD_SLOT * NQ;
    static constexpr u32 RESB = M == 8 ? RES : PARK;          // where the residuals are built
    static_assert(END <= 80u * 1024u, "two workgroups per CU");
    static_assert((HARD & 7u) == 0 && (STHR & 7u) == 0 && (POOL & 7u) == 0, "8-byte bounds");
    static_assert(M == 8 || 16u * (8u + 1u) * NQ * 4u <= COLD - PARK, "m = 16: the residuals of DS <= 8 fit the rings' block");
    static_assert((RESB & 15u) == 0, "16-byte residual rows");
};
static_assert(W8Lds<4>::END == 73264u && W8Lds<8>::END == 77904u, "the layout the plan's LDS figures and the measurements were taken with");
static_assert(W8Lds<4, 2>::END == 75184u && W8Lds<8, 2>::END == 81744u, "the wide pool's layouts: 2 / 4 KB more pool, 32 B per slot of cold-start words");
static_assert(W8Lds<4, 2>::POOL == W8Lds<4>::POOL && W8Lds<8, 2>::POOL == W8Lds<8>::POOL, "everything in front of the pool stands where the helpers below read it");
static_assert(W8Lds<4, 1, 16>::END == 75312u && W8Lds<8, 1, 16>::END == 79952u, "m = 16: 2 KB more of rings (five dwords per parked point), nothing else");
static_assert(W8Lds<4, 1, 16>::PARK == W8Lds<4>::PARK && W8Lds<8, 1, 16>::PARK == W8Lds<8>::PARK, "m = 16: everything up to the rings stands where it stood");

// Sub-space widths the kernel is instantiated for (d = 8 DS), and the residuals' floats per sub-quantizer: DS rows of NQ queries and ONE row
// of padding.  A quad of the table build reads the rows of four neighbouring sub-quantizers at once, 16 B per lane (NQ = 8: 16 B of a
// 32-byte row): sub-quantizer ii's block starts (DS + 1) ii rows on, and DS + 1 is ODD for every DS here, so ii -> (DS + 1) ii is
// one-to-one modulo 16 four-bank groups (NQ = 4: 17, 13, 9 and 5 ii mod 16 are four different groups for ii = 0 .. 3 and for 4 .. 7) and
// modulo 8 eight-bank groups (NQ = 8): the quad's four lanes read four different bank groups at DS = 4, 8, 12 and 16 alike.  Without
// the padding row the blocks would start DS ii rows apart: the same group twice or four times over (DS = 16: always the same one).
constexpr bool w8_ds_ok(int ds) { return ds == 4 || ds == 8 || ds == 12 || ds == 16; }

// ---- the narrow-field list-major kernel (nfscan.hip.h) -------------------------------------------------------------------------------
constexpr int NF_QG = 8;                       // queries per code stream
constexpr u32 NF_TAB_BYTES = 256u * 256u;      // 256 codes x (8 sub-quantizers x 2 copies x 16 bytes)
constexpr int NF_POOL = 128;                   // parked (point, query) pairs per wave; drained from 64 on
constexpr int NF_ES = 4;                       // dwords per parked pair: code bytes (2), list position, integer sum << 8 | query slot

// LDS behind the table (byte offsets)
struct NfLds {
    static constexpr u32 RES = NF_TAB_BYTES;                  // f32 residuals [s][t4][ii][4]: 8 x 4 x 8 x 16 B = 4 KB
    static constexpr u32 RN2 = RES + 4096u;                   // f32 [ii][s]: ||r_s,ii||^2 (1 - 2^-17)
    static constexpr u32 SMIN = RN2 + 256u;                   // u32 [ii][s]: ordered bits of min_c e          (atomic)
    static constexpr u32 SMAX = SMIN + 256u;                  // u32 [ii][s]: ordered bits of max_c e          (atomic)
    static constexpr u32 BASE = SMAX + 256u;                  // f32 [ii][s]: base
    static constexpr u32 QC = BASE + 256u;                    // f32 [4][8]: inv_s, sum of bases, dc_s, nn_s (sum over ii of max ||cb||^2 + ||r||^2)
    static constexpr u32 QI = QC + 128u;                      // u32 [3][8]: probe index, query, visit-order base of slot s
    static constexpr u32 HARD = QI + 96u;                     // u64 [8]: the bounds the item started from (from outside the workgroup)
    static constexpr u32 STHR = HARD + 64u;                   // u64 [8]: workgroup-shared bounds
    static constexpr u32 SCNT = STHR + 64u;                   // int [4][8]
    static constexpr u32 SWI = SCNT + 128u;                   // u32 [4]
    static constexpr u32 TW = SWI + 16u;                      // int [4][8]: each wave's integer budgets of the moment (read by lane-varying slot)
    static constexpr u32 POOL = TW + 128u;                    // u32 [4][NF_POOL][NF_ES]
    static constexpr u32 END = POOL + 4u * NF_POOL * NF_ES * 4u;
};
static_assert(NfLds::END <= 80u * 1024u, "two workgroups per CU");
static_assert((NfLds::POOL & 15u) == 0, "16-byte pool entries");
static_assert((NfLds::HARD & 7u) == 0, "8-byte bounds");

// ---- the UInt16 list-major kernels (u16scan.hip.h) -----------------------------------------------------------------------------------
constexpr int U16_P = 8;                    // (query, probe) pairs per work item, at most
constexpr int U16_PPT = 4;                  // points per thread and pass
constexpr int U16_PASS = 256 * U16_PPT;     // points per pass
constexpr int U16_TAB_FLOATS = 8192;        // table area: 32 KB, P x T floats (T = codewords per tile)
constexpr int U16_XCH_FLOATS = 4 * U16_P * 64 * 2;   // the table-free K <= 64 entry keeps only the wave-merge exchange: 4 x P x 64 keys, 16 KB
// ivfadc_set_u16_tables(h, 2): table-free iff min(avg_len, U16_PASS) * U16_DIRECT_COST <= ksub.  The arithmetic alone says 1, and the
// measurement leaves it there: at k = 1024 the table-free scan is ahead at every avg_len of 128 ... 2048 (no crossover, so <= 1), at
// k = 256 and avg_len 977 the tables are (so > 0.262); 1 is the largest such value (profiles/u16_direct.json)
constexpr float U16_DIRECT_COST = 1.0f;

// dynamic LDS of u16_scan_kernel: residuals [P][m][dsp] (dsp = dsub rounded up to 4: one 16-byte read serves four terms), table area
// (the wave-merge exchange, 4 x P x 64 keys = 16 KB, aliases it), per-wave counts, two words of work-queue / verdict exchange
static inline size_t u16_lds_bytes(int m, int dsub)
{
    return (size_t)U16_P * m * (((size_t)dsub + 3) & ~(size_t)3) * 4 + (size_t)U16_TAB_FLOATS * 4 + 4 * U16_P * 4 + 16;
}

// ... of u16_wide_scan_kernel: the selector buffers [4 waves][qg][cap] u64 between the table area and the small words
static inline size_t u16_wide_lds_bytes(int m, int dsub, int qg, int cap)
{
    return u16_lds_bytes(m, dsub) + (size_t)4 * qg * cap * 8;
}

// ... of the table-free entries: no table area
static inline size_t u16_direct_lds_bytes(int m, int dsub)
{
    return (size_t)U16_P * m * (((size_t)dsub + 3) & ~(size_t)3) * 4 + (size_t)U16_XCH_FLOATS * 4 + 4 * U16_P * 4 + 16;
}
static inline size_t u16_direct_wide_lds_bytes(int m, int dsub, int qg, int cap)
{
    return (size_t)U16_P * m * (((size_t)dsub + 3) & ~(size_t)3) * 4 + (size_t)4 * qg * cap * 8 + 4 * U16_P * 4 + 16;
}

// ---- the four-wave kernels (kernels.hip.h: scan_kernel, qscan_kernel; maskset.hip.h: masked_scan_kernel; smallq.hip.h: sq_kernel) -----
// shapes the striped list-major kernels exist for (IVF_SHAPES with m = 8 / 16)
inline bool filt_shape(int m, int dsub) { return (m == 8 && dsub == 16) || (m == 16 && (dsub == 6 || dsub == 8)); }

// the shape the narrow-field list-major kernel exists for (nfscan.hip.h)
inline bool nf_shape(int m, int dsub) { return m == 8 && dsub == 16; }

constexpr int STHR_WORDS = 5;                 // u64 words per slot of the workgroup-shared bounds: the bound, the four waves' quarter keys (arm_bound)
constexpr int CAND_CAP = 16;                  // parked points per wave (striped list-major kernel: drain_parked)
constexpr int cand_stride(int m) { return m / 4 + 1; }   // dwords of a parked point: code bytes, list position
constexpr u32 QF_OFF = 8u * 256u * 4u * 4u;   // the 16-bit table sits right behind the m = 8, QG = 4 float tables (32 KB)
constexpr u32 QF_BYTES = 256u * 64u;

// The tail of a four-wave carve (byte offsets), which the matrix-core rounds put behind LbCfg::END as it stands:
//   scnt [4][qg] int, swi [4] u32, sthr [qg][STHR_WORDS] u64
//   probes: 768 B, the query-major kernel's LDS copy of the query's probes.  w <= 32: list, coarse distance, visit-order base, length and
//     code offset, 32 entries each, and behind these five arrays 128 B of scratch -- wbound u64 [4], ccnt u32 [2] and flag of the short-row
//     and tiled selections; 32 < w <= 64 (fused top-w only): list, distance and base at 64 entries each, which fill the 768 B.  Before the
//     probes are written the area is refine_probes_wg's scratch (66 ints).
//   park: the striped list-major kernel's parking buffers, CAND_CAP entries of cand_stride(m) dwords for each of the four waves; sized
//     for m = 16 (m = 8 leaves its last 512 B unused)
constexpr size_t FW_PROBE_BYTES = 768;
constexpr int FW_PROBES_CACHED = 32, FW_PROBES_WIDE = 64;   // entries of a probe array: w <= FW_PROBES_CACHED (five arrays), or up to 64 (three)
constexpr int fw_probe_entries(int w) { return w <= FW_PROBES_CACHED ? FW_PROBES_CACHED : FW_PROBES_WIDE; }
constexpr size_t FW_PARK_BYTES = (size_t)4 * CAND_CAP * cand_stride(16) * 4;
struct FwTail {
    size_t scnt, swi, sthr, probes, wbound, ccnt, flag, park, end;
};
constexpr FwTail fw_tail(size_t base, int qg, bool park = false)
{
    FwTail t{};
    t.scnt = base;
    t.swi = t.scnt + (size_t)4 * qg * 4;
    t.sthr = align_up(t.swi + 4 * 4, 8);
    t.probes = t.sthr + (size_t)qg * STHR_WORDS * 8;
    t.wbound = t.probes + 5 * 32 * 4;
    t.ccnt = t.wbound + 4 * 8;
    t.flag = t.ccnt + 2 * 4;
    t.park = t.probes + FW_PROBE_BYTES;
    t.end = t.park + (park ? FW_PARK_BYTES : 0);
    return t;
}
static_assert(fw_tail(0, 1).flag + 4 <= fw_tail(0, 1).park, "the scratch words lie in the 128 B the 32-entry probe arrays leave free");
static_assert(3 * 64 * 4 == FW_PROBE_BYTES && 66 * 4 <= FW_PROBE_BYTES, "the 64-entry arrays fill the probe area; refine_probes_wg's scratch fits it");

// The whole carve.  The plan takes its end; carve_lds (kernels.hip.h) lets the regions in front of the tail follow each other at the
// lengths below (fw_tab_floats, fw_resid_floats, fw_selbuf_keys: typed pointer steps, which is what keeps the kernels' code as it was)
// and places the tail's pointers at fw_tail(0, QG)'s offsets from where it begins; tests/c/scan_lds_check.cpp checks that both agree
// with these offsets wherever the tail stands:
//   tab    [m][256][qg] f32, never smaller than 2 x 256 x qg: after the scan its first bytes are the exchange area of the register
//          selectors, xch [4][qg][64] u64 = 2 KB qg, which m = 1 would not hold
//   qf     m = 8 striped only (extra = QF_BYTES, at QF_OFF): the 16-bit integer filter table
//   resid  [d][qg] f32, rounded up to 16 bytes
//   selbuf [4][nsel][cap] u64, LDS selectors (K > 64: !small) -- nsel = qg in the list-major kernels, 1 in the query-major kernel, whose
//          qg tables all belong to one query
struct FwLds {
    size_t tab, qf, resid, selbuf;
    FwTail t;
};
constexpr size_t fw_tab_floats(int m, int qg) { return (size_t)(m < 2 ? 2 : m) * 256 * qg; }
constexpr size_t fw_resid_floats(int d, int qg) { return ((size_t)d * qg + 3) & ~(size_t)3; }
constexpr size_t fw_selbuf_keys(int nsel, int cap) { return (size_t)4 * nsel * cap; }
constexpr FwLds fw_lds(int m, int d, int qg, int nsel, int cap, bool small, size_t extra = 0, bool park = false)
{
    FwLds l{};
    l.tab = 0;
    l.qf = fw_tab_floats(m, qg) * 4;
    l.resid = l.qf + extra;
    l.selbuf = l.resid + fw_resid_floats(d, qg) * 4;
    l.t = fw_tail(l.selbuf + (small ? 0 : fw_selbuf_keys(nsel, cap) * 8), qg, park);
    return l;
}
static_assert(fw_lds(8, 128, 4, 4, 64, true, QF_BYTES).qf == QF_OFF, "the filter table's place is behind the m = 8, QG = 4 float tables");

// the plan's figure: the end of that carve.  stripe: the plan's (Plan::stripe), for the width qg; groups of four at m = 8 / 16 get the
// parking buffers, striped or not
constexpr size_t scan_lds_bytes(int m, int d, int qg, int cap, bool small, bool list_major = false, bool stripe = false)
{
    return fw_lds(m, d, qg, list_major ? qg : 1, cap, small, stripe && m == 8 ? QF_BYTES : 0, list_major && qg == 4 && (m == 8 || m == 16)).t.end;
}

// sq_kernel (smallq.hip.h): the carve of one query with register selectors; its probes at 64 entries each fill the probe area, and behind
// them come 64 B of the row selection's scratch -- wbound u64 [4], ccnt u32 [4], the gap to the next 16-byte boundary -- and, where the
// coarse search runs inside the launch, the row of kc_inside coarse distances (16-byte rows: the selection reads float4)
constexpr size_t SQ_SCRATCH_BYTES = 64;
struct SqLds {
    size_t s_list, s_dc, s_base, wbound, ccnt, row_lo, s_row, end;
};
// base: where the carve's tail begins (FwTail::scnt, a multiple of 16)
constexpr SqLds sq_tail(size_t base, int kc_inside)
{
    const FwTail t = fw_tail(base, 1);
    SqLds s{};
    s.s_list = t.probes;
    s.s_dc = s.s_list + 64 * 4;
    s.s_base = s.s_dc + 64 * 4;
    s.wbound = t.park;
    s.ccnt = s.wbound + 4 * 8;
    s.row_lo = s.ccnt + 4 * 4;
    s.s_row = align_up(s.row_lo, 16);
    s.end = s.wbound + SQ_SCRATCH_BYTES + (size_t)kc_inside * 4;
    return s;
}
constexpr SqLds sq_lds(int m, int d, int kc_inside) { return sq_tail(fw_lds(m, d, 1, 1, 64, true).t.scnt, kc_inside); }
static_assert(sq_tail(0, 0).s_row <= sq_tail(0, 0).end && sq_tail(8, 0).s_row <= sq_tail(8, 0).end, "the row starts inside the scratch block, whatever the gap");
constexpr size_t sq_lds_bytes(int m, int d, int kc_inside) { return sq_lds(m, d, kc_inside).end; }

// ---- the query-major kernel's matrix-core rounds (lbscan.hip.h, qscan_body<..., LB = true>) ------------------------------------------
// shapes the matrix-core lower-bound rounds (qscan_kernel<..., LB = true>) are instantiated for, and their instantiations (M, DS, PG)
inline bool lb_shape(int m, int dsub) { return (m == 48 && dsub == 16) || (m == 16 && dsub == 6); }
#define IVF_LB_SHAPES(X) X(48, 16, 1) X(48, 16, 2) X(48, 16, 3) X(48, 16, 4) X(16, 6, 1) X(16, 6, 2) X(16, 6, 3) X(16, 6, 4)

template <int M, int DS, int PG> struct LbCfg {
    static constexpr int DSP = (DS + 7) & ~7;            // sub-space width in whole 16-byte parts of bf16
    static constexpr int NP = DSP / 4;                   // parts per label: DSP hi + DSP lo bf16
    static constexpr int NCH = DSP / 4;                  // 4-wide k-chunks of the MFMA
    static constexpr u32 TS = (u32)M * 256u + 32u;       // one probe's u8 table; + 32 B: the PG tables start 8 banks apart
    static constexpr u32 TAB_BYTES = (PG * TS + 15u) & ~15u;
    static constexpr int DSR = (DS + 3) & ~3;            // a sub-space row of the f32 residuals, padded with zeros to whole 16-byte groups
    static constexpr u32 R_OFF = TAB_BYTES;              // f32 residuals r = q - c of the round's probes [PG][M][DSR] (coarsequantizers.jl:40-45)
    static constexpr u32 R_BYTES = (u32)PG * M * DSR * 4u;
    static constexpr u32 CST_OFF = R_OFF + R_BYTES;      // f32 [M][PG]: ||r_ii||^2
    static constexpr u32 BS_OFF = CST_OFF + (u32)M * PG * 4u;   // f32 [M][PG]: base
    static constexpr u32 PC_OFF = BS_OFF + (u32)M * PG * 4u;    // per probe: inv[4], sbase[4], range max bits[4], effective length[4]
    static constexpr u32 PP_OFF = PC_OFF + 128u;         // (+ nn[4]: sum over sub-quantizers of max ||cb||^2 + ||r_ii||^2, for the upper bound)
    static constexpr u32 LQ_OFF = PP_OFF + 256u;         // per probe of the QUERY (w <= 32): inv[32], sbase[32] -- the pool outlives a round
    static constexpr u32 PARK_OFF = LQ_OFF + (u32)M * DS * 4u;   // f32 query [M * DS]
    static constexpr int ES = M / 4 + 2;                 // parked entry: code dwords, visit order, (integer sum << 8 | probe of the query)
    static constexpr int PCAP = PG >= 4 ? 54 : 16;       // entries per wave (two workgroups per CU at PG = 4: LDS to spare)
    static constexpr u32 PARK_BYTES = 4u * PCAP * ES * 4u;
    static constexpr u32 UB_OFF = PARK_OFF + PARK_BYTES; // u64 [4][64]: the waves' upper-bound keys, exchanged at the round boundaries
    static constexpr u32 END = UB_OFF + 4u * 64u * 8u;   // scnt[4], swi[4], sthr, probe cache follow (qscan_kernel)
    static_assert(M % 4 == 0 && M <= 64, "four sub-quantizer groups per parked point; 64 * 255 < 2^15");
    static_assert(DS % 2 == 0, "8-byte rows of the f32 codewords / centroid slices at least");
    static_assert(M + DS <= 120, "scan test: (m + dsub + 4) u <= 2^-17");
    static_assert(PG >= 1 && PG <= 4, "one MFMA column per probe");
};
// LDS of qscan_kernel<M, DS, PG, true, true>: LbCfg's regions, then the four-wave tail.  (size_t)-1: there is no such kernel
constexpr size_t lb_lds_bytes(int m, int dsub, int pg)
{
#define X(M_, D_, P_) if (m == M_ && dsub == D_ && pg == P_) return fw_tail(LbCfg<M_, D_, P_>::END, P_).end;
    IVF_LB_SHAPES(X)
#undef X
    return ~(size_t)0;
}

constexpr size_t LDS_MAX = 160 << 10;
// the eight-wave list-major kernel (wg8scan.hip.h) as the plan's own choice on long lists (ivfadc_set_table_mode(h, 6) asks for it anywhere)
constexpr double W8_Q8_MIN_PPL = 8.0;   // probes per list from which the eight-query form of the eight-wave kernel is planned
// sub-space widths the eight-wave kernel is instantiated for (m = 8: d = 32, 64, 96, 128), and the instantiation of a form and a width
inline bool w8_dsub(int dsub) { return w8_ds_ok(dsub); }
// ... and m = 16 (d = 64, 128: wg8_m16_scan_kernel<NQ, DS>, K <= 64, no wide pool), which runs on request only -- table modes 6 / 7 (8 / 9):
// not timed against the four-wave kernel yet
inline bool w8_m16_dsub(int dsub) { return dsub == 4 || dsub == 8; }
// the wide-pool form (two pool entries per lane: 64 < K <= 128; table modes 8 / 9)
constexpr int W8_WIDE_MAX_K = 128;

// selector capacity of the scan (K) and of the stand-alone top-w (w): registers up to 64, LDS buffers beyond
inline int sel_cap(int k) { return k <= 64 ? 64 : (pow2ceil(k + 64) > 128 ? pow2ceil(k + 64) : 128); }

}  // namespace ivf
