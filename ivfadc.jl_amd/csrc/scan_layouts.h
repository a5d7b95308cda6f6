// scan_layouts.h -- what the search plan (plan.h) has to know about the scan kernels: their dynamic-LDS layouts and sizes, the shapes
// they are instantiated for, the limits their index arithmetic sets.  Plain C++ (no HIP type), so the plan compiles and runs without
// a GPU (tests/c/plan_check.cpp); the kernel headers include this file and read the very same names, namespace ivf:
//   wg8scan.hip.h   W8_*, W8Lds, w8_ds_ok           nfscan.hip.h    NF_*, NfLds
//   u16scan.hip.h   U16_*, u16_*_lds_bytes          lbscan.hip.h    LbCfg (lb_lds_bytes restates its END: asserted in ivfadc_hip.hip)
//   kernels.hip.h   carve_lds (scan_lds_bytes restates it: see there)
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

// ---- the query-major kernel's matrix-core rounds (lbscan.hip.h, qscan_body<..., LB = true>) ------------------------------------------
// shapes the matrix-core lower-bound rounds (qscan_kernel<..., LB = true>) are instantiated for
inline bool lb_shape(int m, int dsub) { return (m == 48 && dsub == 16) || (m == 16 && dsub == 6); }

// LbCfg<M, DS, PG>::END + the tail of qscan_body's carve (scnt, swi, sthr, probe cache): ivfadc_hip.hip asserts the equality for every
// instantiated (M, DS, PG), next to pick_qscan_lb
constexpr size_t lb_lds_bytes(int m, int dsub, int pg)
{
    size_t b = align_up((size_t)pg * ((size_t)m * 256 + 32), 16);
    b += (size_t)m * pg * ((dsub + 3) & ~3) * 4;   // f32 residuals of the round's probes (rows padded to 16-byte groups)
    b += 2 * (size_t)m * pg * 4 + 128 + 256;   // norms, bases, per-probe constants of the round and of the query
    b += (size_t)m * dsub * 4;              // query
    b += (size_t)4 * (pg >= 4 ? 54 : 16) * (m / 4 + 2) * 4;   // parking pools (LbCfg::PCAP entries per wave)
    b += 4 * 64 * 8;                        // upper-bound keys of the four waves
    b += (size_t)4 * pg * 4 + 16 + (size_t)pg * 40 + 3 * 256;
    return b;
}

// ---- the four-wave kernels (kernels.hip.h: scan_kernel, qscan_kernel, sq_kernel) -----------------------------------------------------
// shapes the striped list-major kernels exist for (IVF_SHAPES with m = 8 / 16)
inline bool filt_shape(int m, int dsub) { return (m == 8 && dsub == 16) || (m == 16 && (dsub == 6 || dsub == 8)); }

// the shape the narrow-field list-major kernel exists for (nfscan.hip.h)
inline bool nf_shape(int m, int dsub) { return m == 8 && dsub == 16; }

// restates carve_lds() in kernels.hip.h and what its callers carve behind it (a comment ties the two: carve_lds hands out pointers at run
// time and names no end, so there is no constant to assert against without editing it).  stripe: the plan's (Plan::stripe), for the width qg
constexpr size_t scan_lds_bytes(int m, int d, int qg, int cap, bool small, bool list_major = false, bool stripe = false)
{
    size_t b = (size_t)(m > 2 ? m : 2) * 256 * qg * 4;
    b += align_up((size_t)d * qg, 4) * 4;
    if (!small) b += (size_t)4 * (list_major ? qg : 1) * cap * 8;   // LDS selectors: per wave and query (query-major: one query)
    b += (size_t)4 * qg * 4 + 16;
    b = align_up(b, 8) + (size_t)qg * 40;  // workgroup-shared thresholds + the four waves' quarter keys per slot (STHR_WORDS)
    b += 3 * 256;                           // query-major kernel: LDS copy of the query's probes (see qscan_kernel)
    if (list_major && qg == 4 && (m == 8 || m == 16))
        b += 4 * 16 * 5 * 4;                // groups of four at m = 8 / 16 (striped or not): 4 waves x CAND_CAP parked points x <= 5 dwords
    if (stripe && m == 8)
        b += 256 * 64;                      // m = 8 striped: the 16-bit integer filter table behind the float tables (QF_BYTES)
    return b;
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
