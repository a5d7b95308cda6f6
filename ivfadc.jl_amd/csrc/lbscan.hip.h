// lbscan.hip.h -- query-major rounds with ADC tables built on the matrix cores (included by kernels.hip.h, namespace ivf).
//
// Reference: src/index.jl:232-236 (table build), :240-246 (scan).  The reference's table entry
//     T[ii][c] = sum_t (CB_ii[t,c] - r[ii*dsub + t])^2          (f32, t ascending, one rounding per operation)
// costs 3 vector-ALU operations per (codeword, dimension) and re-reads the whole codebook per probe: on the HD shape
// (m = 48, dsub = 16: 768 KB of codewords, 590 k lane-operations per probe) that build, not the code stream, is what
// the query-major kernel spends its time on.  Nothing in the SELECTION needs those entries exactly --
// only the sums of the few points that can still reach the top-K do.  So:
//
//   1. FILTER TABLES on the matrix cores.  With E = ||cb - r||^2 = ||cb||^2 - 2 cb.r + ||r||^2 (real arithmetic on the
//      given f32 operands), a probe's table is a 256 x dsub by dsub x PG product per sub-quantizer:
//      v_mfma_f32_4x4x4_16b_bf16 (16 independent 4 x 4 x 4 blocks per wave: lane l = codeword 64 g + l as the A row,
//      probe l mod 4 as the B column), operands split into two bf16 pieces each (x = hi + lo + O(2^-18 |x|); hi.hi +
//      lo.hi + hi.lo), the -2 and the quantisation scale folded into the residual operand and ||cb||^2, ||r||^2, the
//      error margin and the base folded into the accumulator's initial value.  (The same build on v_mfma_f32_4x4x1_16b_f32
//      -- no splits, 16 instead of 12 matrix instructions per 64 codewords -- is bit-for-bit as valid and measured 3 % slower.)
//      What leaves the accumulator is
//          v <= (E - base) * inv            (proof below)
//      and q = rne(v - 0.5), saturated to [0, 255] by v_cvt_pk_u8_f32, is an 8-BIT LOWER BOUND: base + q / inv <= E.
//      A probe's table is m x 256 BYTES (12 KB instead of 48 KB), so a round carries PG = 4 probes and the codebook
//      is read once per four probes instead of once per probe.
//   2. SCAN with integer sums: one SDWA address op + ds_read_u8 + half a v_add3_u32 per lookup; integer addition is
//      associative, and a 256-byte table has two dwords per LDS bank, so a gather is at most 2-way conflicted.  A
//      point survives iff sum_i q_i <= Tg, where Tg is derived from the current bound such that every point whose
//      REFERENCE sum is <= the bound survives (no false negatives; proof below).
//   3. SURVIVORS are parked -- code bytes, visit order, integer sum, probe slot -- in a per-wave pool and evaluated LAZILY.
//      The integer sums bound the distances from above as well (lb_scan_step), so a second selector over UPPER bounds
//      tightens the bound without a single exact sum; a full pool is compacted against the bound of the moment (most of
//      what was parked under an older, looser bound drops out) and only then, or at the end of the round, are entries
//      worked off 16 at a time: the four lanes of a quad recompute the reference's table entries of sub-quantizers
//      4 i .. 4 i + 3 from the f32 codebook (sub, mul, add; t ascending) and the running sum -- the coarse distance,
//      then the entries in ascending order (index.jl:242-246) -- walks along the quad.  Only these sums meet the result
//      selectors: ids and distances are bit-identical to the exact kernels.
//
// Error budget of step 1, in units of inv * N with N = ||cb||^2 + ||r||^2 (note 2 |cb.r| <= N), u = 2^-24:
//   norms in f32 (||cb||^2 rounded from double, ||r||^2 a 16-term float sum)            <= 17 u
//   r'' = fl(-2 inv r)                                                                   <=  1 u
//   splits: |x - hi - lo| <= 2^-18 |x| for cb and r'', dropped lo.lo <= 2^-18            <=  3 * 2^-18
//   f32 accumulation: 3 dsub/4 chained MFMAs (12 for dsub = 16), each within 2^-22 of the magnitudes it adds
//   (partial sums <= 2 inv N)                                                            <=  2^-17.4
//   accumulator seed (two fmas)                                                          <=  2 u
//   total < 2^-15.7; the seed subtracts 2^-14 inv N, so v <= (E - base) inv holds with a 3x margin (mu of lb_scan_step:
//   2^-14 + 2^-15.7 < 2^-13.4).
// Scan test.  T_ii >= E_ii (1 - (dsub + 2) u) (rounded differences, squares and dsub adds), the reference sum
// S >= (dc + sum T)(1 - (m + 1) u), hence dc + sum E <= S (1 + 2^-17) for m + dsub <= 120.  With S <= thr:
//   sum q_i <= sum (E_i - base_i) inv <= (thr (1 + 2^-17) - dc - sum base) inv
// and Tg = floor(fl(((thr (1 + 2^-16) - dc) - sbase) * inv) * (1 + 2^-20)) + 2 covers the float evaluation (the extra
// 2^-17 thr dominates the <= 52 u thr of rounding in sbase and the two subtractions).
// base_ii = max(0, ||r_ii|| - max_c ||cb_c||)^2 (1 - 2^-10) <= E for every codeword; inv = 254 / max_ii range_ii with
// range_ii = (||r_ii|| + max_c ||cb_c||)^2 (1 + 2^-10) - base_ii.  Any scale keeps the bound valid (q saturates).
#pragma once

struct LbView {
    const uint4 *cb_split;   // [m][4][NP][64] 16-byte parts: bf16 hi / lo halves of the codewords in LABEL order (see lb_build_tables)
    const float *cb_n2;      // [m][256] ||codeword||^2 by label (rounded from double)
    const float *cb_lab;     // [m][256][dsub] f32 codewords by label: exact sums of the survivors
    const float *cb_maxn;    // [m] >= max_c ||codeword c||
    // round 5: the one-product f16 form of the build (lb_build_tables_f16); null: the three-product bf16 split above
    const uint4 *cb_f16;     // [m][4][DSP / 8][64] 16-byte parts: the codewords as f16 of (codeword x 2^e_ii), LABEL order
    const float *cb_isc;     // [m] 2^-e_ii
    float mu;                // slack of the upper bounds E <= base + (q + 1) / inv + mu N: 2^-13.4 (split) / 2^-9.4 (f16 codewords)
};

// LbCfg<M, DS, PG>, the rounds' LDS layout: scan_layouts.h

// (byte BI of dw) + add in one VALU instruction
template <int BI> static __device__ __forceinline__ u32 sdwa_byte_add(u32 dw, u32 add)
{
    u32 o;
    if constexpr (BI == 0) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD" : "=v"(o) : "v"(dw), "v"(add));
    else if constexpr (BI == 1) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(o) : "v"(dw), "v"(add));
    else if constexpr (BI == 2) asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(o) : "v"(dw), "v"(add));
    else asm("v_add_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(o) : "v"(dw), "v"(add));
    return o;
}

// ---- step 1: the PG lower-bound tables of a round, on the matrix cores -----------------------------------------------------
// Wave wv takes sub-quantizers wv, wv + 4, ...; a unit = (sub-quantizer ii, group g of 64 labels): lane l holds label
// 64 g + l as the A row of block l / 4 (NP 16-byte loads, each 1 KB per wave-instruction: cb_split is stored
// [ii][g][part][lane]), probe l mod 4 as the B column (bf16 pieces of r'' = -2 inv r, from the f32 residuals in LDS), and receives the entries of labels
// 64 g + 4 (l / 4) + {0..3} for probe l mod 4: four bytes = one ds_write_b32 into that probe's table.
typedef short lb_s4 __attribute__((ext_vector_type(4)));
typedef __bf16 lb_bf2 __attribute__((ext_vector_type(2)));
// (x0, x1) -> bf16 pieces: hi = rne(x) (v_cvt_pk_bf16_f32), lo = rne(x - hi); x - hi is exact in f32
static __device__ __forceinline__ void lb_split2(float x0, float x1, u32 &hi, u32 &lo)
{
    const v2f x = (v2f){x0, x1};
    const lb_bf2 h = __builtin_convertvector(x, lb_bf2);
    __builtin_memcpy(&hi, &h, 4);
    const v2f hf = (v2f){__uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u)};
    const lb_bf2 l = __builtin_convertvector(x - hf, lb_bf2);
    __builtin_memcpy(&lo, &l, 4);
}

template <int M, int DS, int PG>
static __device__ __forceinline__ void lb_build_tables(const LbView &lb, unsigned char *smem, int wv, int lane)
{
    using C = LbCfg<M, DS, PG>;
    constexpr int NP = C::NP, NCH = C::NCH;
    constexpr int NBUF = (PG >= 4 || M % 3 != 0) ? 4 : 3;   // units in flight (register budget: PG = 4 runs two workgroups per CU, PG = 3 three)
    static_assert(M % 4 == 0 && M % NBUF == 0, "every wave takes M / 4 sub-quantizers = M units: no tail, compile-time trip counts");
    const int j = lane & 3, jj = j < PG ? j : 0;
    const float rmax = __uint_as_float(((const u32 *)(smem + C::PC_OFF))[8 + jj]);
    const float inv = rmax > 1e-30f ? 254.0f / rmax : 0.0f;
    const float invm = inv * 0.99993896484375f;   // 1 - 2^-14: the error margin, proportional to ||cb||^2 + ||r||^2
    const float m2inv = -2.0f * inv;
    constexpr int nun = M;                        // units of this wave: M / 4 sub-quantizers x 4 label groups
    uint4 A[NBUF][NP];
    float4 N2[NBUF];
    auto load_unit = [&](int u, int b) __attribute__((always_inline)) {
        const int ii = wv + 4 * (u >> 2), g = u & 3;
        const uint4 *src = lb.cb_split + ((size_t)(ii * 4 + g) * NP) * 64 + lane;
#pragma unroll
        for (int p = 0; p < NP; ++p) A[b][p] = src[(size_t)p * 64];
        N2[b] = *(const float4 *)(lb.cb_n2 + (size_t)ii * 256 + g * 64 + (lane >> 2) * 4);
    };
#pragma unroll
    for (int b = 0; b < NBUF - 1; ++b)
        if (b < nun) load_unit(b, b);
    u32 Bh[NCH * 2], Bl[NCH * 2];                // bf16 pairs of r'' = -2 inv r: chunk kc = dwords 2 kc, 2 kc + 1
    float cst = 0.0f;
#pragma unroll 1
    for (int u0 = 0; u0 < nun; u0 += NBUF) {
#pragma unroll
        for (int b = 0; b < NBUF; ++b) {
            const int u = u0 + b;
            if (u < nun) {   // uniform
                if (u + NBUF - 1 < nun) load_unit(u + NBUF - 1, (b + NBUF - 1) % NBUF);
                const int ii = wv + 4 * (u >> 2), g = u & 3;
                if (g == 0) {
                    const float4 *rr = (const float4 *)(smem + C::R_OFF + ((u32)jj * (M * C::DSR) + (u32)ii * C::DSR) * 4u);
#pragma unroll
                    for (int t4 = 0; t4 < NCH; ++t4) {
                        float4 r4 = (float4){0.f, 0.f, 0.f, 0.f};
                        if (t4 * 4 < C::DSR) r4 = rr[t4];
                        lb_split2(m2inv * r4.x, m2inv * r4.y, Bh[2 * t4], Bl[2 * t4]);
                        lb_split2(m2inv * r4.z, m2inv * r4.w, Bh[2 * t4 + 1], Bl[2 * t4 + 1]);
                    }
                    const float r2 = ((const float *)(smem + C::CST_OFF))[ii * PG + jj];
                    const float base = ((const float *)(smem + C::BS_OFF))[ii * PG + jj];
                    cst = __builtin_fmaf(r2, invm, __builtin_fmaf(-base, inv, -0.5f));
                }
                v4f acc = (v4f){__builtin_fmaf(N2[b].x, invm, cst), __builtin_fmaf(N2[b].y, invm, cst), __builtin_fmaf(N2[b].z, invm, cst),
                                __builtin_fmaf(N2[b].w, invm, cst)};
#pragma unroll
                for (int kc = 0; kc < NCH; ++kc) {
                    const uint4 ah4 = A[b][kc >> 1], al4 = A[b][NP / 2 + (kc >> 1)];
                    const uint2 ah = (kc & 1) ? make_uint2(ah4.z, ah4.w) : make_uint2(ah4.x, ah4.y);
                    const uint2 al = (kc & 1) ? make_uint2(al4.z, al4.w) : make_uint2(al4.x, al4.y);
                    const uint2 bh = make_uint2(Bh[2 * kc], Bh[2 * kc + 1]);
                    const uint2 bl = make_uint2(Bl[2 * kc], Bl[2 * kc + 1]);
                    lb_s4 vah, val, vbh, vbl;
                    __builtin_memcpy(&vah, &ah, 8); __builtin_memcpy(&val, &al, 8);
                    __builtin_memcpy(&vbh, &bh, 8); __builtin_memcpy(&vbl, &bl, 8);
                    acc = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(vah, vbh, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(val, vbh, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(vah, vbl, acc, 0, 0, 0);
                }
                u32 pk = 0;
                pk = __builtin_amdgcn_cvt_pk_u8_f32(acc.x, 0, pk);
                pk = __builtin_amdgcn_cvt_pk_u8_f32(acc.y, 1, pk);
                pk = __builtin_amdgcn_cvt_pk_u8_f32(acc.z, 2, pk);
                pk = __builtin_amdgcn_cvt_pk_u8_f32(acc.w, 3, pk);
                if (j < PG) *(u32 *)(smem + (u32)j * C::TS + (u32)ii * 256u + (u32)g * 64u + (u32)(lane >> 2) * 4u) = pk;
            }
        }
    }
}

// ---- step 1, round 5: the same tables from f16 codewords --------------------------------------------------------------------------
// The codebook's trip through L1 / L2 is what the build waits for, and the bf16 split carries 4 bytes per codeword
// element -- as many as the f32 codebook.  f16 carries 11 significant bits in 2: the codewords are stored ONCE as f16 of (codeword x
// 2^e_ii) (per sub-quantizer, max |cb 2^e| in [2^10, 2^11], set at index creation), |cb^ - cb| <= 2^-11 |cb|; the residual, which is made
// in registers, is scaled by 2^(9 - floor(log2 ||r_ii||^2 / 2)) (so |r_t| 2^.. < 2^10) and split into TWO f16 pieces (hi + lo + O(2^-22)),
// so it costs nothing in accuracy.  Products of two f16 are exact in f32, the accumulation is f32:  |cb^ . r - cb . r| <= 2^-11 |cb||r|
// (+ 2^-21), i.e. at most 2^-11 N in E = ||cb||^2 - 2 cb.r + ||r||^2 (2 |cb||r| <= N = ||cb||^2 + ||r||^2).  With the unchanged small
// terms of the header (norms 17 u, r'' 1 u, accumulation 2^-17.4, seed 2 u) the total stays below 2^-10.9 inv N; the seed subtracts
// 2^-10 inv N, so v <= (E - base) inv holds as before, and the upper bounds of lb_scan_step take mu = 2^-10 + 2^-10.9 < 2^-9.4.
// Two v_mfma_f32_4x4x4_16b_f16 per k-chunk instead of three bf16 ones, HALF the codeword bytes; the price is a bound looser by up to
// a quarter of a table unit per entry (254 x 2^-10) -- and where a probe's residual dwarfs its codewords the round falls back to the
// split (lb_prepare_round).
typedef _Float16 lb_h4 __attribute__((ext_vector_type(4)));
typedef _Float16 lb_h2 __attribute__((ext_vector_type(2)));

template <int M, int DS, int PG>
static __device__ __forceinline__ void lb_build_tables_f16(const LbView &lb, unsigned char *smem, int wv, int lane)
{
    using C = LbCfg<M, DS, PG>;
    constexpr int NPH = C::DSP / 8, NCH = C::NCH;
    constexpr int NBUF = (PG >= 4 || M % 3 != 0) ? 4 : 3;
    static_assert(M % 4 == 0 && M % NBUF == 0, "every wave takes M / 4 sub-quantizers = M units: no tail, compile-time trip counts");
    const int j = lane & 3, jj = j < PG ? j : 0;
    const float rmax = __uint_as_float(((const u32 *)(smem + C::PC_OFF))[8 + jj]);
    const float inv = rmax > 1e-30f ? 254.0f / rmax : 0.0f;
    const float invm = inv * 0.9990234375f;       // 1 - 2^-10: the error margin, proportional to ||cb||^2 + ||r||^2
    const float m2inv = -2.0f * inv;
    constexpr int nun = M;
    uint4 A[NBUF][NPH];
    float4 N2[NBUF];
    auto load_unit = [&](int u, int b) __attribute__((always_inline)) {
        const int ii = wv + 4 * (u >> 2), g = u & 3;
        const uint4 *src = lb.cb_f16 + ((size_t)(ii * 4 + g) * NPH) * 64 + lane;
#pragma unroll
        for (int p = 0; p < NPH; ++p) A[b][p] = src[(size_t)p * 64];
        N2[b] = *(const float4 *)(lb.cb_n2 + (size_t)ii * 256 + g * 64 + (lane >> 2) * 4);
    };
#pragma unroll
    for (int b = 0; b < NBUF - 1; ++b)
        if (b < nun) load_unit(b, b);
    u32 Bf[NCH * 2], Bg[NCH * 2];                // f16 pairs of r 2^(9 - hx), hi and lo pieces: chunk kc = dwords 2 kc, 2 kc + 1
    float cst = 0.0f, ksc = 0.0f;
#pragma unroll 1
    for (int u0 = 0; u0 < nun; u0 += NBUF) {
#pragma unroll
        for (int b = 0; b < NBUF; ++b) {
            const int u = u0 + b;
            if (u < nun) {   // uniform
                if (u + NBUF - 1 < nun) load_unit(u + NBUF - 1, (b + NBUF - 1) % NBUF);
                const int ii = wv + 4 * (u >> 2), g = u & 3;
                if (g == 0) {
                    const float r2 = ((const float *)(smem + C::CST_OFF))[ii * PG + jj];
                    const float base = ((const float *)(smem + C::BS_OFF))[ii * PG + jj];
                    // ||r|| < 2^(hx + 1) with hx = floor(exponent(r2) / 2): every |r_t| 2^(9 - hx) < 2^10
                    const int hx = ((int)((__float_as_uint(r2) >> 23) & 255u) - 127) >> 1;
                    const float scr = __uint_as_float((u32)(127 + 9 - hx) << 23);
                    ksc = m2inv * lb.cb_isc[ii] * __uint_as_float((u32)(127 - 9 + hx) << 23);
                    const float4 *rr = (const float4 *)(smem + C::R_OFF + ((u32)jj * (M * C::DSR) + (u32)ii * C::DSR) * 4u);
#pragma unroll
                    for (int t4 = 0; t4 < NCH; ++t4) {
                        float4 r4 = (float4){0.f, 0.f, 0.f, 0.f};
                        if (t4 * 4 < C::DSR) r4 = rr[t4];
                        // the residual is made in registers, so it can afford two pieces (x = hi + lo + O(2^-22 |x|)): only the codewords,
                        // which come from memory, are rounded to 11 bits
                        const v2f xa = (v2f){r4.x * scr, r4.y * scr}, xb = (v2f){r4.z * scr, r4.w * scr};
                        const lb_h2 ha = __builtin_convertvector(xa, lb_h2), hb = __builtin_convertvector(xb, lb_h2);   // v_cvt_f16_f32: round to nearest even
                        const lb_h2 la = __builtin_convertvector(xa - __builtin_convertvector(ha, v2f), lb_h2);
                        const lb_h2 lc = __builtin_convertvector(xb - __builtin_convertvector(hb, v2f), lb_h2);
                        __builtin_memcpy(&Bf[2 * t4], &ha, 4);
                        __builtin_memcpy(&Bf[2 * t4 + 1], &hb, 4);
                        __builtin_memcpy(&Bg[2 * t4], &la, 4);
                        __builtin_memcpy(&Bg[2 * t4 + 1], &lc, 4);
                    }
                    cst = __builtin_fmaf(r2, invm, __builtin_fmaf(-base, inv, -0.5f));
                }
                v4f acc = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kc = 0; kc < NCH; ++kc) {
                    const uint4 a4 = A[b][kc >> 1];
                    const uint2 a2 = (kc & 1) ? make_uint2(a4.z, a4.w) : make_uint2(a4.x, a4.y);
                    const uint2 b2 = make_uint2(Bf[2 * kc], Bf[2 * kc + 1]), g2 = make_uint2(Bg[2 * kc], Bg[2 * kc + 1]);
                    lb_h4 va, vb, vg;
                    __builtin_memcpy(&va, &a2, 8);
                    __builtin_memcpy(&vb, &b2, 8);
                    __builtin_memcpy(&vg, &g2, 8);
                    acc = __builtin_amdgcn_mfma_f32_4x4x4f16(va, vg, acc, 0, 0, 0);   // small terms first
                    acc = __builtin_amdgcn_mfma_f32_4x4x4f16(va, vb, acc, 0, 0, 0);
                }
                const float v0 = __builtin_fmaf(ksc, acc.x, __builtin_fmaf(N2[b].x, invm, cst)), v1 = __builtin_fmaf(ksc, acc.y, __builtin_fmaf(N2[b].y, invm, cst));
                const float v2 = __builtin_fmaf(ksc, acc.z, __builtin_fmaf(N2[b].z, invm, cst)), v3 = __builtin_fmaf(ksc, acc.w, __builtin_fmaf(N2[b].w, invm, cst));
                u32 pk = 0;
                pk = __builtin_amdgcn_cvt_pk_u8_f32(v0, 0, pk);
                pk = __builtin_amdgcn_cvt_pk_u8_f32(v1, 1, pk);
                pk = __builtin_amdgcn_cvt_pk_u8_f32(v2, 2, pk);
                pk = __builtin_amdgcn_cvt_pk_u8_f32(v3, 3, pk);
                if (j < PG) *(u32 *)(smem + (u32)j * C::TS + (u32)ii * 256u + (u32)g * 64u + (u32)(lane >> 2) * 4u) = pk;
            }
        }
    }
}

// ---- step 3: reference-order sums of parked points (index.jl:232-246), 16 per pass ------------------------------------
// Lane 4 e + part: entry e, sub-quantizers part, part + 4, part + 8, ...  In trip i the four lanes of a quad hold the
// reference's table entries of sub-quantizers 4 i .. 4 i + 3 (r_t = q_t - c_t, df = cb_t - r_t, sum = sum + df * df for t
// ascending), and the running sum -- dc, then the entries in ascending sub-quantizer order (index.jl:242-246) -- walks along the
// quad by DPP row_shr:1 adds: after step p lane `part == p` holds the sum through sub-quantizer 4 i + p; the quad's last
// lane hands it back to all four for the next trip.
// DS floats from a row that is 16-byte aligned when DS % 4 == 0, 8-byte aligned otherwise (DS even)
template <int DS> static __device__ __forceinline__ void lb_load_row(const float *p, float (&o)[DS])
{
    if constexpr (DS % 4 == 0) {
#pragma unroll
        for (int t = 0; t < DS; t += 4) {
            const float4 v = *(const float4 *)(p + t);
            o[t] = v.x; o[t + 1] = v.y; o[t + 2] = v.z; o[t + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int t = 0; t < DS; t += 2) {
            const float2 v = *(const float2 *)(p + t);
            o[t] = v.x; o[t + 1] = v.y;
        }
    }
}

template <int M, int DS, int G>
static __device__ __forceinline__ void lb_drain(const u32 *pbuf, int cnt, const LbView &lb, const float *centroids, const float *qf, const int *s_list,
                                                const float *s_dc, WSel<true> &sel, u32 &thr_hi, int K, int lane, u64 *sthr)   // entries pbuf[0 .. cnt), cnt <= 16
{
    constexpr int ES = M / 4 + 2, NI = M / 4;
    static_assert(NI % G == 0, "G trips per load group: G codewords and centroid slices (4 DS bytes each) in flight per lane");
    const int e = lane >> 2, part = lane & 3;
    const bool ok = e < cnt;
    const u32 *ent = pbuf + (ok ? e : 0) * ES;
    const u32 seq = ent[M / 4];
    const int slot = (int)(ent[M / 4 + 1] & 0xffu);               // probe of the query
    float run = s_dc[slot];
    const float *crow = centroids + (size_t)s_list[slot] * (M * DS) + part * DS;
    const float *qrow = qf + part * DS;
    float x = 0.0f;
#pragma unroll 1
    for (int i0 = 0; i0 < NI; i0 += G) {
        float cwv[G][DS], ccv[G][DS];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const u32 byte = (ent[i0 + g] >> (8 * part)) & 0xffu;               // code byte of sub-quantizer 4 (i0 + g) + part
            lb_load_row<DS>(lb.cb_lab + ((size_t)(4 * (i0 + g) + part) * 256 + byte) * DS, cwv[g]);
            lb_load_row<DS>(crow + (size_t)(i0 + g) * 4 * DS, ccv[g]);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float qv[DS];
            lb_load_row<DS>(qrow + (size_t)(i0 + g) * 4 * DS, qv);
            float T = 0.0f;
#pragma unroll
            for (int t = 0; t < DS; ++t) {
                // r = q - c (coarsequantizers.jl:40-45); df = cb - r, T += df * df for t ascending (index.jl:234, colwise SqEuclidean)
                const float r = qv[t] - ccv[g][t];
                const float df = cwv[g][t] - r;
                T = T + df * df;
            }
            x = run + T;                              // lane `part == 0`: the sum through sub-quantizer 4 i
#pragma unroll
            for (int p = 1; p < 4; ++p) {             // row_shr:1: lane l reads lane l - 1 (same row of 16: quads never straddle rows)
                const float up = __uint_as_float((u32)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), 0x111, 0xf, 0xf, false));
                x = up + T;
            }
            run = __uint_as_float((u32)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), 0xFF, 0xf, 0xf, false));   // quad_perm:[3,3,3,3]
        }
    }
    sel.tighten(readfirstlane64(sthr[0]));
    const u64 key = make_key(x, seq);
    sel.push(ok && part == 3 && key < sel.thr(), key, K, lane);
    if (lane == 0 && (u32)(sel.thr() >> 32) < thr_hi) atomicMin(&sthr[0], sel.thr());
    thr_hi = (u32)(sel.thr() >> 32);
}

// integer target of a bound (high word of the K-th best key so far) for one probe: see the header
static __device__ __forceinline__ int lb_target(u32 thr_hi, float dc, float sbase, float inv)
{
    if (thr_hi >= 0x7F800000u) return 0x7FFF;
    const float thr = __uint_as_float(thr_hi);
    const float x = ((thr * 1.0000152587890625f - dc) - sbase) * inv * 1.00000095367431640625f;   // (1 + 2^-16), (1 + 2^-20)
    return x < 0.0f ? -1 : (x < 32000.0f ? (int)x + 2 : 0x7FFF);
}

// One step of a wave: the STEP points whose codes sit in `cr` (positions pb.. of a list of p1 points), table of their probe at
// LDS byte toff.  pbuf / ccnt: this wave's parking buffer and its fill.
// The pool of one wave is full: drop the entries that the bound of the moment rules out (the filter's own test, per probe of the
// query: pp = inv[32], sbase[32]); if every entry stays, work 16 off.  Entry e belongs to lane e.
template <int M, int DS, int G, int PCAP>
static __device__ __forceinline__ void lb_pool_make_room(u32 *pbuf, int &pcnt, const LbView &lb, const float *centroids, const float *qf,
                                                         const int *s_list, const float *s_dc, const float *pp, WSel<true> &sel, u32 &thr_hi, int K,
                                                         int lane, u64 *sthr, u32 &nsurv, bool flush = false)
{
    constexpr int ES = M / 4 + 2;
    static_assert(PCAP <= 64, "one pool entry per lane");
    wave_sync();
    sel.tighten(readfirstlane64(sthr[0]));
    thr_hi = (u32)(sel.thr() >> 32);
    u32 ew[ES];
    const bool have = lane < pcnt;
#pragma unroll
    for (int k = 0; k < ES; ++k) ew[k] = have ? pbuf[lane * ES + k] : 0u;
    const int slot = (int)(ew[ES - 1] & 0xffu);
    const int tg = lb_target(thr_hi, s_dc[slot], pp[32 + slot], pp[slot]);
    const u64 keep = __builtin_amdgcn_ballot_w64(have && (int)(ew[ES - 1] >> 8) <= tg);
    const int nk = __popcll(keep);
    if (nk < pcnt) {
        wave_sync();   // every entry is in registers before one is overwritten
        if ((keep >> lane) & 1ull) {
            u32 *dst = pbuf + __popcll(keep & ((1ull << lane) - 1ull)) * ES;
#pragma unroll
            for (int k = 0; k < ES; ++k) dst[k] = ew[k];
        }
        pcnt = nk;
        wave_sync();
    }
    while (pcnt > 0 && (flush || pcnt == PCAP)) {   // uniform
        const int take = pcnt < 16 ? pcnt : 16;
        nsurv += (u32)take;
        lb_drain<M, DS, G>(pbuf + (pcnt - take) * ES, take, lb, centroids, qf, s_list, s_dc, sel, thr_hi, K, lane, sthr);
        pcnt -= take;
        if (!flush) break;
    }
    wave_sync();
}

template <int M, int DS, int PPL, int G, int PCAP>
static __device__ __forceinline__ void lb_scan_step(const CodeRegs<M, PPL> &cr, u32 toff, u32 pb, u32 p1, u32 seq0, int slot, float dc, float sbase,
                                                    float inv, float nn, int &Tg, u32 &thr_hi, u32 *pbuf, int &pcnt, const LbView &lb,
                                                    const float *centroids, const float *qf, const int *s_list, const float *s_dc, const float *pp,
                                                    WSel<true> &sel, WSel<true> &usel, int K, int lane, u64 *sthr, u32 &nsurv)
{
    using CR = CodeRegs<M, PPL>;
    constexpr int ES = M / 4 + 2;
    u32 pw[PPL][M / 4], acc[PPL];
    static_for<PPL>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        cr.words(r, pw[r]);
        acc[r] = 0u;
    });
    // lookups in groups of GT sub-quantizers, two groups in flight: with two waves per SIMD the LDS pipe only stays busy if every
    // wave keeps ~12 reads outstanding (the counter holds 15); the sums of group g are taken while group g + 1 is on its way
    constexpr int GT = M % 3 == 0 ? 3 : 2, NG = M / GT;
    static_assert(M % GT == 0, "whole groups");
    u32 v[2][GT * PPL];
    auto issue = [&](auto gc, u32 (&dst)[GT * PPL]) __attribute__((always_inline)) {
        constexpr int g = decltype(gc)::value;
        static_for<GT>([&](auto kc) {
            constexpr int t = g * GT + decltype(kc)::value;
            static_for<PPL>([&](auto rc) {
                constexpr int r = decltype(rc)::value;
                const u32 ea = sdwa_byte_add<(t & 3)>(pw[r][t >> 2], toff);
                dst[decltype(kc)::value * PPL + r] = (u32)lds_load_abs<unsigned char>(ea + (u32)t * 256u);
            });
        });
    };
    issue(IntC<0>{}, v[0]);
    static_for<NG>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        if constexpr (g + 1 < NG) issue(IntC<g + 1>{}, v[(g + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < GT; ++k)
#pragma unroll
            for (int r = 0; r < PPL; ++r) acc[r] += v[g & 1][k * PPL + r];
        __builtin_amdgcn_sched_barrier(0);
    });
    u64 cm[PPL];
    int n = 0;
#pragma unroll
    for (int r = 0; r < PPL; ++r) {
        cm[r] = __builtin_amdgcn_ballot_w64((int)acc[r] <= Tg && CR::point(pb, r, lane) < p1);
        n += __popcll(cm[r]);
    }
    if (n == 0) return;
    // Upper bounds.  q = rne(v) >= v - 0.5 and no entry saturates at 255 (the scale comes from a rigorous range), so
    // E_i <= base_i + (q_i + 1) / inv + mu N_i with mu < 2^-13.4 (margin + error budget of the header); with T_i <= E_i (1 + (dsub + 2) u)
    // and (m + 1) roundings of the reference sum, a point with integer sum Q has S <= (dc + sbase + (Q + M) / inv + mu NN)(1 + 2^-16) =: ub.
    // The K-th smallest ub over the candidates seen so far is a bound that K real points meet -- an upper bound of the final
    // K-th key -- found without an exact sum.  Only candidates are offered: a point below the K-th ub has Q <= Tg.
    if (inv > 0.0f) {
        const float c0 = dc + sbase, c1 = 1.0000002f / inv, c2 = nn * lb.mu;   // mu: 9.2e-5 (bf16 split) / 1.48e-3 (f16 codewords)
#pragma unroll
        for (int r = 0; r < PPL; ++r) {
            const float ub = ((c0 + (float)(acc[r] + (u32)M) * c1) + c2) * 1.0000153f;
            const u64 key = make_key(ub, seq0 + CR::point(pb, r, lane));
            usel.push(((cm[r] >> lane) & 1ull) != 0 && key < usel.thr(), key, K, lane);
        }
        const u64 ut = usel.thr();
        if ((u32)(ut >> 32) < 0x7F800000u) {   // K upper bounds stand
            sel.tighten(ut | 0xFFFFFFFFull);
            if ((u32)(sel.thr() >> 32) < thr_hi) {
                if (lane == 0) atomicMin(&sthr[0], sel.thr());
                thr_hi = (u32)(sel.thr() >> 32);
                Tg = lb_target(thr_hi, dc, sbase, inv);
                n = 0;
#pragma unroll
                for (int r = 0; r < PPL; ++r) {
                    cm[r] &= __builtin_amdgcn_ballot_w64((int)acc[r] <= Tg);
                    n += __popcll(cm[r]);
                }
            }
        }
    }
    // park what is left; a full pool is compacted against the bound of the moment first, and only if that frees nothing are 16
    // entries worked off
#pragma unroll
    for (int r = 0; r < PPL; ++r) {
        u64 m = cm[r];
        while (m) {   // uniform
            if (pcnt == PCAP) {
                lb_pool_make_room<M, DS, G, PCAP>(pbuf, pcnt, lb, centroids, qf, s_list, s_dc, pp, sel, thr_hi, K, lane, sthr, nsurv);
                Tg = lb_target(thr_hi, dc, sbase, inv);
                m &= __builtin_amdgcn_ballot_w64((int)acc[r] <= Tg);
                continue;
            }
            const int room = PCAP - pcnt;
            u64 tk = m;
            while (__popcll(tk) > room) tk &= ~(1ull << (63 - __builtin_clzll(tk)));
            if ((tk >> lane) & 1ull) {
                u32 *ent = pbuf + (pcnt + __popcll(tk & ((1ull << lane) - 1ull))) * ES;
#pragma unroll
                for (int k = 0; k < M / 4; ++k) ent[k] = pw[r][k];
                ent[M / 4] = seq0 + CR::point(pb, r, lane);
                ent[M / 4 + 1] = (acc[r] << 8) | (u32)slot;
            }
            pcnt += __popcll(tk);
            m &= ~tk;
        }
    }
}

// ---- residuals, norms, scales and the PG tables of one round: probes j0 .. j0 + PG - 1 of the query (s_list: its probed cells, LDS) ----
// Every thread of the workgroup calls it (barriers (B), (C), (D) inside); qf: the query in LDS.  Leaves the tables at LDS byte 0,
// the f32 residuals at R_OFF and the per-probe constants at PC_OFF (inv, sbase, nn) and PP_OFF (per probe of the query).
template <int M, int DS, int PG>
static __device__ __forceinline__ void lb_prepare_round(const IndexView &ix, const LbView &lb, unsigned char *smem, const float *qf,
                                                        const int *s_list, int j0, int w, int wv, int lane, int tid)
{
    using C = LbCfg<M, DS, PG>;
    constexpr int D = M * DS;
    float *cst = (float *)(smem + C::CST_OFF), *bs = (float *)(smem + C::BS_OFF), *pc = (float *)(smem + C::PC_OFF);
    u32 *pcu = (u32 *)pc;
    float *rres = (float *)(smem + C::R_OFF), *pp = (float *)(smem + C::PP_OFF);
        // (1) residuals of the round's probes, f32 (coarsequantizers.jl:40-45), rows padded with zeros to whole 16-byte groups
#pragma unroll
        for (int s = 0; s < PG; ++s) {
            const int pj = (j0 + s) < w ? j0 + s : j0;
            const float *crow = ix.centroids + (size_t)s_list[pj] * D;
            if constexpr (DS % 4 == 0) {
                for (int i = tid * 4; i < D; i += 1024) {
                    const float4 c4 = *(const float4 *)(crow + i), q4 = *(const float4 *)(qf + i);
                    *(float4 *)(rres + s * D + i) = (float4){q4.x - c4.x, q4.y - c4.y, q4.z - c4.z, q4.w - c4.w};
                }
            } else {
                for (int e = tid; e < M * C::DSR; e += 256) {
                    const int ii = e / C::DSR, t = e - ii * C::DSR;
                    rres[s * (M * C::DSR) + e] = t < DS ? qf[ii * DS + t] - crow[ii * DS + t] : 0.0f;
                }
            }
        }
        __syncthreads();   // (B)
        // (2) per (sub-quantizer, probe): ||r||^2, base, range
        for (int e = tid; e < M * PG; e += 256) {
            const int ii = e / PG, s = e - ii * PG;
            const float4 *rr = (const float4 *)(rres + s * (M * C::DSR) + ii * C::DSR);
            float r2 = 0.0f;
#pragma unroll
            for (int t4 = 0; t4 < C::DSR / 4; ++t4) {
                const float4 r4 = rr[t4];
                r2 = __builtin_fmaf(r4.x, r4.x, r2); r2 = __builtin_fmaf(r4.y, r4.y, r2);
                r2 = __builtin_fmaf(r4.z, r4.z, r2); r2 = __builtin_fmaf(r4.w, r4.w, r2);
            }
            const float nr = __builtin_sqrtf(r2), cm = lb.cb_maxn[ii];
            // ||r|| - max ||cb|| from below and ||r|| + max ||cb|| from above: the norms carry a few ulp, the margins 2^-10
            const float lo0 = nr * 0.9990234375f - cm * 1.0009765625f;
            const float lo = lo0 > 0.0f ? lo0 : 0.0f;
            const float hi = (nr + cm) * 1.0009765625f;
            const float base = lo * lo, range = hi * hi - base;
            cst[e] = r2;
            bs[e] = base;
            atomicMax(&pcu[8 + s], __float_as_uint(range));                       // range >= +0: the bit pattern orders like the value
            atomicAdd(&pc[20 + s], r2 + cm * cm);                                 // sum over sub-quantizers of N: which build the round takes
        }
        __syncthreads();   // (C)
        if (wv < PG) {     // what the scan needs of this: scale and sum of bases of probe wv (read behind barrier (D))
            float sb = lane < M ? bs[lane * PG + wv] : 0.0f;
            float cmx = lane < M ? lb.cb_maxn[lane] : 0.0f;
            float nv = lane < M ? cst[lane * PG + wv] + cmx * cmx : 0.0f;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {   // a fixed order: the same value in every lane
                sb = sb + __shfl_xor(sb, off);
                nv = nv + __shfl_xor(nv, off);
            }
            if (lane == 0) {
                const float rmax = __uint_as_float(pcu[8 + wv]);
                const float iv = rmax > 1e-30f ? 254.0f / rmax : 0.0f;
                pc[wv] = iv;
                pc[4 + wv] = sb;
                if (j0 + wv < w) { pp[j0 + wv] = iv; pp[32 + j0 + wv] = sb; }
                pc[16 + wv] = nv * 1.00001f;
            }
        }
        // Which build.  The f16 form's margin is 2^-10 inv N per entry; where a probe's residual dwarfs its codewords (N >> range: a query
        // far from every cell) that is many table units and the filter would go blind, while the split's 2^-14 keeps it sharp.  So the
        // round takes the f16 form only if its AVERAGE margin stays within one table unit for every probe of the round (the sums of N were
        // accumulated in step (2); every wave reads the same LDS words; either build is a valid lower bound, so even a split decision
        // would be exact).
        bool use16 = lb.cb_f16 != nullptr;
        if (use16) {
            float worst = 0.0f;
#pragma unroll
            for (int s = 0; s < PG; ++s) {
                const float rmax = __uint_as_float(pcu[8 + s]);
                worst = fmaxf(worst, rmax > 1e-30f ? pc[20 + s] * (254.0f / rmax) : 0.0f);
            }
            use16 = worst * 0.0009765625f <= (float)M;   // 2^-10 inv sum_ii N_ii <= M table units
        }
        if (use16) lb_build_tables_f16<M, DS, PG>(lb, smem, wv, lane);   // uniform
        else lb_build_tables<M, DS, PG>(lb, smem, wv, lane);
        __syncthreads();   // (D)
}

// The four waves' upper-bound selectors each see a quarter of the points: the K-th smallest upper bound of their UNION is the bound
// worth having (K-th of ~N points instead of K-th of N / 4).  store: a wave's keys -> LDS (own slice; no reader before the next
// barrier); merge (behind that barrier, every wave for itself): K smallest of the union.  Wave 0 carries the union on, the others
// restart empty under its K-th key, so no key is ever held twice.
static __device__ __forceinline__ void lb_ub_store(const WSel<true> &usel, u64 *ubx, int *ubc, int K, int wv, int lane)
{
    const int c = usel.finish(K, lane);
    usel.store(ubx + wv * 64, c, lane);
    if (lane == 0) ubc[wv] = c;
}
static __device__ __forceinline__ void lb_ub_merge(WSel<true> &usel, WSel<true> &sel, const u64 *ubx, const int *ubc, int K, int wv, int lane,
                                                   u64 *sthr, u32 &thr_hi)
{
    WSel<true> mg;
    mg.init(KEY_MAX, nullptr, 64, K);
    if (4 * K <= 64) {
        const int v = lane / K, i = lane - v * K;
        const bool pred = lane < 4 * K && i < ubc[v];
        const u64 key = pred ? ubx[v * 64 + i] : KEY_MAX;
        mg.seed_from_block(pred, key, K, lane);
    } else {
        for (int ow = 0; ow < 4; ++ow) sel_absorb(mg, ubx + ow * 64, ubc[ow], K, lane);
    }
    const u64 kth = readlane64(mg.top, K - 1);   // KEY_MAX while the union holds fewer than K keys
    if (wv == 0) usel = mg;
    else usel.init(kth, nullptr, 64, K);
    if ((u32)(kth >> 32) < 0x7F800000u) {
        sel.tighten(kth | 0xFFFFFFFFull);
        if (lane == 0 && (u32)(sel.thr() >> 32) < thr_hi) atomicMin(&sthr[0], sel.thr());
        thr_hi = (u32)(sel.thr() >> 32);
    }
}

// ---- the rounds of one query (called by qscan_kernel<M, DS, PG, true, LB = true> after its top-w prologue) ------------------
// s_list / s_dc / s_base / s_len / s_coff: the LDS copy of the query's probes (w <= 32).  sel: this wave's selector; sthr: the
// workgroup-shared bound.  Four barriers per round: (A) the previous round's scans are over; (B) the f32 residuals stand;
// (C) norms, bases and range maxima stand; (D) the tables stand.
template <int M, int DS, int PG>
static __device__ __forceinline__ void lb_rounds(const IndexView &ix, const LbView &lb, const float *queries, unsigned char *smem, int q, int w, int K,
                                                 int prune, u64 *scanned_points, WSel<true> &sel, u64 *sthr, const int *s_list, const float *s_dc,
                                                 const u32 *s_base, const u32 *s_len, const u32 *s_coff, int wv, int lane, int tid)
{
    using C = LbCfg<M, DS, PG>;
    constexpr int D = M * DS;
    constexpr int PPL = PG >= 4 ? 2 : 1;          // points per lane and step, codeword groups of a drain: register budget, as NBUF
    constexpr int DG = 1;                         // (a drain inside the scan is rare now; the final flush below keeps three groups in flight)
    using CR = CodeRegs<M, PPL>;
    constexpr u32 STEP = CR::STEP;
    float *cst = (float *)(smem + C::CST_OFF), *bs = (float *)(smem + C::BS_OFF), *pc = (float *)(smem + C::PC_OFF);
    u32 *pcu = (u32 *)pc;
    float *rres = (float *)(smem + C::R_OFF), *pp = (float *)(smem + C::PP_OFF), *qf = (float *)(smem + C::LQ_OFF);
    for (int i = tid; i < D; i += 256) qf[i] = queries[(size_t)q * D + i];
    u32 *pbuf = (u32 *)(smem + C::PARK_OFF) + (size_t)wv * C::PCAP * C::ES;
    WSel<true> usel;   // K smallest UPPER bounds this wave has seen (lb_scan_step)
    usel.init(KEY_MAX, nullptr, 64, K);
    u64 *ubx = (u64 *)(smem + C::UB_OFF);
    int *ubc = (int *)(smem + C::PC_OFF) + 24;   // [4] key counts (words 24..27 of the per-probe block)
    if (tid < PG) { pcu[8 + tid] = 0u; pcu[20 + tid] = 0u; }
    int ccnt = 0;
    u32 nsurv = 0;
    u32 thr_hi = 0xFFFFFFFFu;
    for (int j0 = 0; j0 < w; j0 += PG) {
        if (j0 > 0) lb_ub_store(usel, ubx, ubc, K, wv, lane);
        __syncthreads();   // (A)
        if (j0 > 0) lb_ub_merge(usel, sel, ubx, ubc, K, wv, lane, sthr, thr_hi);
        // exact pruning, as in the exact rounds: nothing writes the shared bound between barrier (A) and the next scan
        const u32 thi = (u32)(readfirstlane64(sthr[0]) >> 32);
        if (prune == 1 && __float_as_uint(s_dc[j0]) > thi) {
            if (tid == 0) {
                u64 skipped = 0;
                for (int pj = j0; pj < w; ++pj) skipped += s_len[pj];
                atomicAdd(scanned_points + (size_t)(q & 63) * 8 + 1, skipped);
            }
            break;
        }
        // prune == 2 (probes in the caller's order, ivfadc_search_preassigned): a list above the bound ends nothing -- every probe of a
        // round is judged alone, the first like the others below, and the rounds with nothing left to scan are stepped over right here
        // (uniform: LDS words and the shared bound), before any table is built
        if (prune == 2) {
            for (; j0 < w; j0 += PG) {
                bool none = true;
                for (int s = 0; s < PG && (j0 + s) < w; ++s) none = none && (s_len[j0 + s] == 0 || __float_as_uint(s_dc[j0 + s]) > thi);
                if (!none) break;
                if (tid < PG && (j0 + tid) < w && s_len[j0 + tid] != 0) atomicAdd(scanned_points + (size_t)(q & 63) * 8 + 1, (u64)s_len[j0 + tid]);
            }
            if (j0 >= w) {
                __syncthreads();   // the flush below stores the waves' upper-bound keys again: every wave is done reading them first
                break;
            }
        }
        if (tid < PG) {
            const int s = tid;
            u32 len = (j0 + s) < w ? s_len[j0 + s] : 0u;
            if (prune && (s > 0 || prune == 2) && len != 0 && __float_as_uint(s_dc[(j0 + s) < w ? j0 + s : j0]) > thi) {
                atomicAdd(scanned_points + (size_t)(q & 63) * 8 + 1, (u64)len);
                len = 0;
            }
            pcu[12 + s] = len;
        }
        lb_prepare_round<M, DS, PG>(ix, lb, smem, qf, s_list, j0, w, wv, lane, tid);   // barriers (B), (C), (D) inside
        if (tid < PG) { pcu[8 + tid] = 0u; pcu[20 + tid] = 0u; }   // range maxima (and sums of N) of the next round (every reader of this round's is behind barrier (D))
        // scan: the four waves interleave the steps of each list; a wave's next step (of this or the next list) is in flight
        __builtin_amdgcn_s_setprio(3);
        int s = 0;
        u32 pb = wv * STEP;
        auto norm = [&](int &ss, u32 &pp) __attribute__((always_inline)) {
            while (ss < PG && pp >= pcu[12 + ss]) { ++ss; pp = wv * STEP; }
        };
        norm(s, pb);
        CR cr;
        if (s < PG) cr.load(ix.codes + ((size_t)s_coff[j0 + s] << 8), pb, lane);
        int cur = -1, Tg = 0x7FFF;
        float dc = 0.f, sbase = 0.f, inv = 0.f, nn = 0.f;
        u32 p1 = 0, seq0 = 0;
        while (s < PG) {   // uniform
            int s2 = s;
            u32 pb2 = pb + 4 * STEP;
            norm(s2, pb2);
            CR nx;
            if (s2 < PG) nx.load(ix.codes + ((size_t)s_coff[j0 + s2] << 8), pb2, lane);
            else nx = cr;
            const bool fresh = s != cur;
            if (fresh) {
                cur = s;
                dc = s_dc[j0 + s]; sbase = pc[4 + s]; inv = pc[s]; nn = pc[16 + s];
                p1 = pcu[12 + s]; seq0 = s_base[j0 + s];
            }
            sel.tighten(readfirstlane64(sthr[0]));
            const u32 th = (u32)(sel.thr() >> 32);
            if (fresh || th != thr_hi) {
                thr_hi = th;
                Tg = lb_target(thr_hi, dc, sbase, inv);
            }
            if (!(prune && __float_as_uint(dc) > thr_hi))   // per wave, exact: no point of this list can beat the bound any more
                lb_scan_step<M, DS, PPL, DG, C::PCAP>(cr, (u32)s * C::TS, pb, p1, seq0, j0 + s, dc, sbase, inv, nn, Tg, thr_hi, pbuf, ccnt, lb,
                                                      ix.centroids, qf, s_list, s_dc, pp, sel, usel, K, lane, sthr, nsurv);
            cr = nx; s = s2; pb = pb2;
        }
        __builtin_amdgcn_s_setprio(0);
    }
    {   // what is still viable under the final bound gets its exact sum (the pool outlives the rounds: most of it never does)
        lb_ub_store(usel, ubx, ubc, K, wv, lane);
        __syncthreads();
        lb_ub_merge(usel, sel, ubx, ubc, K, wv, lane, sthr, thr_hi);
        if (ccnt > 0)
            lb_pool_make_room<M, DS, (M / 4) % 3 == 0 ? 3 : ((M / 4) % 2 == 0 ? 2 : 1), C::PCAP>(pbuf, ccnt, lb, ix.centroids, qf, s_list, s_dc, pp, sel, thr_hi, K, lane, sthr, nsurv, true);
    }
    if (lane == 0 && nsurv) atomicAdd(scanned_points + (size_t)(q & 63) * 8 + 2, (u64)nsurv);
}

// ---- test hook (ivfadc_debug_lb_table): the lower-bound table of ONE (query, cell) pair, built by the production code path ----
// out_tab: M x 256 bytes (table slot = label); out_f: inv, sbase, nn, then base[M], then ||r_ii||^2[M]
template <int M, int DS>
__global__ __launch_bounds__(256) void lb_debug_kernel(const IndexView ix, const LbView lb, const float *query, int list, unsigned char *out_tab,
                                                       float *out_f)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using C = LbCfg<M, DS, 1>;
    constexpr int D = M * DS;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float *qf = (float *)(smem_raw + C::LQ_OFF);
    int *s_list = (int *)(smem_raw + C::END);
    u32 *pcu = (u32 *)(smem_raw + C::PC_OFF);
    for (int i = tid; i < D; i += 256) qf[i] = query[i];
    if (tid == 0) { s_list[0] = list; pcu[8] = 0u; pcu[20] = 0u; }
    __syncthreads();
    lb_prepare_round<M, DS, 1>(ix, lb, smem_raw, qf, s_list, 0, 1, wv, lane, tid);
    for (int i = tid; i < M * 256; i += 256) out_tab[i] = smem_raw[i];
    const float *pc = (const float *)(smem_raw + C::PC_OFF), *bs = (const float *)(smem_raw + C::BS_OFF), *cst = (const float *)(smem_raw + C::CST_OFF);
    if (tid == 0) { out_f[0] = pc[0]; out_f[1] = pc[4]; out_f[2] = pc[16]; }
    if (tid < M) { out_f[3 + tid] = bs[tid]; out_f[3 + M + tid] = cst[tid]; }
}

// ---- measurement hook (ivfadc_set_profiling(h, 2)): the table build of a batch ALONE, same code and same LDS footprint as in the
// search kernel (so the same two workgroups per CU), one workgroup per query over the probes the search used.  sink keeps the result live.
template <int M, int DS, int PG>
__global__ __launch_bounds__(256, M <= 16 ? 3 : (PG >= 4 ? 2 : (PG == 3 ? 3 : 4))) void lb_build_only_kernel(const IndexView ix, const LbView lb, const float *queries,
                                                                                               const int *probe_list, int w, u32 *sink)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    using C = LbCfg<M, DS, PG>;
    constexpr int D = M * DS;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = blockIdx.x;
    float *qf = (float *)(smem_raw + C::LQ_OFF);
    int *s_list = (int *)(smem_raw + C::END);
    u32 *pcu = (u32 *)(smem_raw + C::PC_OFF);
    for (int i = tid; i < D; i += 256) qf[i] = queries[(size_t)q * D + i];
    if (tid < w && tid < 32) s_list[tid] = probe_list[(size_t)q * w + tid];
    if (tid < PG) { pcu[8 + tid] = 0u; pcu[20 + tid] = 0u; }
    u32 acc = 0;
    for (int j0 = 0; j0 < w; j0 += PG) {
        __syncthreads();
        lb_prepare_round<M, DS, PG>(ix, lb, smem_raw, qf, s_list, j0, w, wv, lane, tid);
        if (tid < PG) { pcu[8 + tid] = 0u; pcu[20 + tid] = 0u; }
        acc += ((const u32 *)smem_raw)[tid];
    }
    if (acc == 0xDEADBEEFu) sink[q] = acc;
}
