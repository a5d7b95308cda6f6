// Host-side packers of ivfadc_create: every device operand that is derived from the caller's centroids, codebooks and labels, one
// function per operand family.  Plain C++ (no HIP): each takes the caller's arrays and returns std::vectors, so the layouts can be
// compiled and run without a GPU.  The arithmetic is part of the kernels' error bounds: sums in double rounded once, the (1.0 + 1e-6)
// factors, power-of-two scales through std::ldexp.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace pack {

inline uint16_t to_bf16(float x)   // round to nearest even
{
    uint32_t b;
    memcpy(&b, &x, 4);
    return (uint16_t)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);
}

// x = hi + lo + O(2^-18 |x|)
inline void split_bf16(float v, uint16_t &hi, uint16_t &lo)
{
    hi = to_bf16(v);
    const uint32_t hb32 = (uint32_t)hi << 16;
    float hf;
    memcpy(&hf, &hb32, 4);
    lo = to_bf16(v - hf);
}

inline uint16_t f16_bits(float x)
{
    const _Float16 v = (_Float16)x;
    uint16_t b;
    memcpy(&b, &v, 2);
    return b;
}

// regrouped codebooks for the table build (IndexView::codebooks_t): [m][dp / 4][ksub][4], dp = dsub rounded up to 4, zero-padded.
// pair_packed (build_tables_t, DSUB == 6, even m, 8-bit handles): [m / 2][3][ksub][4], element e = 0..11 of pair p, codeword c =
// dimension e of sub-quantizer 2p (e < 6) or dimension e - 6 of sub-quantizer 2p + 1
inline std::vector<float> codebooks_t(const float *codebooks, int m, int ksub, int dsub, bool pair_packed)
{
    const int dp = (dsub + 3) & ~3;
    std::vector<float> t((size_t)m * dp * ksub, 0.0f);
    if (pair_packed) {
        for (int p = 0; p < m / 2; ++p)
            for (int c = 0; c < ksub; ++c)
                for (int e = 0; e < 12; ++e) {
                    const int ii = 2 * p + e / 6, x = e % 6;
                    t[(size_t)p * 12 * ksub + ((size_t)(e / 4) * ksub + c) * 4 + (e % 4)] = codebooks[((size_t)ii * ksub + c) * dsub + x];
                }
        return t;
    }
    for (int ii = 0; ii < m; ++ii)
        for (int c = 0; c < ksub; ++c)
            for (int x = 0; x < dsub; ++x)
                t[(size_t)ii * dp * ksub + ((size_t)(x / 4) * ksub + c) * 4 + (x % 4)] = codebooks[((size_t)ii * ksub + c) * dsub + x];
    return t;
}

// pair-interleaved codebooks for the packed-FP32 table build of the m = 48 query-major kernel (IndexView::codebooks_p)
inline std::vector<float> codebooks_p(const float *codebooks, int m, int ksub, int dsub)
{
    std::vector<float> pp((size_t)m * dsub * ksub);
    for (int p = 0; p < m / 2; ++p)
        for (int c = 0; c < ksub; ++c)
            for (int x = 0; x < dsub; ++x)
                for (int hh = 0; hh < 2; ++hh)
                    pp[(size_t)p * dsub * 2 * ksub + ((size_t)(x / 2) * ksub + c) * 4 + (x % 2) * 2 + hh] =
                        codebooks[((size_t)(2 * p + hh) * ksub + c) * dsub + x];
    return pp;
}

// the f32 codewords in LABEL order (table slot = code byte), [m][256][dsub]; f(ii, c, label, ||codeword||^2 summed in double) is
// called once per codeword
template <class F>
std::vector<float> label_order_codewords(const float *codebooks, const uint8_t *labels, int m, int ksub, int dsub, F f)
{
    std::vector<float> lab((size_t)m * 256 * dsub, 0.0f);
    for (int ii = 0; ii < m; ++ii)
        for (int c = 0; c < ksub; ++c) {
            const int L = labels[(size_t)ii * ksub + c];
            const float *cw = codebooks + ((size_t)ii * ksub + c) * dsub;
            double acc = 0.0;
            for (int t = 0; t < dsub; ++t) {
                acc += (double)cw[t] * cw[t];
                lab[((size_t)ii * 256 + L) * dsub + t] = cw[t];
            }
            f(ii, c, L, acc);
        }
    return lab;
}

// operands of the lower-bound table build (lbscan.hip.h; ksub = 256), everything in LABEL order:
// split[ii][g][p][lane] = 8 bf16 of label 64 g + lane -- parts p < NP / 2: hi pieces of dimensions 8 p .. 8 p + 7, the others the lo
// pieces; n2 = ||codeword||^2 rounded once; maxn >= max ||codeword|| per sub-quantizer;
// f16[ii][g][p][lane] = 8 f16 of label 64 g + lane, dimensions 8 p .. 8 p + 7, scaled by 2^e_ii with max |cb 2^e_ii| in [2^10, 2^11],
// isc = 2^-e_ii (the one-product build)
struct LbOperands {
    std::vector<uint16_t> split, f16;
    std::vector<float> n2, lab, maxn, isc;
};
inline LbOperands lb_operands(const float *codebooks, const uint8_t *labels, int m, int ksub, int dsub)
{
    const int dsp = (dsub + 7) & ~7, np = dsp / 4, nph = dsp / 8;
    LbOperands o;
    o.n2.assign((size_t)m * 256, 0.0f);
    std::vector<double> mxn((size_t)m, 0.0);
    o.lab = label_order_codewords(codebooks, labels, m, ksub, dsub, [&](int ii, int, int L, double acc) {
        o.n2[(size_t)ii * 256 + L] = (float)acc;
        mxn[ii] = std::max(mxn[ii], acc);
    });
    o.maxn.resize((size_t)m);
    for (int ii = 0; ii < m; ++ii) o.maxn[ii] = (float)(std::sqrt(mxn[ii]) * (1.0 + 1e-6));
    o.split.assign((size_t)m * 4 * np * 64 * 8, 0);
    o.f16.assign((size_t)m * 4 * nph * 64 * 8, 0);
    o.isc.assign((size_t)m, 1.0f);
    for (int ii = 0; ii < m; ++ii) {
        const float *cbi = codebooks + (size_t)ii * ksub * dsub;
        double mxa = 0.0;
        for (int i = 0; i < ksub * dsub; ++i) mxa = std::max(mxa, (double)std::fabs(cbi[i]));
        int ex = 0;
        if (mxa > 0.0) ex = std::max(-100, std::min(100, (int)std::floor(std::log2(2048.0 / mxa))));
        const float sc = std::ldexp(1.0f, ex);
        o.isc[ii] = std::ldexp(1.0f, -ex);
        for (int c = 0; c < ksub; ++c) {
            const int L = labels[(size_t)ii * ksub + c], g = L >> 6, ln = L & 63;
            const size_t base = (((size_t)(ii * 4 + g) * np) * 64) * 8;
            for (int t = 0; t < dsub; ++t) {
                const float v = cbi[(size_t)c * dsub + t];
                uint16_t hi, lo;
                split_bf16(v, hi, lo);
                o.split[base + ((size_t)(t >> 3) * 64 + ln) * 8 + (t & 7)] = hi;
                o.split[base + ((size_t)(np / 2 + (t >> 3)) * 64 + ln) * 8 + (t & 7)] = lo;
                o.f16[((((size_t)(ii * 4 + g) * nph) + (t >> 3)) * 64 + ln) * 8 + (t & 7)] = f16_bits(v * sc);
            }
        }
    }
    return o;
}

// operands of the narrow-field list-major kernel (nfscan.hip.h; ksub = 256): n2[m][256] = ||codeword||^2 by CODEWORD index (rounded
// once) for the filter tables, then max ||codeword||^2 per block; lab = the f32 codewords in LABEL order for the exact sums of what the
// filter lets through
struct NfOperands {
    std::vector<float> n2, lab;
};
inline NfOperands nf_operands(const float *codebooks, const uint8_t *labels, int m, int ksub, int dsub)
{
    NfOperands o;
    o.n2.assign((size_t)m * 256 + m, 0.0f);
    o.lab = label_order_codewords(codebooks, labels, m, ksub, dsub, [&](int ii, int c, int, double acc) {
        o.n2[(size_t)ii * 256 + c] = (float)acc;
        o.n2[(size_t)m * 256 + ii] = std::max(o.n2[(size_t)m * 256 + ii], (float)(acc * (1.0 + 1e-6)));
    });
    return o;
}

// inverse labels of an 8-bit handle (recon_decode_kernel, reconstruct.hip.h): [m][256], slot = the label byte a stored code holds,
// value = the index of the codeword it names; a byte that is no label of its block maps to 0 (no stored code holds one)
inline std::vector<uint8_t> label_inverse(const uint8_t *labels, int m, int ksub)
{
    std::vector<uint8_t> inv((size_t)m * 256, 0);
    for (int ii = 0; ii < m; ++ii)
        for (int c = 0; c < ksub; ++c) inv[(size_t)ii * 256 + labels[(size_t)ii * ksub + c]] = (uint8_t)c;
    return inv;
}

// ||c||^2 in double, rounded once: error <= u ||c||^2 (see refine_probes); cmaxn >= max ||centroid||
struct CentroidNorms {
    std::vector<float> n2;
    float cmaxn;
};
inline CentroidNorms centroid_norms(const float *centroids, int d, int kc)
{
    CentroidNorms o;
    o.n2.resize((size_t)kc);
    double mx = 0.0;
    for (int c = 0; c < kc; ++c) {
        double acc = 0.0;
        for (int i = 0; i < d; ++i) acc += (double)centroids[(size_t)c * d + i] * centroids[(size_t)c * d + i];
        o.n2[c] = (float)acc;
        mx = std::max(mx, acc);
    }
    o.cmaxn = (float)(std::sqrt(mx) * (1.0 + 1e-6));
    return o;
}

// regrouped centroids for the latency path's coarse search (smallq.hip.h): [d / 4][kc][4] (d % 4 == 0)
inline std::vector<float> cent_t(const float *centroids, int d, int kc)
{
    std::vector<float> ct((size_t)d * kc);
    for (int c = 0; c < kc; ++c)
        for (int i = 0; i < d; ++i) ct[((size_t)(i >> 2) * kc + c) * 4 + (i & 3)] = centroids[(size_t)c * d + i];
    return ct;
}

// bf16 split of the centroids for coarse_bf16_kernel, rows zero-padded to dp dimensions
struct CentroidBf16 {
    std::vector<uint16_t> hi, lo;
};
inline CentroidBf16 centroid_bf16(const float *centroids, int d, int kc, int dp)
{
    CentroidBf16 o;
    o.hi.assign((size_t)kc * dp, 0);
    o.lo.assign((size_t)kc * dp, 0);
    for (int c = 0; c < kc; ++c)
        for (int i = 0; i < d; ++i) split_bf16(centroids[(size_t)c * d + i], o.hi[(size_t)c * dp + i], o.lo[(size_t)c * dp + i]);
    return o;
}

// the f16 form of the same rows: one power-of-two scale for the whole quantizer (and for the queries, which live in the same space),
// 2^11 <= scale * max |component| <= 2^12.  scale == 0 and no rows: the form does not exist (all-zero centroids, a scale out of range)
struct CentroidF16 {
    std::vector<uint16_t> rows;
    float scale = 0.f;
};
inline CentroidF16 centroid_f16(const float *centroids, int d, int kc, int dp)
{
    CentroidF16 o;
    double maxabs = 0.0;
    for (size_t i = 0; i < (size_t)kc * d; ++i) maxabs = std::max(maxabs, (double)std::fabs(centroids[i]));
    if (!(maxabs > 0.0 && std::isfinite(maxabs))) return o;
    const int ex = (int)std::floor(std::log2(4096.0 / maxabs));
    if (!(ex > -100 && ex < 100)) return o;
    o.scale = std::ldexp(1.0f, ex);
    o.rows.assign((size_t)kc * dp, 0);
    for (int c = 0; c < kc; ++c)
        for (int i = 0; i < d; ++i) o.rows[(size_t)c * dp + i] = f16_bits(centroids[(size_t)c * d + i] * o.scale);
    return o;
}

}  // namespace pack
