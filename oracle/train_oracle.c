/*
 * train_oracle.c -- CPU restatement of the project's own trainer (ivfadc_train).
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under ivfadc.jl_amd/ (the product) may
 * include, link, load or call this file.  Unlike ivfadc_oracle.c, which restates
 * the reference's search, this file restates the algorithm of
 * ivfadc.jl_amd/csrc/train.hip.h driven by kmeans_dev / train_impl
 * (ivfadc.jl_amd/csrc/ivfadc_hip.hip), operation for operation, so that the
 * device result can be pinned bit for bit:
 *
 *   sample        S = min(n, max(32768, 32k)); sample s is point (s * n) / S
 *   tr_hash       mix64(a + 0x9E3779B97F4A7C15 (b+1) + 0xD1B54A32D192ED03 (c+1)), u64 wrap-around
 *   k-means++     first pick tr_hash(seed,0,0) % S; then Float32 sequential distances to the newest
 *                 centre, running minimum, per-256 block sums in double in the kernel's tree order
 *                 (off = 128 ... 1), the D^2 pick walk of tr_kmpp_pick_kernel
 *   assignment    Float32 sequential distances over the window's columns, first minimum on ties
 *                 (coarse_dist_kernel + argmin_rows_kernel)
 *   update        llrint(x * scale) summed in int64 (order-independent), mean
 *                 (float)((double)acc * inv_scale / count); an empty cluster restarts from point
 *                 tr_hash(seed, iter + 7777, c) % n; stop when no centre changes bits
 *   scale         2^(61 - e) with n * max|x| < 2^e exactly (frexp): every fixed-point sum stays
 *                 below 2^61 + n/2 < 2^62, and the quantum 1/scale follows the data's magnitude
 *   PQ stage      final coarse assignment, residuals x - c in Float32, sub-space i trained with seed
 *                 seed + 1 + i on the n x dsub window at column i * dsub, leading dimension d
 *
 * OpenMP only parallelises over points / samples whose results do not depend on one another;
 * every sum keeps its one order.  Build with -ffp-contract=off and without -ffast-math.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ORA_OK 0
#define ORA_ERR_ASSERT 1
#define ORA_ERR_NOMEM 2
#define ORA_ERR_INVALID 3

uint64_t ora_mix64(uint64_t x);   /* ivfadc_oracle.c */

static uint64_t tr_hash(uint64_t a, uint64_t b, uint64_t c)
{
    return ora_mix64(a + 0x9E3779B97F4A7C15ull * (b + 1) + 0xD1B54A32D192ED03ull * (c + 1));
}

/* Float32 squared distance, columns in ascending order, one rounding per operation */
static float sqdist(const float *a, const float *b, int dcols)
{
    float acc = 0.0f;
    for (int i = 0; i < dcols; ++i) {
        const float t = a[i] - b[i];
        acc = acc + t * t;
    }
    return acc;
}

/* nearest centre of every point of the n x dcols window (leading dimension ld); ties -> lowest index */
static void assign_all(const float *x, int64_t n, int dcols, int ld, const float *centres, int k, int32_t *assign)
{
#pragma omp parallel for schedule(static)
    for (int64_t p = 0; p < n; ++p) {
        const float *row = x + p * ld;
        float best = sqdist(row, centres, dcols);
        int bi = 0;
        for (int c = 1; c < k; ++c) {
            const float v = sqdist(row, centres + (size_t)c * dcols, dcols);
            if (v < best) { best = v; bi = c; }
        }
        assign[p] = bi;
    }
}

/* fixed-point scale of kmeans_dev: n * maxabs < 2^e, scale = 2^(61 - e) (all-zero data: e = 0) */
static double fixed_point_scale(const float *x, int64_t n, int dcols, int ld)
{
    float maxabs = 0.0f;
    for (int64_t p = 0; p < n; ++p)
        for (int i = 0; i < dcols; ++i) maxabs = fmaxf(maxabs, fabsf(x[p * ld + i]));
    int e = 0;
    frexp((double)n * (double)maxabs, &e);
    return ldexp(1.0, 61 - e);
}

/* kmeans_dev: k-means of the n x dcols window of x (leading dimension ld) into centres [k][dcols] */
static int kmeans(const float *x, int64_t n, int dcols, int ld, int k, int maxiter, uint64_t seed, float *centres,
                  int32_t *out_iters, int32_t *out_converged)
{
    const int64_t want = 32 * (int64_t)k > 32768 ? 32 * (int64_t)k : 32768;
    const int S = (int)(n < want ? n : want);
    const int nblk = (S + 255) / 256;
    float *mind = (float *)malloc(sizeof(float) * (size_t)S);
    double *partial = (double *)malloc(sizeof(double) * (size_t)nblk);
    int32_t *assign = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
    int64_t *acc = (int64_t *)malloc(sizeof(int64_t) * (size_t)k * dcols);
    uint32_t *counts = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)k);
    if (!mind || !partial || !assign || !acc || !counts) {
        free(mind); free(partial); free(assign); free(acc); free(counts);
        return ORA_ERR_NOMEM;
    }

    /* ---- k-means++ over the strided subsample (tr_kmpp_update_kernel / tr_kmpp_pick_kernel) */
    for (int j = 0; j < k; ++j) {
        if (j > 0) {
            const float *centre = centres + (size_t)(j - 1) * dcols;
            const int first = j == 1;
#pragma omp parallel for schedule(static)
            for (int s = 0; s < S; ++s) {
                const int64_t p = ((int64_t)s * n) / S;
                const float a = sqdist(x + p * ld, centre, dcols);
                mind[s] = first ? a : fminf(mind[s], a);
            }
#pragma omp parallel for schedule(static)
            for (int b = 0; b < nblk; ++b) {
                double sm[256];
                for (int t = 0; t < 256; ++t) sm[t] = b * 256 + t < S ? (double)mind[b * 256 + t] : 0.0;
                for (int off = 128; off > 0; off >>= 1)
                    for (int t = 0; t < off; ++t) sm[t] += sm[t + off];
                partial[b] = sm[0];
            }
        }
        int s;
        if (j == 0) {
            s = (int)(tr_hash(seed, 0, 0) % (uint64_t)S);
        } else {
            double total = 0.0;
            for (int b = 0; b < nblk; ++b) total += partial[b];
            const double u = (double)(tr_hash(seed, (uint64_t)j, 1) >> 11) * (1.0 / 9007199254740992.0);
            if (total <= 0.0) {
                s = (int)(tr_hash(seed, (uint64_t)j, 2) % (uint64_t)S);
            } else {
                const double r = u * total;
                double run = 0.0;
                int b = 0;
                while (b < nblk - 1 && run + partial[b] <= r) { run += partial[b]; ++b; }
                s = b * 256;
                const int hi = S < b * 256 + 256 ? S : b * 256 + 256;
                while (s < hi - 1 && run + (double)mind[s] <= r) { run += (double)mind[s]; ++s; }
            }
        }
        const int64_t p = ((int64_t)s * n) / S;
        memcpy(centres + (size_t)j * dcols, x + p * ld, sizeof(float) * (size_t)dcols);
    }

    /* ---- Lloyd (coarse_dist_kernel + argmin_rows_kernel, tr_accumulate_kernel, tr_finalize_kernel) */
    const double scale = fixed_point_scale(x, n, dcols, ld), inv_scale = 1.0 / scale;
    int it = 0, converged = 0;
    while (it < maxiter) {
        assign_all(x, n, dcols, ld, centres, k, assign);
        memset(acc, 0, sizeof(int64_t) * (size_t)k * dcols);
        memset(counts, 0, sizeof(uint32_t) * (size_t)k);
        for (int64_t p = 0; p < n; ++p) {
            const int c = assign[p];
            for (int i = 0; i < dcols; ++i) {
                const long long v = llrint((double)x[p * ld + i] * scale);   /* round half to even, as __double2ll_rn */
                acc[(size_t)c * dcols + i] = (int64_t)((uint64_t)acc[(size_t)c * dcols + i] + (uint64_t)v);
            }
            counts[c]++;
        }
        int changed = 0;
        for (int c = 0; c < k; ++c)
            for (int i = 0; i < dcols; ++i) {
                float v;
                if (counts[c] > 0) {
                    v = (float)((double)acc[(size_t)c * dcols + i] * inv_scale / (double)counts[c]);
                } else {
                    const int64_t p = (int64_t)(tr_hash(seed, (uint64_t)it + 7777, (uint64_t)c) % (uint64_t)n);
                    v = x[p * ld + i];
                }
                float *dst = centres + (size_t)c * dcols + i;
                uint32_t vb, ob;
                memcpy(&vb, &v, 4);
                memcpy(&ob, dst, 4);
                if (vb != ob) { *dst = v; changed = 1; }
            }
        ++it;
        if (!changed) { converged = 1; break; }
    }
    *out_iters = it;
    *out_converged = converged;
    free(mind); free(partial); free(assign); free(acc); free(counts);
    return ORA_OK;
}

/* ivfadc_train (train_impl): data n x d row-major -> centroids [kc][d], codebooks [m][k][dsub];
 * iters / converged [1 + m]: Lloyd iterations run and fixed point reached, coarse stage first. */
int ora_train(int d, int64_t n, const float *data, int kc, int k, int m, int coarse_maxiter, int quant_maxiter,
              uint64_t seed, float *out_centroids, float *out_codebooks, int32_t *out_iters, int32_t *out_converged)
{
    if (d < 1 || n < 1 || kc < 2 || kc > n || k < 1 || k > n || k > 65536 || m < 1 || m > d || d % m != 0 ||
        coarse_maxiter < 1 || quant_maxiter < 1)
        return ORA_ERR_ASSERT;
    for (int64_t e = 0; e < n * d; ++e)
        if (!isfinite(data[e])) return ORA_ERR_INVALID;
    const int dsub = d / m;
    int32_t *assign = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
    float *resid = (float *)malloc(sizeof(float) * (size_t)n * d);
    if (!assign || !resid) { free(assign); free(resid); return ORA_ERR_NOMEM; }
    int rc = kmeans(data, n, d, d, kc, coarse_maxiter, seed, out_centroids, &out_iters[0], &out_converged[0]);
    if (rc == ORA_OK) {
        /* final assignment against the final centres -> residuals (tr_residual_kernel) */
        assign_all(data, n, d, d, out_centroids, kc, assign);
        for (int64_t p = 0; p < n; ++p)
            for (int i = 0; i < d; ++i) resid[p * d + i] = data[p * d + i] - out_centroids[(size_t)assign[p] * d + i];
        for (int i = 0; i < m && rc == ORA_OK; ++i)
            rc = kmeans(resid + (size_t)i * dsub, n, dsub, d, k, quant_maxiter, seed + 1 + (uint64_t)i,
                        out_codebooks + (size_t)i * k * dsub, &out_iters[1 + i], &out_converged[1 + i]);
    }
    free(assign);
    free(resid);
    return rc;
}
