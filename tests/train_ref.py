"""Slow numpy restatement of the trainer (ivfadc_train), independent of oracle/train_oracle.c: tests use it to
cross-check the C restatement bit for bit on tiny shapes, and its helpers to judge trained quantizers in float64."""
import numpy as np

M64 = (1 << 64) - 1
f32 = np.float32


def mix64(x):
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def tr_hash(a, b, c):
    return mix64(a + 0x9E3779B97F4A7C15 * (b + 1) + 0xD1B54A32D192ED03 * (c + 1))


def sqdist(x, centres):
    """(n, dcols) x (k, dcols) -> (n, k) Float32 squared distances, columns summed in ascending order."""
    acc = np.zeros((x.shape[0], centres.shape[0]), f32)
    for i in range(x.shape[1]):
        t = x[:, i][:, None] - centres[:, i][None, :]
        acc = acc + t * t
    return acc


def assign(x, centres):
    return sqdist(x, centres).argmin(1)       # first minimum on ties


def quantum(x):
    """The fixed-point quantum 1 / scale of a stage on data x: n * max|x| < 2^e, scale = 2^(61 - e)."""
    e = int(np.frexp(np.float64(x.shape[0]) * np.float64(np.abs(x).max()))[1])
    return np.ldexp(1.0, e - 61)


def kmeans(x, k, maxiter, seed):
    """kmeans_dev on a contiguous (n, dcols) float32 array -> (centres, iterations run, converged)."""
    n, dcols = x.shape
    S = min(n, max(32768, 32 * k))
    nblk = (S + 255) // 256
    sample = x[(np.arange(S, dtype=np.int64) * n) // S]
    centres = np.zeros((k, dcols), f32)
    mind = None
    partial = None
    for j in range(k):
        if j > 0:
            d2 = sqdist(sample, centres[j - 1:j])[:, 0]
            mind = d2 if j == 1 else np.fmin(mind, d2)
            sm = np.zeros((nblk, 256))
            sm.reshape(-1)[:S] = mind.astype(np.float64)
            off = 128
            while off > 0:
                sm[:, :off] = sm[:, :off] + sm[:, off:2 * off]
                off >>= 1
            partial = sm[:, 0]
        if j == 0:
            s = tr_hash(seed, 0, 0) % S
        else:
            total = 0.0
            for b in range(nblk):
                total += float(partial[b])
            u = float(tr_hash(seed, j, 1) >> 11) * (1.0 / 9007199254740992.0)
            if total <= 0.0:
                s = tr_hash(seed, j, 2) % S
            else:
                r = u * total
                run = 0.0
                b = 0
                while b < nblk - 1 and run + float(partial[b]) <= r:
                    run += float(partial[b])
                    b += 1
                s = b * 256
                hi = min(S, b * 256 + 256)
                while s < hi - 1 and run + float(mind[s]) <= r:
                    run += float(mind[s])
                    s += 1
        centres[j] = sample[s]
    scale = 1.0 / quantum(x)
    fixed = np.rint(x.astype(np.float64) * scale).astype(np.int64)     # round half to even
    it = 0
    while it < maxiter:
        a = assign(x, centres)
        acc = np.zeros((k, dcols), np.int64)
        np.add.at(acc, a, fixed)
        counts = np.bincount(a, minlength=k)
        new = centres.copy()
        for c in range(k):
            if counts[c] > 0:
                new[c] = (acc[c].astype(np.float64) * (1.0 / scale) / np.float64(counts[c])).astype(f32)
            else:
                new[c] = x[tr_hash(seed, it + 7777, c) % n]
        changed = not np.array_equal(new.view(np.uint32), centres.view(np.uint32))
        centres = new
        it += 1
        if not changed:
            return centres, it, True
    return centres, it, False


def train(data, kc, k, m, coarse_maxiter, quant_maxiter, seed):
    """ivfadc_train -> (centroids (kc, d), codebooks (m, k, dsub), iters (1 + m,), converged (1 + m,))."""
    x = np.ascontiguousarray(data, f32)
    d = x.shape[1]
    dsub = d // m
    seed %= 1 << 64
    cent, it0, cv0 = kmeans(x, kc, coarse_maxiter, seed)
    resid = x - cent[assign(x, cent)]
    cbs, iters, conv = [], [it0], [cv0]
    for i in range(m):
        cb, it, cv = kmeans(np.ascontiguousarray(resid[:, i * dsub:(i + 1) * dsub]), k, quant_maxiter, (seed + 1 + i) % (1 << 64))
        cbs.append(cb)
        iters.append(it)
        conv.append(cv)
    return cent, np.stack(cbs), np.array(iters), np.array(conv)


def stages(data, cent, m):
    """The (points, centres) of every stage of a trained quantizer, as the trainer saw them at its end: the coarse
    stage on the data, then sub-space i of the Float32 residuals against the final coarse assignment."""
    x = np.ascontiguousarray(data, f32)
    dsub = x.shape[1] // m
    resid = x - cent[assign(x, cent)]
    return x, [np.ascontiguousarray(resid[:, i * dsub:(i + 1) * dsub]) for i in range(m)]


def check_float64_means(x, centres, what):
    """At a Lloyd fixed point every non-empty centre is the Float32-rounded mean of the points assigned to it
    (Float32 argmin, as the trainer assigns).  Error budget per component of centre c:
      fixed point   every x * scale is rounded to an integer (error <= 1/2 unit), so the mean of the rounded values
                    is within q/2 of the exact mean, q = quantum(x);
      double        acc -> double (exact below 2^53, else 2^-53 relative), * 2^-s (exact), / count (2^-53
                    relative), and numpy's float64 mean of the float32 inputs (<= log2(n) 2^-53 of mean|x|):
                    together below 2^-40 mean|x|;
      Float32       the final rounding: half an ulp of the result.
    So |c - mean64| <= ulp(c)/2 + q/2 + 2^-40 mean|x|; the test allows the full quantum q in place of q/2."""
    a = assign(x, centres)
    q = quantum(x)
    for c in np.unique(a):
        pts = x[a == c].astype(np.float64)
        mean = pts.mean(0)
        slack = np.abs(pts).mean(0) * 2.0 ** -40
        tol = 0.5 * np.spacing(np.abs(centres[c])).astype(np.float64) + q + slack
        err = np.abs(centres[c].astype(np.float64) - mean)
        assert np.all(err <= tol), "%s: centre %d is %.3g off the float64 mean (tolerance %.3g, quantum %.3g)" % (
            what, c, float(err.max()), float(tol[err.argmax()]), q)
