"""The native trainer (ivfadc_train): deterministic, and statistically as good as a reference Lloyd implementation."""
import numpy as np
import pytest

import helpers
import torch_kmeans
import train_ref
from oracle import oracle as ora

pytestmark = pytest.mark.gpu


def _inertia(x, cent):
    d2 = ((x[:, None, :] - cent[None, :, :]) ** 2).sum(-1)
    return float(d2.min(1).sum())


def _mixture(seed, n, d, nc, sigma):
    rng = np.random.default_rng(seed)
    c = rng.random((nc, d), dtype=np.float32)
    return (c[rng.integers(0, nc, n)] + sigma * rng.standard_normal((n, d))).astype(np.float32)


def test_trainer_is_deterministic_and_converges(native):
    x = _mixture(1, 20000, 32, 40, 0.05)
    a = native.trainer.train_ivfadc_hip(x, 40, 64, 8, seed=3)
    b = native.trainer.train_ivfadc_hip(x, 40, 64, 8, seed=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])          # bit for bit
    c = native.trainer.train_ivfadc_hip(x, 40, 64, 8, seed=4)
    assert not np.array_equal(a[0], c[0])
    # quality: within 10 % of the torch/CPU Lloyd trainer, far below a random-centre baseline
    ref = torch_kmeans.train_ivfadc(x, 40, 64, 8, seed=3, device="cpu")
    rng = np.random.default_rng(0)
    rand = x[rng.choice(len(x), 40, replace=False)]
    # k-means++ outcomes vary by tens of percent from seed to seed: compare the better of two native runs
    ia, ir, i0 = min(_inertia(x, a[0]), _inertia(x, c[0])), _inertia(x, ref[0]), _inertia(x, rand)
    assert ia <= 1.25 * ir and ia < 0.5 * i0, (ia, ir, i0)
    # codebooks: the quantisation error of the residuals is comparable too
    def qerr(cent, cbs):
        assign = ((x[:, None, :] - cent[None]) ** 2).sum(-1).argmin(1)
        r = x - cent[assign]
        e = 0.0
        for i in range(8):
            sub = r[:, i * 4:(i + 1) * 4]
            e += float(((sub[:, None, :] - cbs[i][None]) ** 2).sum(-1).min(1).sum())
        return e
    assert qerr(a[0], a[1]) <= 1.3 * qerr(ref[0], ref[1])


def test_constructor_end_to_end_with_native_trainer(native):
    """IVFADCIndex(data; kc, k, m) as in README.md:33-47 (50 x 1000 Float32, kc=100, k=256, m=10, UInt16 ids)."""
    rng = np.random.default_rng(5)
    data = rng.random((1000, 50), dtype=np.float32)
    idx = native.IVFADCIndex(data, kc=100, k=256, m=10, index_type=np.uint16, seed=1)
    assert repr(idx) == "IVFADCIndex, naive coarse quantizer, 12-byte encoding (2 + 1×10), 1000 Float32 vectors"
    ids, dists = native.knn_search(idx, data[122], 3)
    assert ids.dtype == np.uint16 and ids[0] == 122 and np.all(np.diff(dists) >= 0)   # README.md:88-97: the point finds itself
    offsets, codes, lids = idx._lists()
    oidx = ora.OracleIndex(idx._centroids, idx._codebooks, idx._labels, offsets, codes, lids)
    qs = rng.random((20, 50), dtype=np.float32)
    helpers.assert_same_results(idx.search_raw(qs, 5, 4), oidx.knn_search(qs, 5, 4))
    lst, enc = oidx.encode(data)
    assert np.array_equal(np.sort(lids), np.arange(1000))                          # every point indexed once


def test_reference_known_answers_with_native_trainer(native):
    """test/search.jl:26-49 end to end through the product path (native trainer + HIP search)."""
    data = np.array([[0, 0, 0, 1, 1, 1, 1, 1, 20, 20, 20, 20, 20],
                     [0.1, 0.11, 0.12, 8, 10, 15, 14, 16, 5, 5.1, 5.2, 5.4, 5.5]], np.float32).T.copy()
    points = [np.array(p, np.float32) for p in ([1.0, 10.0], [0.0, 0.0], [20.0, 5.0])]
    exp_w1 = [{5, 4, 7, 6, 8}, {1, 2, 3}, {9, 10, 11, 12, 13}]
    exp_w2 = [{5, 4, 7, 6, 8}, {1, 2, 3, 4, 5}, {9, 10, 11, 12, 13}]
    for seed in range(20):                      # k-means++ may merge two of the three clusters: the reference's test data
        idx = native.IVFADCIndex(data, kc=3, k=8, m=2, seed=seed)     # is built for the well-separated outcome
        if np.ptp(idx._centroids[:, 0]) > 15 and len({tuple(np.round(c, 2)) for c in idx._centroids}) == 3:
            break
    for w, exp in ((1, exp_w1), (2, exp_w2)):
        for p, e in zip(points, exp):
            got = set((native.knn_search(idx, p, 5, w=w)[0].astype(int) + 1).tolist())
            assert got and got <= e, (w, got, e)


def test_trainer_assertions(native):
    """test/index.jl:37-40 through the C ABI."""
    x = np.random.default_rng(0).random((300, 2), dtype=np.float32)
    for kc, k, m in ((1, 2, 1), (2, 301, 1), (2, 300, 3)):
        with pytest.raises(AssertionError):
            native.trainer.train_ivfadc_hip(x, kc, k, m)


def test_trainer_quality_at_the_benchmark_shape_vs_sklearn(native):
    """the recall the bench reports is only as good as the trainer.  At the SIFT1M shape's
    quantizer sizes (d = 128, m = 8, kc = 1024, k = 256) on a 2e5-point sample, the native trainer's coarse inertia and
    the quantisation error of its product quantizer must be within 10 % of sklearn.cluster.KMeans (k-means++, Lloyd, 25
    iterations) -- the PQ stage compared on the SAME residuals (those of the native coarse quantizer), so the two
    stages are judged separately.  Data with structure (anisotropic clusters): on isotropic noise every codebook is
    equally useless and the comparison says nothing."""
    import torch
    from sklearn.cluster import KMeans
    n, d, m, kc, k = 200_000, 128, 8, 1024, 256
    rng = np.random.default_rng(77)
    cen = rng.random((300, d), dtype=np.float32)
    basis = np.linalg.qr(rng.standard_normal((d, 24)))[0].astype(np.float32)
    scale = (0.05 + 0.3 * rng.random(24)).astype(np.float32)
    x = (cen[rng.integers(0, 300, n)] + (rng.standard_normal((n, 24)).astype(np.float32) * scale) @ basis.T
         + 0.02 * rng.standard_normal((n, d)).astype(np.float32)).astype(np.float32)
    cent, cbs, _ = native.trainer.train_ivfadc_hip(x, kc, k, m, 25, 25, seed=7)

    def assign(xx, cc):
        xt, ct = torch.as_tensor(xx), torch.as_tensor(cc)
        out = torch.empty(xx.shape[0], dtype=torch.int64)
        dist = torch.empty(xx.shape[0])
        for s in range(0, xx.shape[0], 20000):
            dd = torch.cdist(xt[s:s + 20000], ct) ** 2
            dist[s:s + 20000], out[s:s + 20000] = dd.min(1)
        return out.numpy(), float(dist.sum())

    a_nat, inertia_nat = assign(x, cent)
    sk = KMeans(n_clusters=kc, init="k-means++", n_init=1, max_iter=25, algorithm="lloyd", random_state=0).fit(x)
    inertia_sk = float(sk.inertia_)
    assert inertia_nat <= 1.10 * inertia_sk, "coarse inertia %.4g vs sklearn %.4g" % (inertia_nat, inertia_sk)
    resid = x - cent[a_nat]
    dsub = d // m
    err_nat = err_sk = 0.0
    for i in range(m):
        sub = np.ascontiguousarray(resid[:, i * dsub:(i + 1) * dsub])
        err_nat += assign(sub, cbs[i])[1]
        err_sk += float(KMeans(n_clusters=k, init="k-means++", n_init=1, max_iter=25, algorithm="lloyd", random_state=i).fit(sub).inertia_)
    assert err_nat <= 1.10 * err_sk, "PQ error %.4g vs sklearn %.4g" % (err_nat, err_sk)
    print("trainer vs sklearn: coarse inertia %.4g / %.4g, PQ error %.4g / %.4g" % (inertia_nat, inertia_sk, err_nat, err_sk))


# ---- bit-exact pinning against the CPU restatement (oracle/train_oracle.c) ------------------------------------------

def _train_data(kind, seed, n, d):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((n, d), dtype=np.float32)
    if kind == "normal":                                    # negative fixed-point sums
        return rng.standard_normal((n, d)).astype(np.float32)
    if kind == "mixture":
        return _mixture(seed, n, d, 40, 0.05)
    if kind == "zeros":                                     # maxabs = 0; k-means++ takes the total <= 0 branch
        return np.zeros((n, d), np.float32)
    if kind == "repeated":                                  # one point n times: total <= 0 branch
        return np.tile(rng.standard_normal((1, d)).astype(np.float32), (n, 1))
    if kind == "few":                                       # 300 distinct points < k: empty clusters restart every iteration
        return rng.random((300, d), dtype=np.float32)[rng.integers(0, 300, n)]
    if kind == "mixed":                                     # columns of magnitude 1e4 next to 1e-4
        return (rng.standard_normal((n, d)) * np.where(np.arange(d) % 2 == 0, 1e4, 1e-4)).astype(np.float32)
    raise ValueError(kind)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# every value of every axis at least once: n % 256 tails (300, 4097) and the strided k-means++ sample (40 000 > S);
# dsub 4 / 5 / 1 / 16 / 6 (5, 1 and 6 leave sub-space windows that are not 16-byte aligned: coarse_dist_kernel's scalar
# loads); k > 256 (UInt16 labels) and k = 8192 at n = 40 000 (two Lloyd assignment chunks); maxiter 1 / 2 / 25
@pytest.mark.parametrize("kind,n,d,m,kc,k,maxiter,seed", [
    ("uniform", 300, 32, 8, 2, 2, 25, 0),
    ("normal", 4097, 50, 10, 64, 16, 25, 3),
    ("mixture", 4097, 12, 12, 64, 256, 2, 2**64 - 1),
    ("mixture", 40000, 128, 8, 1024, 256, 1, 0),
    ("uniform", 40000, 32, 8, 2, 8192, 2, 3),
    ("few", 4097, 96, 16, 64, 1024, 25, 0),
    ("zeros", 300, 32, 8, 2, 16, 25, 3),
    ("repeated", 300, 50, 10, 2, 16, 25, 2**64 - 1),
    ("mixed", 4097, 32, 8, 64, 256, 25, 3),
])
def test_trainer_matches_cpu_restatement_bit_for_bit(native, kind, n, d, m, kc, k, maxiter, seed):
    x = _train_data(kind, seed, n, d)
    cent, cbs, _ = native.trainer.train_ivfadc_hip(x, kc, k, m, maxiter, maxiter, seed=seed)
    ecent, ecbs, _, _ = ora.train(x, kc, k, m, maxiter, maxiter, seed)
    assert np.array_equal(_bits(cent), _bits(ecent)), "centroids differ in %d of %d values" % (
        int((_bits(cent) != _bits(ecent)).sum()), cent.size)
    assert np.array_equal(_bits(cbs), _bits(ecbs)), "codebooks differ in %d of %d values" % (
        int((_bits(cbs) != _bits(ecbs)).sum()), cbs.size)


@pytest.mark.parametrize("e", [-40, -20, 20, 40])
def test_trainer_commutes_with_power_of_two_scaling(native, e):
    """train(x * 2^e) == train(x) * 2^e bit for bit: the fixed-point quantum follows the data's binary exponent, and
    every Float32 / double operation of the trainer is exact under a power-of-two scaling while its results stay
    normal.  The data (|x| < 2^5) keep them so for |e| <= 40: at the trained quantizer the smallest nonzero squared
    difference (x - c)^2 is ~2^-42 and the largest distance ~2^11, i.e. 2^-122 and 2^91 after scaling by 2^(2e)
    (Float32 normals: 2^-126 .. 2^128); the premise is asserted below."""
    rng = np.random.default_rng(21)
    n, d, m, kc, k = 4097, 32, 8, 16, 16
    c = rng.random((12, d)) * 16.0
    x = (c[rng.integers(0, 12, n)] + rng.standard_normal((n, d))).astype(np.float32)
    cent, cbs, _ = native.trainer.train_ivfadc_hip(x, kc, k, m, 25, 25, seed=3)
    xs, subs = train_ref.stages(x, cent, m)
    for pts, cen in [(xs, cent)] + [(subs[i], cbs[i]) for i in range(m)]:
        t = pts[:, None, :] - cen[None]
        t2 = t * t
        assert t2[t2 > 0].min() >= 2.0 ** (-126 + 80) and t2.sum(-1).max() < 2.0 ** (128 - 80 - 1)
    xe = np.ldexp(x, e).astype(np.float32)
    assert np.array_equal(np.ldexp(xe, -e).astype(np.float32), x)          # the scaling itself is exact
    scent, scbs, _ = native.trainer.train_ivfadc_hip(xe, kc, k, m, 25, 25, seed=3)
    assert np.array_equal(_bits(scent), _bits(np.ldexp(cent, e).astype(np.float32))), "centroids, e = %d" % e
    assert np.array_equal(_bits(scbs), _bits(np.ldexp(cbs, e).astype(np.float32))), "codebooks, e = %d" % e


@pytest.mark.parametrize("scale", [1.0, 1e-18])
def test_trainer_output_is_a_float64_lloyd_fixed_point(native, scale):
    """On a well-separated mixture, with maxiter chosen so that every stage reaches its fixed point (the restatement
    reports it), every centroid and every codeword is the float64 mean of its cluster within half a Float32 ulp plus
    the fixed-point quantum (tests/train_ref.py:check_float64_means).  At 1e-18, n * max|x| < 1."""
    n, d, m, kc, k, maxiter = 4097, 16, 4, 8, 16, 100
    rng = np.random.default_rng(8)
    centres = rng.random((8, d)) * 4.0
    x = ((centres[rng.integers(0, 8, n)] + 0.05 * rng.standard_normal((n, d))) * scale).astype(np.float32)
    _, _, iters, conv = ora.train(x, kc, k, m, maxiter, maxiter, 5)
    assert conv.all(), iters
    cent, cbs, _ = native.trainer.train_ivfadc_hip(x, kc, k, m, maxiter, maxiter, seed=5)
    xs, subs = train_ref.stages(x, cent, m)
    train_ref.check_float64_means(xs, cent, "coarse")
    for i in range(m):
        train_ref.check_float64_means(subs[i], cbs[i], "sub-space %d" % i)
