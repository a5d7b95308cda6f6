"""CPU tests of the trainer's restatement (oracle/train_oracle.c, the checker of ivfadc_train): against the independent
numpy restatement in train_ref.py, against float64 Lloyd semantics, and its refusal of non-finite data."""
import numpy as np
import pytest

import train_ref
from oracle import oracle as ora


def _data(kind, seed, n, d):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((n, d), dtype=np.float32)
    if kind == "normal":                                   # negative fixed-point sums
        return rng.standard_normal((n, d)).astype(np.float32)
    if kind == "mixture":
        c = rng.random((6, d), dtype=np.float32) * 4
        return (c[rng.integers(0, 6, n)] + 0.1 * rng.standard_normal((n, d))).astype(np.float32)
    if kind == "repeated":                                 # one point n times: k-means++ takes the total <= 0 branch
        return np.tile(rng.random((1, d), dtype=np.float32), (n, 1))
    if kind == "few":                                      # 5 distinct points: empty clusters restart every iteration
        return rng.random((5, d), dtype=np.float32)[rng.integers(0, 5, n)]
    if kind == "zeros":
        return np.zeros((n, d), np.float32)
    if kind == "mixed":                                    # 1e4 next to 1e-4
        return (rng.standard_normal((n, d)) * np.where(np.arange(d) % 2 == 0, 1e4, 1e-4)).astype(np.float32)
    raise ValueError(kind)


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("kind,n,d,m,kc,k,maxiter,seed", [
    ("uniform", 300, 4, 1, 5, 16, 1, 0),                  # dsub 4, one step from the seeds
    ("uniform", 2000, 12, 4, 16, 16, 25, 3),              # dsub 3, to a fixed point; n % 256 != 0
    ("normal", 1000, 6, 6, 8, 8, 25, 2**64 - 1),          # dsub 1; u64 wrap-around in tr_hash
    ("mixture", 777, 8, 2, 6, 16, 25, 11),
    ("repeated", 300, 3, 3, 4, 4, 3, 5),
    ("few", 500, 8, 2, 8, 16, 25, 7),
    ("zeros", 257, 4, 1, 2, 2, 2, 1),
    ("mixed", 600, 8, 2, 4, 8, 25, 9),
    ("uniform", 40000, 2, 1, 4, 4, 2, 4),                 # n > S: the strided k-means++ sample
])
def test_train_oracle_matches_numpy_restatement(kind, n, d, m, kc, k, maxiter, seed):
    x = _data(kind, seed, n, d)
    cent, cbs, iters, conv = ora.train(x, kc, k, m, maxiter, maxiter, seed)
    ecent, ecbs, eiters, econv = train_ref.train(x, kc, k, m, maxiter, maxiter, seed)
    assert _same(cent, ecent)
    assert _same(cbs, ecbs)
    assert iters.tolist() == eiters.tolist() and conv.tolist() == econv.tolist()


@pytest.mark.parametrize("kind,scale,seed", [("mixture", 1.0, 1), ("normal", 1.0, 2), ("mixed", 1.0, 3),
                                             ("mixture", 1e-18, 4), ("mixture", 1e18, 5)])
def test_train_oracle_converged_stages_are_float64_means(kind, scale, seed):
    """Every stage that reached its fixed point: each centre is the float64 mean of its points within half a Float32
    ulp plus the fixed-point quantum (train_ref.check_float64_means derives the budget)."""
    n, d, m, kc, k = 3000, 8, 4, 6, 8
    x = (_data(kind, seed, n, d) * np.float32(scale)).astype(np.float32)
    cent, cbs, iters, conv = ora.train(x, kc, k, m, 100, 100, seed)
    assert conv.all(), iters
    xs, subs = train_ref.stages(x, cent, m)
    train_ref.check_float64_means(xs, cent, "coarse")
    for i in range(m):
        train_ref.check_float64_means(subs[i], cbs[i], "sub-space %d" % i)


@pytest.mark.parametrize("dsub,kc,k,seed", [(1, 16, 16, 1), (4, 64, 64, 2), (16, 8, 256, 3)])
def test_train_oracle_float32_assignment_matches_float64_argmin(dsub, kc, k, seed):
    """In every stage the Float32 assignment (sequential sums, first minimum) agrees with the float64 argmin except
    where the two float64 distances are closer than the Float32 rounding bound of a sum of dsub squares: each computed
    distance is within (dsub + 3) 2^-24 (1 + small) of the exact one (one rounding each for the difference, its square
    and every partial sum), so a disagreement is allowed only when
    D64[f32 choice] - D64[f64 choice] <= (dsub + 4) 2^-24 (D64[f32 choice] + D64[f64 choice])."""
    m = 2
    x = np.random.default_rng(seed).standard_normal((4000, dsub * m)).astype(np.float32)
    cent, cbs, _, _ = ora.train(x, kc, k, m, 25, 25, seed)
    xs, subs = train_ref.stages(x, cent, m)
    for pts, centres in [(xs, cent)] + [(subs[i], cbs[i]) for i in range(m)]:
        a32 = train_ref.assign(pts, centres)
        d64 = ((pts.astype(np.float64)[:, None, :] - centres.astype(np.float64)[None, :, :]) ** 2).sum(-1)
        a64 = d64.argmin(1)
        rows = np.arange(len(pts))
        gap = d64[rows, a32] - d64[rows, a64]
        bound = (pts.shape[1] + 4) * 2.0 ** -24 * (d64[rows, a32] + d64[rows, a64])
        assert np.all((a32 == a64) | (gap <= bound)), int(((a32 != a64) & (gap > bound)).sum())


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("where", [0, -1])
def test_train_oracle_refuses_non_finite_data(bad, where):
    """As ivfadc_train does (tests/test_abi.py::test_trainer_refuses_non_finite_data_without_gpu)."""
    x = np.random.default_rng(0).random((300, 4), dtype=np.float32)
    x.reshape(-1)[where] = bad
    with pytest.raises(ValueError):
        ora.train(x, 4, 8, 2)
