"""GPU: full posterior covariance and posterior samples of GPR_1d (asvgp_posterior_cov_prepare_1d + asvgp_predict_cov_1d).
Yardstick: cov = K(X1, X2) + Kus1^T (P^-1 - Kuu^-1) Kus2, evaluated densely in numpy (fp64 Cholesky solves), and in long
double with banded factors for the ill-conditioned headline case.  Tolerances: DESIGN.md section 5."""
import os

import numpy as np
import pytest
import torch

from oracle import asvgp_oracle as O

pytestmark = pytest.mark.gpu

KINDS = {0: "Matern12", 1: "Matern32", 2: "Matern52"}


@pytest.fixture(scope="module")
def A():
    import asvgp_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from asvgp_amd import _lib
    _lib.get_lib()
    return asvgp_amd


def matern(kind, v, l, x, y):
    """gpflow's Matern kernels; dtype follows the inputs (fp64 or long double)."""
    x = np.asarray(x).reshape(-1)
    y = np.asarray(y).reshape(-1)
    r = np.abs(x[:, None] - y[None, :]) / l
    if kind == 0:
        return v * np.exp(-r)
    if kind == 1:
        sr = np.sqrt(r.dtype.type(3)) * r
        return v * (1 + sr) * np.exp(-sr)
    sr = np.sqrt(r.dtype.type(5)) * r
    return v * (1 + sr + r * r * 5 / 3) * np.exp(-sr)


def dense_sym(band, k):
    return O.unpack_banded_matrix_to_dense(O.symmetrise_band(band, k), k, k)


def yardstick(ob, kind, Aband, v, l, s, X1, X2):
    """K(X1, X2) + Kus1^T P^-1 Kus2 - Kus1^T Kuu^-1 Kus2 through dense fp64 Cholesky factors."""
    k = ob.order
    Kd = dense_sym(O.make_Kuu(ob, kind, v, l), k)
    Pd = dense_sym(Aband, k) / s + Kd
    K1, K2 = ob.evaluate_basis(X1, sparse=False), ob.evaluate_basis(X2, sparse=False)
    LK, LP = np.linalg.cholesky(Kd), np.linalg.cholesky(Pd)
    tk1, tk2 = np.linalg.solve(LK, K1), np.linalg.solve(LK, K2)
    tp1, tp2 = np.linalg.solve(LP, K1), np.linalg.solve(LP, K2)
    return matern(kind, v, l, X1, X2) + tp1.T @ tp2 - tk1.T @ tk2


def _model(A, order, kind, M, D, v, l, s, N=5000, seed=0, a=0, b=1):
    rng = np.random.default_rng(seed)
    x = rng.uniform(a, b, N)
    x = x[(x > a) & (x < b)]
    y = np.stack([np.sin(7 * (d + 1) * x) for d in range(D)], 1) + 0.1 * rng.normal(size=(x.shape[0], D))
    basis = getattr(A, "B%dSpline" % order)(a, b, M)
    model = A.GPR_1d((x.reshape(-1, 1), y), getattr(A, KINDS[kind])(variance=v, lengthscales=l), basis)
    model.likelihood.variance.assign(s)
    return model, O.Basis(order, a, b, M)


# ------------------------------------------------------------------------------------------------ 1. Snelson
def test_snelson_full_cov(A, golden_dir):
    S = np.load(os.path.join(golden_dir, "snelson_fixtures.npz"))
    Xs = np.loadtxt(os.path.join(golden_dir, "snelson", "test_inputs")).reshape(-1, 1)
    v, l, s = 0.798145059, 1.026880136, 0.080066643
    model = A.GPR_1d((S["X"], S["Y"]), A.Matern32(variance=v, lengthscales=l), A.B3Spline(-3.5, 10.5, 100))
    model.likelihood.variance.assign(s)
    mean, cov = model.predict_f_full_cov(Xs)
    assert mean.shape == (301, 1) and cov.shape == (1, 301, 301)
    assert not cov.flags.writeable
    ob = O.Basis(3, -3.5, 10.5, 100)
    Ab, b, yy = O.sufficient_stats(ob, S["X"], S["Y"])
    ref = yardstick(ob, 1, Ab, v, l, s, Xs, Xs)
    np.testing.assert_allclose(cov[0], ref, rtol=0, atol=1e-8)
    m1, v1 = model.predict_f(Xs)
    np.testing.assert_array_equal(mean, m1)
    np.testing.assert_allclose(np.diag(cov[0]), v1[:, 0], rtol=0, atol=1e-10)
    with pytest.raises(NotImplementedError):          # predict_f itself stays the reference's
        model.predict_f(Xs, full_cov=True)
    model.close()


# ------------------------------------------------------------------------------------------------ 2. sweep
# (order, kind, M, D, lengthscale): every order, every kernel an order has static bands for, M in {16, 257, 2048}, D in {1, 3}
SWEEP = [(1, 0, 16, 1, 0.2), (2, 1, 257, 3, 0.05), (3, 2, 16, 1, 0.1), (4, 0, 2048, 1, 0.02), (5, 2, 257, 1, 0.05),
         (6, 1, 257, 3, 0.05), (3, 1, 2048, 3, 0.02), (2, 0, 2048, 1, 0.05), (6, 0, 16, 1, 0.2), (4, 2, 257, 1, 0.1),
         (5, 1, 16, 3, 0.2), (1, 0, 2048, 3, 0.02)]


@pytest.mark.parametrize("order,kind,M,D,l", SWEEP)
def test_sweep_cross_covariance(A, order, kind, M, D, l):
    v, s = 1.3, 0.01
    model, ob = _model(A, order, kind, M, D, v, l, s)
    rng = np.random.default_rng(1)
    d = ob.delta
    X1 = np.concatenate([[0.0, 0.3 * d, 1 - 0.3 * d, 1.0], rng.uniform(0, 1, 37)])
    X2 = np.concatenate([[1.0, 0.5 * d, 0.0], rng.uniform(0, 1, 21), [1 - 0.7 * d]])
    C12 = model.predict_f_cov_device(X1, X2).cpu().numpy()
    assert C12.shape == (X1.size, X2.size)
    Aband = model.KufKfu.cpu().numpy()
    ref = yardstick(ob, kind, Aband, v, l, s, X1, X2)
    np.testing.assert_allclose(C12, ref, rtol=0, atol=1e-8)
    X = np.concatenate([X1, X2])
    C = model.predict_f_cov_device(X).cpu().numpy()
    np.testing.assert_allclose(C[:X1.size, X1.size:], C12, rtol=0, atol=1e-14)
    assert np.max(np.abs(C - C.T)) <= 1e-12 * v
    _, var = model.predict_f(X)
    np.testing.assert_allclose(np.diag(C), var[:, 0], rtol=0, atol=1e-10)
    # positive semi-definite up to rounding wherever the model's own posterior is: the reference's Matern-3/2 and 5/2 inner products
    # leave k - Kus^T Kuu^-1 Kus indefinite near the boundaries (the dense yardstick and predict_f's variance show the same), so there the
    # gate is the yardstick's smallest eigenvalue
    e = np.linalg.eigvalsh(0.5 * (C + C.T)).min()
    e_ref = np.linalg.eigvalsh(yardstick(ob, kind, Aband, v, l, s, X, X)).min()
    assert e >= min(0.0, e_ref) - 1e-9 * v, (e, e_ref)
    model.close()


# ------------------------------------------------------------------------------------------------ 3. headline conditioning
def _chol_band_ld(Kb):
    k, M = Kb.shape[0] - 1, Kb.shape[1]
    K = np.asarray(Kb, dtype=np.longdouble)
    L = np.zeros_like(K)
    for j in range(M):
        for i in range(j, min(j + k, M - 1) + 1):
            acc = K[i - j, j]
            for p in range(max(0, i - k), j):
                acc -= L[i - p, p] * L[j - p, p]
            L[i - j, j] = np.sqrt(acc) if i == j else acc / L[0, j]
    return L


def _solve_band_ld(L, B):
    """L^-1 B, one row of the result at a time with every column of B at once."""
    k, M = L.shape[0] - 1, L.shape[1]
    T = np.array(B, dtype=np.longdouble)
    for j in range(M):
        acc = T[j].copy()
        for q in range(1, min(k, j) + 1):
            acc -= L[q, j - q] * T[j - q]
        T[j] = acc / L[0, j]
    return T


def test_headline_conditioning_long_double(A):
    M, order, kind, v, l, s = 2048, 4, 1, 1.0, 0.05, 0.01
    model, ob = _model(A, order, kind, M, 1, v, l, s, N=200_000, seed=3)
    xs = np.sort(np.random.default_rng(4).uniform(0, 1, 256))
    C = model.predict_f_cov_device(xs).cpu().numpy()
    _, var = model.predict_f(xs)
    Aband = model.KufKfu.cpu().numpy().astype(np.longdouble)
    Kuu = O.make_Kuu(ob, kind, v, l).astype(np.longdouble)
    Kus = ob.evaluate_basis(xs, sparse=False)
    TK = _solve_band_ld(_chol_band_ld(Kuu), Kus)
    TP = _solve_band_ld(_chol_band_ld(Aband / np.longdouble(s) + Kuu), Kus)
    xl = xs.astype(np.longdouble)
    ref = matern(kind, np.longdouble(v), np.longdouble(l), xl, xl) + TP.T @ TP - TK.T @ TK
    err_full = float(np.max(np.abs(C - ref)))
    err_diag = float(np.max(np.abs(var[:, 0] - np.diag(ref))))
    assert err_full <= err_diag + 1e-8 * v, (err_full, err_diag)


# ------------------------------------------------------------------------------------------------ 4. samples
@pytest.fixture(scope="module")
def small(A):
    model, ob = _model(A, 3, 0, 64, 2, 1.0, 0.1, 0.01, N=3000, seed=5)
    yield model
    model.close()


def test_samples_shapes_and_seed(small):
    X = np.linspace(0.1, 0.9, 12)
    f = small.predict_f_samples(X, num_samples=5, seed=1)
    assert f.shape == (5, 12, 2) and np.all(np.isfinite(f))
    assert small.predict_f_samples(X, seed=1).shape == (12, 2)
    assert small.predict_f_samples(X, num_samples=3, full_cov=False, seed=1).shape == (3, 12, 2)
    np.testing.assert_array_equal(small.predict_f_samples(X, num_samples=5, seed=7), small.predict_f_samples(X, num_samples=5, seed=7))
    assert not np.array_equal(small.predict_f_samples(X, num_samples=5, seed=7), small.predict_f_samples(X, num_samples=5, seed=8))


def test_samples_moments(small):
    X = np.linspace(0.05, 0.95, 20)
    Ssz, jitter = 20_000, 1e-6
    mean, cov = small.predict_f_full_cov(X)
    C = cov[0] + jitter * np.eye(20)
    f = small.predict_f_samples(X, num_samples=Ssz, seed=11, jitter=jitter)
    for d in range(2):
        fd = f[:, :, d]
        se_m = np.sqrt(np.diag(C) / Ssz)
        assert np.all(np.abs(fd.mean(0) - mean[:, d]) <= 5 * se_m)
        Ch = np.cov(fd, rowvar=False)
        se_c = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C * C) / Ssz)
        assert np.all(np.abs(Ch - C) <= 5 * se_c)
    # full_cov=False: independent draws from predict_f's marginals
    m1, v1 = small.predict_f(X)
    g = small.predict_f_samples(X, num_samples=Ssz, full_cov=False, seed=12)
    for d in range(2):
        assert np.all(np.abs(g[:, :, d].mean(0) - m1[:, d]) <= 5 * np.sqrt(v1[:, 0] / Ssz))
        assert np.all(np.abs(g[:, :, d].var(0) - v1[:, 0]) <= 5 * v1[:, 0] * np.sqrt(2.0 / Ssz))
    r = np.corrcoef(g[:, 9, 0], g[:, 10, 0])[0, 1]
    assert abs(r) <= 5 / np.sqrt(Ssz)


def test_samples_singular_and_indefinite(small, A):
    from asvgp_amd.banded import NotPositiveDefiniteError
    X = np.array([0.2, 0.2, 0.5, 0.5, 0.5, 0.8])          # duplicated points: cov is singular
    f = small.predict_f_samples(X, num_samples=4, seed=0)
    assert np.all(np.isfinite(f))
    with pytest.raises(NotPositiveDefiniteError, match="jitter"):
        small.predict_f_samples(X, num_samples=4, jitter=-1.0, seed=0)


# ------------------------------------------------------------------------------------------------ 5. cache
def test_cache_follows_theta_and_close_frees(A):
    model, ob = _model(A, 4, 1, 128, 1, 1.0, 0.1, 0.01, N=4000, seed=6)
    X = np.linspace(0, 1, 50)
    c0 = model.predict_f_cov_device(X).cpu().numpy()
    key0 = model._post_cov[0]
    model.kernel.lengthscales.assign(0.2)
    c1 = model.predict_f_cov_device(X).cpu().numpy()
    assert model._post_cov[0] != key0
    fresh, _ = _model(A, 4, 1, 128, 1, 1.0, 0.2, 0.01, N=4000, seed=6)
    np.testing.assert_allclose(c1, fresh.predict_f_cov_device(X).cpu().numpy(), rtol=0, atol=1e-10)
    assert np.max(np.abs(c1 - c0)) > 1e-3
    model.close()
    assert model._post_cov is None and model._cov_ws is None
    fresh.close()


# ------------------------------------------------------------------------------------------------ 6. both band algorithms
@pytest.mark.parametrize("algo", [0, 1])
def test_dense_band_is_posterior_prepare_band(A, algo):
    A.set_band_algorithm(algo)
    try:
        model, ob = _model(A, 4, 1, 300, 1, 1.0, 0.05, 0.01, N=4000, seed=7)
        Wd = model._posterior_cov().cpu().numpy()
        _, W = model._posterior()
        W = W.cpu().numpy()
        M, k = 300, 4
        for d in range(k + 1):
            j = np.arange(M - d)
            np.testing.assert_array_equal(Wd[j + d, j], W[d, :M - d])
            np.testing.assert_array_equal(Wd[j, j + d], W[d, :M - d])
        np.testing.assert_array_equal(Wd, Wd.T)
        model.close()
    finally:
        A.set_band_algorithm(0)
