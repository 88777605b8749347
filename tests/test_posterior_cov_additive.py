"""GPU: full posterior covariance and posterior samples of GPR_additive (torch prepare of W = P^-1 - blockdiag(K_i^-1), then
asvgp_predict_cov_additive).  Yardstick: cov = sum_i K_i(X1_i, X2_i) + Phi1^T P^-1 Phi2 - sum_i Phi1_i^T K_i^-1 Phi2_i, dense in numpy from the
oracle's P and Kuu (elbo_additive) and bases (evaluate_basis); at the probe's size the same formula through dense torch on the GPU.
Tolerances: DESIGN.md section 5."""
import numpy as np
import pytest
import torch

from oracle import asvgp_oracle as O

pytestmark = pytest.mark.gpu

KINDS = {0: "Matern12", 1: "Matern32", 2: "Matern52"}
DOMS = ((0.0, 1.0), (-1.0, 2.0), (0.5, 1.5), (-2.0, 0.0))


@pytest.fixture(scope="module")
def A():
    import asvgp_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from asvgp_amd import _lib
    _lib.get_lib()
    return asvgp_amd


def matern(kind, v, l, x, y):
    r = np.abs(np.asarray(x).reshape(-1)[:, None] - np.asarray(y).reshape(-1)[None, :]) / l
    if kind == 0:
        return v * np.exp(-r)
    if kind == 1:
        sr = np.sqrt(3.0) * r
        return v * (1 + sr) * np.exp(-sr)
    sr = np.sqrt(5.0) * r
    return v * (1 + sr + r * r * 5 / 3) * np.exp(-sr)


class Case:
    """A GPR_additive model and its dense numpy yardstick."""

    def __init__(self, A, order, kinds, ms, th, s, N, seed=0):
        d = len(ms)
        rng = np.random.default_rng(seed)
        doms = DOMS[:d]
        X = np.stack([rng.uniform(a, b, N) for a, b in doms], 1)
        X = X[np.all([(X[:, i] > a) & (X[:, i] < b) for i, (a, b) in enumerate(doms)], 0)]
        y = sum(np.sin((3 + i) * (X[:, i:i + 1] - a) / (b - a)) for i, (a, b) in enumerate(doms)) + 0.1 * rng.normal(size=(X.shape[0], 1))
        B = getattr(A, "B%dSpline" % order)
        self.mk = lambda th_: [getattr(A, KINDS[kinds[i]])(variance=th_[i][0], lengthscales=th_[i][1]) for i in range(d)]
        self.mkbases = lambda: [B(a, b, m) for (a, b), m in zip(doms, ms)]
        self.model = A.GPR_additive((X, y), self.mk(th), self.mkbases())
        self.model.likelihood.variance.assign(s)
        self.X, self.y, self.doms, self.d = X, y, doms, d
        self.obases = [O.Basis(order, a, b, m) for (a, b), m in zip(doms, ms)]
        self.kinds, self.th, self.s, self.order, self.ms = kinds, th, s, order, ms
        self.vs = sum(v for v, _ in th)
        _, parts = O.elbo_additive(self.obases, kinds, th, s, X, y)
        self.P, self.Kuu = parts["P"], parts["Kuu"]

    def phi(self, Xq):
        return np.concatenate([ob.evaluate_basis(Xq[:, i:i + 1], sparse=False) for i, ob in enumerate(self.obases)], 0)

    def yardstick(self, X1, X2):
        F1, F2 = self.phi(X1), self.phi(X2)
        out = sum(matern(self.kinds[i], self.th[i][0], self.th[i][1], X1[:, i], X2[:, i]) for i in range(self.d))
        return out + F1.T @ np.linalg.solve(self.P, F2) - F1.T @ np.linalg.solve(self.Kuu, F2)   # (Kuu block diagonal)

    def points(self, n, seed=1):
        """n points inside the domain, the first and last cells of every dimension included."""
        rng = np.random.default_rng(seed)
        cols = []
        for i, ((a, b), ob) in enumerate(zip(self.doms, self.obases)):
            dl = ob.delta
            edge = np.array([a + 0.3 * dl, b - 0.2 * dl, a + 0.05 * dl, b - 0.9 * dl, 0.5 * (a + b), b - 0.5 * dl])
            cols.append(np.concatenate([np.roll(edge, i), rng.uniform(a, b, n - len(edge))]))
        return np.stack(cols, 1)


# ------------------------------------------------------------------------------------------------ 1. sweep
# (order, kinds per dimension, m per dimension, lengthscales): every order, d = 1..4, unequal m_i, mixed Materns (orders 1 and 2 carry
# only the Materns their bases support; order 6 has no Matern-5/2, and with Matern-1/2 its P is near singular), different domains per
# dimension.
SWEEP = [(1, [0], [15], [0.3]), (2, [1, 0], [14, 11], [0.2, 0.8]), (3, [2, 1, 0], [13, 16, 10], [0.25, 0.5, 0.4]),
         (4, [1, 2, 0, 1], [16, 12, 13, 14], [0.3, 0.7, 0.5, 0.4]), (5, [2, 1], [17, 14], [0.4, 0.9]),
         (6, [1, 1, 1], [18, 15, 16], [0.3, 0.6, 0.5]), (2, [1, 1, 0, 1], [9, 12, 10, 11], [0.5, 0.4, 0.6, 0.3])]


@pytest.mark.parametrize("order,kinds,ms,ls", SWEEP)
def test_sweep_cross_covariance(A, order, kinds, ms, ls):
    th = [(1.2 - 0.2 * i, l) for i, l in enumerate(ls)]
    c = Case(A, order, kinds, ms, th, 0.02, 4000, seed=order + 10 * len(ms))
    X1 = c.points(40, seed=2)
    X2 = c.points(25, seed=3)[::-1].copy()
    got = c.model.predict_f_cov_device(X1, X2).cpu().numpy()
    assert got.shape == (40, 25)
    np.testing.assert_allclose(got, c.yardstick(X1, X2), rtol=0, atol=1e-8 * c.vs)
    c.model.close()


# ------------------------------------------------------------------------------------------------ 2. consistency, d = 1, PSD
@pytest.fixture(scope="module")
def small(A):
    c = Case(A, 3, [1, 2, 1], [20, 16, 12], [(1.3, 0.25), (0.6, 0.5), (0.9, 0.4)], 0.01, 6000, seed=9)
    yield c
    c.model.close()


def test_consistency(small):
    m = small.model
    X1, X2 = small.points(30, seed=7), small.points(45, seed=8)
    C = m.predict_f_cov_device(X1).cpu().numpy()
    mp, var = m.predict_f(X1)
    np.testing.assert_allclose(np.diag(C), var[:, 0], rtol=0, atol=1e-10 * small.vs)
    assert np.max(np.abs(C - C.T)) <= 1e-12 * small.vs
    C12 = m.predict_f_cov_device(X1, X2).cpu().numpy()
    Call = m.predict_f_cov_device(np.concatenate([X1, X2])).cpu().numpy()
    np.testing.assert_allclose(C12, Call[:30, 30:], rtol=0, atol=1e-14)
    mean, cov = m.predict_f_full_cov(X1)
    assert mean.shape == (30, 1) and cov.shape == (1, 30, 30) and not cov.flags.writeable
    np.testing.assert_array_equal(cov[0], C)
    np.testing.assert_array_equal(mean, mp)
    _, v2 = m.predict_f(X1, full_cov=True)          # predict_f itself stays the reference's: full_cov ignored
    np.testing.assert_array_equal(v2, var)


@pytest.mark.parametrize("order,kind,M", [(1, 0, 40), (3, 1, 60), (4, 2, 50)])
def test_one_dimension_against_gpr_1d(A, order, kind, M):
    """d = 1: the additive model on the 1-D model's data and theta matches GPR_1d.predict_f_cov_device, which reaches its W by back
    substitution in HIP (asvgp_posterior_cov_prepare_1d), not by dense torch inverses."""
    rng = np.random.default_rng(order)
    x = rng.uniform(0.0, 1.0, 5000)
    x = x[(x > 0) & (x < 1)]
    y = (np.sin(7 * x) + 0.1 * rng.normal(size=x.shape[0])).reshape(-1, 1)
    B = getattr(A, "B%dSpline" % order)
    mk = lambda: getattr(A, KINDS[kind])(variance=0.9, lengthscales=0.2)
    m1 = A.GPR_1d((x.reshape(-1, 1), y), mk(), B(0, 1, M))
    ma = A.GPR_additive((x.reshape(-1, 1), y), [mk()], [B(0, 1, M)])
    for m in (m1, ma):
        m.likelihood.variance.assign(0.02)
    Xq = np.concatenate([[0.001, 0.999, 0.5], rng.uniform(0, 1, 97)]).reshape(-1, 1)
    X2 = rng.uniform(0, 1, 60).reshape(-1, 1)
    for a, b in ((Xq, None), (Xq, X2)):
        ref = m1.predict_f_cov_device(a, b).cpu().numpy()
        got = ma.predict_f_cov_device(a, b).cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-8 * 0.9)
    m1.close()
    ma.close()


@pytest.fixture(scope="module")
def m12(A):
    """Matern-1/2 in every dimension: the posterior is PSD."""
    c = Case(A, 2, [0, 0, 0], [18, 14, 12], [(1.0, 0.3), (1.5, 0.6), (0.8, 0.4)], 0.02, 5000, seed=4)
    yield c
    c.model.close()


def test_psd(m12, small):
    # Matern-1/2 in every dimension: the yardstick is PSD, so is the result to 1e-9 sum v_i
    X = m12.points(120, seed=6)
    C = m12.model.predict_f_cov_device(X).cpu().numpy()
    assert np.linalg.eigvalsh(0.5 * (C + C.T)).min() >= -1e-9 * m12.vs
    # Matern-3/2 / 5/2: the posterior of the reference's inner products is itself indefinite, most of all near the ends (DESIGN.md
    # section 5, found on the 1-D model), so the gate is the yardstick's own smallest eigenvalue - 1e-9 sum v_i
    X = small.points(120, seed=10)
    ref = np.linalg.eigvalsh(small.yardstick(X, X)).min()
    C = small.model.predict_f_cov_device(X).cpu().numpy()
    assert np.linalg.eigvalsh(0.5 * (C + C.T)).min() >= min(ref, 0.0) - 1e-9 * small.vs


# ------------------------------------------------------------------------------------------------ 3. samples
# (on the Matern-1/2 model, interior points: cov + jitter I has a Cholesky factor)
def interior(c, n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(a + 0.1 * (b - a), b - 0.1 * (b - a), n) for a, b in c.doms], 1)


def test_samples_shapes_and_seed(m12):
    m = m12.model
    X = interior(m12, 12, 11)
    f = m.predict_f_samples(X, num_samples=5, seed=1)
    assert f.shape == (5, 12, 1) and np.all(np.isfinite(f))
    assert m.predict_f_samples(X, seed=1).shape == (12, 1)
    assert m.predict_f_samples(X, num_samples=3, full_cov=False, seed=1).shape == (3, 12, 1)
    assert m.predict_f_samples(X, full_cov=False, seed=1).shape == (12, 1)
    np.testing.assert_array_equal(m.predict_f_samples(X, num_samples=5, seed=7), m.predict_f_samples(X, num_samples=5, seed=7))
    assert not np.array_equal(m.predict_f_samples(X, num_samples=5, seed=7), m.predict_f_samples(X, num_samples=5, seed=8))


def test_samples_moments(m12):
    m = m12.model
    X = interior(m12, 20, 12)
    Ssz, jitter = 20_000, 1e-6
    mean, cov = m.predict_f_full_cov(X)
    C = cov[0] + jitter * np.eye(20)
    f = m.predict_f_samples(X, num_samples=Ssz, seed=11, jitter=jitter)[:, :, 0]
    assert np.all(np.abs(f.mean(0) - mean[:, 0]) <= 5 * np.sqrt(np.diag(C) / Ssz))
    se_c = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C * C) / Ssz)
    assert np.all(np.abs(np.cov(f, rowvar=False) - C) <= 5 * se_c)
    m1, v1 = m.predict_f(X)
    g = m.predict_f_samples(X, num_samples=Ssz, full_cov=False, seed=12)[:, :, 0]
    assert np.all(np.abs(g.mean(0) - m1[:, 0]) <= 5 * np.sqrt(v1[:, 0] / Ssz))
    assert np.all(np.abs(g.var(0) - v1[:, 0]) <= 5 * v1[:, 0] * np.sqrt(2.0 / Ssz))


def test_samples_duplicates_with_default_jitter(m12):
    from asvgp_amd.banded import NotPositiveDefiniteError
    X = np.repeat(interior(m12, 14, 13), 3, axis=0)    # every point three times: cov is singular
    assert np.all(np.isfinite(m12.model.predict_f_samples(X, num_samples=4, seed=0)))
    with pytest.raises(NotPositiveDefiniteError, match="jitter"):
        m12.model.predict_f_samples(X, num_samples=4, jitter=0.0, seed=0)


# ------------------------------------------------------------------------------------------------ 4. cache, empty input
def test_cache_follows_theta_and_close_frees(A):
    th = [(1.0, 0.3), (0.8, 0.5), (0.6, 0.4)]
    c = Case(A, 2, [1, 1, 0], [16, 13, 11], th, 0.02, 4000, seed=14)
    m = c.model
    X = c.points(30, seed=15)
    c0 = m.predict_f_cov_device(X).cpu().numpy()
    ptr = m._post_cov[1].data_ptr()
    np.testing.assert_array_equal(m.predict_f_cov_device(X).cpu().numpy(), c0)
    assert m._post_cov[1].data_ptr() == ptr                       # unchanged theta: the cached W
    m.predict_f_full_cov(X)
    assert m._post_cov[1].data_ptr() == ptr
    prev = c0
    for change in (lambda: m.kernels[0].variance.assign(1.1), lambda: m.kernels[1].lengthscales.assign(0.45),
                   lambda: m.kernels[2].variance.assign(0.7), lambda: m.kernels[2].lengthscales.assign(0.35),
                   lambda: m.likelihood.variance.assign(0.03)):
        key = m._post_cov[0]
        change()
        cur = m.predict_f_cov_device(X).cpu().numpy()
        assert m._post_cov[0] != key
        assert np.max(np.abs(cur - prev)) > 1e-6
        prev = cur
    th2 = [(1.1, 0.3), (0.8, 0.45), (0.7, 0.35)]
    fresh = A.GPR_additive((c.X, c.y), c.mk(th2), c.mkbases())
    fresh.likelihood.variance.assign(0.03)
    np.testing.assert_allclose(prev, fresh.predict_f_cov_device(X).cpu().numpy(), rtol=0, atol=1e-9 * c.vs)   # (own Phi pass)
    fresh.close()
    m.phi_pass()                                                  # new statistics: the cached W goes with them
    assert m._post_cov is None
    np.testing.assert_allclose(m.predict_f_cov_device(X).cpu().numpy(), prev, rtol=0, atol=1e-9 * c.vs)
    m.close()
    assert m._post_cov is None


def test_empty_input(small):
    m = small.model
    X = small.points(7, seed=16)
    for a, b, shape in ((X[:0], X, (0, 7)), (X, X[:0], (7, 0)), (X[:0], None, (0, 0))):
        out = m.predict_f_cov_device(a, b)
        assert tuple(out.shape) == shape and out.dtype == torch.float64 and out.is_cuda


# ------------------------------------------------------------------------------------------------ 5. the probe's size
def test_probe_size_against_dense_torch(A):
    """d = 8, m_i = 256 (M_tot = 2048), order 3, Matern-3/2 (N = 100k here): 2 000 test points against the same formula through dense
    torch on the GPU (dense Kus, Cholesky solves, GEMMs), and the diagonal against predict_f."""
    from asvgp_amd import utils
    rng = np.random.default_rng(17)
    N, d, m = 100_000, 8, 256
    X = rng.uniform(0.0005, 0.9995, (N, d))
    y = (np.sin(6 * X).sum(1, keepdims=True) + 0.1 * rng.normal(size=(N, 1)))
    th, s = [(1.0 - 0.05 * i, 0.1 + 0.02 * i) for i in range(d)], 0.01
    vs = sum(v for v, _ in th)
    model = A.GPR_additive((X, y), [A.Matern32(variance=v, lengthscales=l) for v, l in th], [A.B3Spline(0, 1, m) for _ in range(d)])
    model.likelihood.variance.assign(s)
    Xq = np.concatenate([np.full((1, d), 0.001), np.full((1, d), 0.999), rng.uniform(0.001, 0.999, (1998, d))])
    got = model.predict_f_cov_device(Xq)
    _, var = model.predict_f(Xq)
    np.testing.assert_allclose(torch.diagonal(got).cpu().numpy(), var[:, 0], rtol=0, atol=1e-10 * vs)
    f = model._factor()
    Xt = torch.from_numpy(Xq).to(got.device)
    Kus = torch.cat([b.evaluate_basis(Xt[:, i:i + 1].contiguous(), sparse=False) for i, b in enumerate(model.bases)], 0)
    Z = torch.linalg.solve_triangular(f["L"], Kus, upper=False)
    ref = Z.t() @ Z
    del Z
    for i, (b, K) in enumerate(zip(model.bases, f["Ks"])):
        LK = torch.linalg.cholesky(utils.band_to_dense_sym(K))
        T = torch.linalg.solve_triangular(LK, Kus[model.offsets[i]:model.offsets[i + 1]], upper=False)
        ref -= T.t() @ T
        ref += torch.from_numpy(matern(1, th[i][0], th[i][1], Xq[:, i], Xq[:, i])).to(got.device)
    assert float((got - ref).abs().max()) <= 1e-8 * vs
    model.close()
