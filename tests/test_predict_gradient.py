"""GPU: posterior gradient predictions of GPR_1d and GPR_kron (d = 2): asvgp_predict_deriv_1d, asvgp_predict_cov_deriv_1d and
asvgp_predict_grad_kron2d.  Yardsticks: the same posterior differentiated densely in numpy (derivative bases of the oracle, dense fp64
Cholesky factors of P and Kuu), finite differences of the model's own predict_f_device / predict_f_cov_device, a long-double banded
yardstick at the headline conditioning, and dense torch on the GPU at the eNATL60 size.  Tolerances: DESIGN.md section 5.
Every comparison prints one "GRADERR" line (error over its scale) for the record."""
import numpy as np
import pytest
import torch

from oracle import asvgp_oracle as O

pytestmark = pytest.mark.gpu

KINDS = {0: "Matern12", 1: "Matern32", 2: "Matern52"}
CK = {1: 3.0, 2: 5.0 / 3.0}                   # -k''(0) = c v / l^2


@pytest.fixture(scope="module")
def A():
    import asvgp_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from asvgp_amd import _lib
    _lib.get_lib()
    return asvgp_amd


def report(what, err, scale):
    print("GRADERR %-60s %.3e" % (what, err / scale))
    return err / scale


def matern(kind, v, l, x, y):
    r = np.abs(np.asarray(x).reshape(-1)[:, None] - np.asarray(y).reshape(-1)[None, :]) / l
    if kind == 0:
        return v * np.exp(-r)
    if kind == 1:
        sr = np.sqrt(r.dtype.type(3)) * r
        return v * (1 + sr) * np.exp(-sr)
    sr = np.sqrt(r.dtype.type(5)) * r
    return v * (1 + sr + r * r * 5 / 3) * np.exp(-sr)


def dmatern(kind, v, l, x, y, p, q):
    """d^p/dx^p d^q/dx'^q k(x, x') (Matern-3/2 and 5/2), the closed forms of the issue, written independently of the kernel."""
    if p == 0 and q == 0:
        return matern(kind, v, l, x, y)
    tau = np.asarray(x).reshape(-1)[:, None] - np.asarray(y).reshape(-1)[None, :]
    a = np.sqrt(3.0 if kind == 1 else 5.0) / l
    ar = a * np.abs(tau)
    e = np.exp(-ar)
    if kind == 1:
        dxp = v * a * a * tau * e
        dd = v * a * a * (1 - ar) * e
    else:
        dxp = v * a * a / 3 * tau * (1 + ar) * e
        dd = v * a * a / 3 * (1 + ar - ar * ar) * e
    if p == 1 and q == 1:
        return dd
    return dxp if q == 1 else -dxp


def dense_sym(band, k):
    return O.unpack_banded_matrix_to_dense(O.symmetrise_band(band, k), k, k)


def _model(A, order, kind, M, D, v, l, s, N=5000, seed=0, a=0.0, b=1.0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(a, b, N)
    x = x[(x > a) & (x < b)]
    y = np.stack([np.sin(7 * (d + 1) * x) for d in range(D)], 1) + 0.1 * rng.normal(size=(x.shape[0], D))
    basis = getattr(A, "B%dSpline" % order)(a, b, M)
    model = A.GPR_1d((x.reshape(-1, 1), y), getattr(A, KINDS[kind])(variance=v, lengthscales=l), basis)
    model.likelihood.variance.assign(s)
    return model, O.Basis(order, a, b, M), x, y


class Yard1:
    """The 1-D posterior of f and f' through dense fp64 Cholesky factors of P and Kuu (statistics from the oracle)."""

    def __init__(self, ob, kind, v, l, s, x, y):
        k = ob.order
        Ab, b, _ = O.sufficient_stats(ob, x, y)
        Kd = dense_sym(O.make_Kuu(ob, kind, v, l), k)
        Pd = dense_sym(Ab, k) / s + Kd
        self.LK, self.LP = np.linalg.cholesky(Kd), np.linalg.cholesky(Pd)
        self.alpha = np.linalg.solve(Pd, b) / s
        self.ob, self.kind, self.v, self.l = ob, kind, v, l
        self.prior = CK[kind] * v / l ** 2

    def phi(self, X, dx):
        return self.ob.evaluate_basis(X, dx=dx, sparse=False)

    def mean(self, X):
        return self.phi(X, 1).T @ self.alpha

    def var(self, X):
        P1 = self.phi(X, 1)
        tp, tk = np.linalg.solve(self.LP, P1), np.linalg.solve(self.LK, P1)
        return self.prior + np.sum(tp * tp, 0) - np.sum(tk * tk, 0)

    def cov(self, X1, X2, p, q):
        P1, P2 = self.phi(X1, p), self.phi(X2, q)
        tp1, tp2 = np.linalg.solve(self.LP, P1), np.linalg.solve(self.LP, P2)
        tk1, tk2 = np.linalg.solve(self.LK, P1), np.linalg.solve(self.LK, P2)
        return dmatern(self.kind, self.v, self.l, X1, X2, p, q) + tp1.T @ tp2 - tk1.T @ tk2


def planted_points(ob, n, seed):
    """Both mesh ends, knots, one ulp either side of knots, and uniform points."""
    mesh = np.asarray(ob.mesh)
    j = np.unique(np.linspace(1, mesh.size - 2, min(6, mesh.size - 2)).astype(int))
    knots = mesh[j]
    pts = [mesh[:1], mesh[-1:], knots, np.nextafter(knots, -np.inf), np.nextafter(knots, np.inf),
           np.random.default_rng(seed).uniform(mesh[0], mesh[-1], n)]
    return np.concatenate(pts)


# ------------------------------------------------------------------------------------------------ 1. sweep against the dense yardstick
# (order, kind, M, D, lengthscale): Matern-3/2 at orders 2-6 and Matern-5/2 at orders 3-5 (the orders their static bands allow),
# M in {16, 257, 2048}, D in {1, 3}.  Matern-5/2 at M = 2048 takes l = 0.01 (20 cells): at l = 0.05 cond(Kuu) is beyond what the dense
# fp64 yardstick can resolve (it is off the kernel by 1e-9 of the mean there, as the elbo sweeps found for config 3).
SWEEP = [(2, 1, 257, 3, 0.05), (3, 1, 2048, 1, 0.05), (4, 1, 16, 1, 0.2), (5, 1, 257, 1, 0.05), (6, 1, 2048, 3, 0.05),
         (6, 1, 16, 1, 0.2), (3, 2, 16, 3, 0.2), (4, 2, 2048, 1, 0.01), (5, 2, 257, 1, 0.1)]
BIG = 65_537                                  # odd n >= 65 536: the LDS-staged, paired launch (D = 1) with its odd last point


@pytest.mark.parametrize("order,kind,M,D,l", SWEEP)
def test_sweep_against_dense_yardstick(A, order, kind, M, D, l):
    v, s = 1.3, 0.01
    model, ob, x, y = _model(A, order, kind, M, D, v, l, s)
    yd = Yard1(ob, kind, v, l, s, x, y)
    X = planted_points(ob, 60, seed=order + M)
    ref_m, ref_v = yd.mean(X), yd.var(X)
    m_scale = max(np.max(np.abs(ref_m)), 1e-300)
    tag = "1-D order %d %s M=%d D=%d" % (order, KINDS[kind], M, D)
    # small batch
    mean, var = model.predict_f_gradient(X)
    assert mean.shape == (X.size, D) and var.shape == (X.size, 1)
    assert report(tag + " mean", np.max(np.abs(mean - ref_m)), m_scale) <= 1e-9
    assert report(tag + " var", np.max(np.abs(var[:, 0] - ref_v)), yd.prior) <= 1e-8
    # a large odd batch of the same points (staged, paired, odd last point) and the same batch through a view that is not 16-byte aligned
    idx = np.resize(np.arange(X.size), BIG)
    buf = torch.empty(BIG + 1, dtype=torch.float64, device="cuda")
    buf[1:] = torch.from_numpy(X[idx]).cuda()
    for name, xb in (("aligned", buf[1:].clone()), ("unaligned", buf[1:])):
        assert (xb.data_ptr() % 16 == 0) == (name == "aligned")
        mb, vb = model.predict_f_gradient_device(xb)
        mb, vb = mb.cpu().numpy(), vb.cpu().numpy()
        assert report(tag + " mean, n=%d %s" % (BIG, name), np.max(np.abs(mb - ref_m[idx])), m_scale) <= 1e-9
        assert report(tag + " var, n=%d %s" % (BIG, name), np.max(np.abs(vb[:, 0] - ref_v[idx])), yd.prior) <= 1e-8
    model.close()


# ------------------------------------------------------------------------------------------------ 2. finite differences (no oracle)
@pytest.mark.parametrize("kind", [1, 2])
def test_finite_differences_of_the_models_own_outputs(A, kind):
    v, l, s, M, order = 1.0, 0.1, 0.01, 64, 4
    model, ob, _, _ = _model(A, order, kind, M, 1, v, l, s, seed=11)
    h = 1e-5 * l
    delta = ob.delta
    rng = np.random.default_rng(12)
    cells = rng.integers(0, M - order, 40)
    X = ob.mesh[cells] + delta * rng.uniform(0.2, 0.8, cells.size)       # >= 0.2 delta (>> 2h) from every knot
    mean, var = model.predict_f_gradient(X)
    mp, _ = model.predict_f(X + h)
    mm, _ = model.predict_f(X - h)
    fd = (mp - mm) / (2 * h)
    # central difference of a spline piece: truncation h^2/6 |m'''| ~ h^2 / delta^2 * |m'| ~ 1e-9 relative; rounding eps |m| / h ~ 1e-10
    g_scale = np.max(np.abs(mean))
    assert report("FD mean %s" % KINDS[kind], np.max(np.abs(fd - mean)), g_scale) <= 1e-6
    # mixed second difference of predict_f_cov_device on 2n points: O(a h) = 2e-5 relative truncation for Matern-3/2 (k is C^2 only
    # at 0), O(h^2) for 5/2; rounding ~ 4 eps |C| / h^2 = 4e-4 absolute against c v / l^2 = 300 / 167
    n = X.size
    C = model.predict_f_cov_device(np.concatenate([X - h, X + h])).cpu().numpy()
    i = np.arange(n)
    mixed = (C[n + i, n + i] - C[n + i, i] - C[i, n + i] + C[i, i]) / (4 * h * h)
    prior = CK[kind] * v / l ** 2
    assert report("FD var %s" % KINDS[kind], np.max(np.abs(mixed - var[:, 0])), prior) <= 1e-4
    model.close()


# ------------------------------------------------------------------------------------------------ 3. cross-covariance
@pytest.mark.parametrize("order,kind,M,l", [(4, 1, 257, 0.05), (3, 2, 2048, 0.01), (6, 1, 16, 0.2)])
def test_cross_covariance(A, order, kind, M, l):
    v, s = 1.3, 0.01
    model, ob, x, y = _model(A, order, kind, M, 1, v, l, s, seed=order)
    yd = Yard1(ob, kind, v, l, s, x, y)
    X1 = planted_points(ob, 30, seed=1)
    X2 = np.concatenate([[1.0, 0.0], np.random.default_rng(2).uniform(0, 1, 21)])
    tag = "1-D cov order %d %s M=%d" % (order, KINDS[kind], M)
    scale = {(0, 1): v * np.sqrt(CK[kind]) / l, (1, 0): v * np.sqrt(CK[kind]) / l, (1, 1): yd.prior}
    for pq in ((0, 1), (1, 0), (1, 1)):
        got = model.predict_f_gradient_cov_device(X1, X2, derivs=pq).cpu().numpy()
        assert got.shape == (X1.size, X2.size)
        assert report(tag + " derivs %s" % (pq,), np.max(np.abs(got - yd.cov(X1, X2, *pq))), scale[pq]) <= 1e-8
    c10 = model.predict_f_gradient_cov_device(X1, X2, derivs=(1, 0)).cpu().numpy()
    c01 = model.predict_f_gradient_cov_device(X2, X1, derivs=(0, 1)).cpu().numpy()
    assert report(tag + " (1,0) vs (0,1)^T", np.max(np.abs(c10 - c01.T)), scale[(1, 0)]) <= 1e-12
    C = model.predict_f_gradient_cov_device(X1).cpu().numpy()
    _, var = model.predict_f_gradient(X1)
    assert report(tag + " diag vs gradient var", np.max(np.abs(np.diag(C) - var[:, 0])), yd.prior) <= 1e-10
    assert report(tag + " symmetry", np.max(np.abs(C - C.T)), yd.prior) <= 1e-12
    # derivs (0, 0) is predict_f_cov_device
    np.testing.assert_array_equal(model.predict_f_gradient_cov_device(X1, X2, derivs=(0, 0)).cpu().numpy(),
                                  model.predict_f_cov_device(X1, X2).cpu().numpy())
    model.close()


# ------------------------------------------------------------------------------------------------ 4. headline conditioning
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
    model, ob, _, _ = _model(A, order, kind, M, 1, v, l, s, N=200_000, seed=3)
    xs = np.sort(np.random.default_rng(4).uniform(0, 1, 256))
    _, var = model.predict_f_gradient(xs)
    Aband = model.KufKfu.cpu().numpy().astype(np.longdouble)
    Kuu = O.make_Kuu(ob, kind, v, l).astype(np.longdouble)
    Kus = ob.evaluate_basis(xs, dx=1, sparse=False)
    TK = _solve_band_ld(_chol_band_ld(Kuu), Kus)
    TP = _solve_band_ld(_chol_band_ld(Aband / np.longdouble(s) + Kuu), Kus)
    prior = CK[kind] * v / l ** 2
    ref = np.longdouble(prior) + np.sum(TP * TP, 0) - np.sum(TK * TK, 0)
    assert report("headline gradient var vs long double", float(np.max(np.abs(var[:, 0] - ref))), prior) <= 1e-9
    model.close()


# ------------------------------------------------------------------------------------------------ 5. 2-D
class Case:
    """A GPR_kron model and its dense numpy yardstick of the gradient."""

    def __init__(self, A, order, kinds, m1, m2, th, s, N, dom=((0.0, 1.0), (-1.0, 2.0)), seed=0):
        rng = np.random.default_rng(seed)
        (a1, b1), (a2, b2) = dom
        X = np.stack([rng.uniform(a1, b1, N), rng.uniform(a2, b2, N)], 1)
        X = X[(X[:, 0] > a1) & (X[:, 0] < b1) & (X[:, 1] > a2) & (X[:, 1] < b2)]
        y = np.sin(6 * (X[:, :1] - a1) / (b1 - a1)) * np.cos(2 * X[:, 1:]) + 0.1 * rng.normal(size=(X.shape[0], 1))
        B = getattr(A, "B%dSpline" % order)
        self.model = A.GPR_kron((X, y), [getattr(A, KINDS[kinds[d]])(variance=th[d][0], lengthscales=th[d][1]) for d in range(2)],
                                [B(a1, b1, m1), B(a2, b2, m2)])
        self.model.likelihood.variance.assign(s)
        self.dom = dom
        self.obases = [O.Basis(order, a1, b1, m1), O.Basis(order, a2, b2, m2)]
        _, parts = O.elbo_kron(self.obases, kinds, th, s, X, y)
        self.LP = np.linalg.cholesky(parts["P"])
        self.alpha = np.linalg.solve(parts["P"], parts["b"]) / s
        self.Ks = [dense_sym(O.make_Kuu(ob, kd, v, l), order) for ob, kd, (v, l) in zip(self.obases, kinds, th)]
        self.prior = [CK[kinds[0]] * th[0][0] / th[0][1] ** 2 * th[1][0], CK[kinds[1]] * th[1][0] / th[1][1] ** 2 * th[0][0]]

    def yardstick(self, Xq):
        n = Xq.shape[0]
        V = [ob.evaluate_basis(Xq[:, d:d + 1], sparse=False) for d, ob in enumerate(self.obases)]
        D = [ob.evaluate_basis(Xq[:, d:d + 1], dx=1, sparse=False) for d, ob in enumerate(self.obases)]
        kr = lambda p0, p1: (p0[:, None, :] * p1[None, :, :]).reshape(-1, n)
        psi = [kr(D[0], V[1]), kr(V[0], D[1])]
        mean = np.stack([p.T @ self.alpha[:, 0] for p in psi], 1)
        Z = [np.linalg.solve(self.LP, p) for p in psi]
        q = lambda d, P1, P2: np.sum(P1 * np.linalg.solve(self.Ks[d], P2), 0)
        cov = np.empty((n, 2, 2))
        cov[:, 0, 0] = self.prior[0] + np.sum(Z[0] * Z[0], 0) - q(0, D[0], D[0]) * q(1, V[1], V[1])
        cov[:, 0, 1] = cov[:, 1, 0] = np.sum(Z[0] * Z[1], 0) - q(0, D[0], V[0]) * q(1, V[1], D[1])
        cov[:, 1, 1] = self.prior[1] + np.sum(Z[1] * Z[1], 0) - q(0, V[0], V[0]) * q(1, D[1], D[1])
        return mean, cov

    def points(self, n, seed=1):
        rng = np.random.default_rng(seed)
        (a1, b1), (a2, b2) = self.dom
        d1, d2 = self.obases[0].delta, self.obases[1].delta
        edge = np.array([[a1, a2], [b1, b2], [a1 + 0.3 * d1, b2 - 0.6 * d2], [b1 - 0.2 * d1, a2 + 0.5 * d2],
                         [self.obases[0].mesh[3], self.obases[1].mesh[2]]])
        inner = np.stack([rng.uniform(a1, b1, n - len(edge)), rng.uniform(a2, b2, n - len(edge))], 1)
        return np.concatenate([edge, inner])

    def check(self, tag, mean, cov, Xq):
        rm, rc = self.yardstick(Xq)
        assert mean.shape == (Xq.shape[0], 2) and cov.shape == (Xq.shape[0], 2, 2)
        assert report(tag + " mean", np.max(np.abs(mean - rm)), np.max(np.abs(rm))) <= 1e-9
        sc = np.sqrt(np.outer(self.prior, self.prior))
        assert report(tag + " cov", np.max(np.abs(cov - rc) / sc), 1.0) <= 1e-8
        np.testing.assert_array_equal(cov[:, 0, 1], cov[:, 1, 0])


@pytest.mark.parametrize("order,k1,k2,m1,m2", [(3, 1, 2, 60, 10), (4, 2, 1, 26, 14), (5, 2, 2, 17, 14), (2, 1, 1, 40, 12)])
def test_kron_both_layouts_against_dense_yardstick(A, order, k1, k2, m1, m2):
    c = Case(A, order, [k1, k2], m1, m2, [(1.2, 0.3), (0.8, 0.7)], 0.02, 5000, seed=order)
    Xq = c.points(50)
    out = {}
    for tw in (False, True):
        c.model.twisted = tw
        if tw and c.model._twist_layout() is None:
            continue
        mean, cov = c.model.predict_f_gradient(Xq)
        assert (c.model._post[1].get("twist") is not None) == tw
        c.check("2-D order %d %s x %s %dx%d twisted=%s" % (order, KINDS[k1], KINDS[k2], m1, m2, tw), mean, cov, Xq)
        out[tw] = (mean, cov)
    if order == 3:
        assert len(out) == 2                   # (60 x 10, k = 3: both layouts exist)
        sc = np.sqrt(np.outer(c.prior, c.prior))
        assert np.max(np.abs(out[True][1] - out[False][1]) / sc) <= 1e-10
        assert np.max(np.abs(out[True][0] - out[False][0])) <= 1e-10 * np.max(np.abs(out[False][0]))
    c.model.close()


def test_enatl60_shape_against_dense_torch_and_finite_differences(A):
    """100 x 100 B4, N = 200k (twisted by default): 500 points against the same formulas through dense torch on the GPU, and the mean
    against central differences of predict_f_device."""
    rng = np.random.default_rng(21)
    N, m = 200_000, 100
    X = rng.uniform(0.0005, 0.9995, (N, 2))
    y = np.sin(8 * X[:, :1]) * np.cos(5 * X[:, 1:]) + 0.1 * rng.normal(size=(N, 1))
    th, s = [(1.1, 0.1), (0.9, 0.15)], 0.01
    model = A.GPR_kron((X, y), [A.Matern32(variance=v, lengthscales=l) for v, l in th], [A.B4Spline(0, 1, m), A.B4Spline(0, 1, m)])
    model.likelihood.variance.assign(s)
    assert model._twist_layout() is not None
    Xq = np.concatenate([[[0.001, 0.002], [0.999, 0.998]], rng.uniform(0.001, 0.999, (498, 2))])
    mean, cov = model.predict_f_gradient_device(Xq)
    dev = mean.device
    ob = [O.Basis(4, 0, 1, m), O.Basis(4, 0, 1, m)]
    Ks = [torch.from_numpy(dense_sym(O.make_Kuu(b, 1, v, l), 4)).to(dev) for b, (v, l) in zip(ob, th)]
    P = model.KufKfu_dense / s + torch.kron(Ks[0], Ks[1])
    L = torch.linalg.cholesky(P)
    alpha = torch.cholesky_solve(model.Kuf_y, L) / s
    del P
    Xt = torch.from_numpy(Xq).to(dev)
    n = Xq.shape[0]
    V = [b.evaluate_basis(Xt[:, d:d + 1].contiguous(), sparse=False) for d, b in enumerate(model.bases)]
    D = [b.evaluate_basis(Xt[:, d:d + 1].contiguous(), dx=1, sparse=False) for d, b in enumerate(model.bases)]
    kr = lambda p0, p1: (p0[:, None, :] * p1[None, :, :]).reshape(-1, n)
    psi = [kr(D[0], V[1]), kr(V[0], D[1])]
    rm = torch.stack([p.t() @ alpha[:, 0] for p in psi], 1)
    Z = [torch.linalg.solve_triangular(L, p, upper=False) for p in psi]
    del L
    q = lambda d, P1, P2: (P1 * torch.linalg.solve(Ks[d], P2)).sum(0)
    prior = [3.0 * th[0][0] / th[0][1] ** 2 * th[1][0], 3.0 * th[1][0] / th[1][1] ** 2 * th[0][0]]
    rc = torch.empty((n, 2, 2), dtype=torch.float64, device=dev)
    rc[:, 0, 0] = prior[0] + (Z[0] * Z[0]).sum(0) - q(0, D[0], D[0]) * q(1, V[1], V[1])
    rc[:, 0, 1] = rc[:, 1, 0] = (Z[0] * Z[1]).sum(0) - q(0, D[0], V[0]) * q(1, V[1], D[1])
    rc[:, 1, 1] = prior[1] + (Z[1] * Z[1]).sum(0) - q(0, V[0], V[0]) * q(1, D[1], D[1])
    sc = torch.sqrt(torch.outer(torch.tensor(prior, dtype=torch.float64), torch.tensor(prior, dtype=torch.float64))).to(dev)
    assert report("eNATL60 100x100 B4 mean vs dense torch", float((mean - rm).abs().max()), float(rm.abs().max())) <= 1e-9
    assert report("eNATL60 100x100 B4 cov vs dense torch", float(((cov - rc).abs() / sc).max()), 1.0) <= 1e-8
    # central differences of predict_f_device's mean, points >= 0.2 delta from every knot in both dimensions
    h = 1e-6
    cells = rng.integers(0, m - 4, (40, 2))
    Xf = (cells + rng.uniform(0.2, 0.8, (40, 2))) / (m - 4)
    gm, _ = model.predict_f_gradient(Xf)
    for d in range(2):
        e = np.zeros(2)
        e[d] = h
        fp, _ = model.predict_f(Xf + e)
        fm, _ = model.predict_f(Xf - e)
        fd = (fp[:, 0] - fm[:, 0]) / (2 * h)
        assert report("eNATL60 FD mean dimension %d" % d, np.max(np.abs(fd - gm[:, d])), np.max(np.abs(gm[:, d]))) <= 1e-6
    model.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(A):
    model, _, _, _ = _model(A, 3, 0, 32, 1, 1.0, 0.2, 0.01, N=500)
    for call in (lambda: model.predict_f_gradient_device([0.5]), lambda: model.predict_f_gradient([0.5]),
                 lambda: model.predict_f_gradient_cov_device([0.5], derivs=(1, 0)),
                 lambda: model.predict_f_gradient_cov_device([0.5], derivs=(0, 1))):
        with pytest.raises(ValueError, match="Matern12"):
            call()
    assert model._post is None and model._post_cov is None          # refused before any launch
    model.predict_f_gradient_cov_device([0.5], derivs=(0, 0))        # f itself is fine
    with pytest.raises(ValueError, match="derivs"):
        model.predict_f_gradient_cov_device([0.5], derivs=(2, 0))
    model.close()
    rng = np.random.default_rng(5)
    X = rng.uniform(0.01, 0.99, (2000, 2))
    y = np.sin(3 * X[:, :1]) + 0.1 * rng.normal(size=(2000, 1))
    for kinds in ((A.Matern12, A.Matern32), (A.Matern52, A.Matern12)):
        km = A.GPR_kron((X, y), [K(variance=1.0, lengthscales=0.3) for K in kinds], [A.B3Spline(0, 1, 12), A.B3Spline(0, 1, 10)])
        for call in (lambda: km.predict_f_gradient_device(X[:5]), lambda: km.predict_f_gradient(X[:5])):
            with pytest.raises(ValueError, match="Matern12"):
                call()
        assert km._post is None
        km.close()
    X3 = rng.uniform(0.01, 0.99, (500, 3))
    m3 = A.GPR_kron((X3, np.sin(X3[:, :1])), [A.Matern32(variance=1.0, lengthscales=0.3) for _ in range(3)],
                    [A.B2Spline(0, 1, 6) for _ in range(3)])
    for call in (lambda: m3.predict_f_gradient_device(X3[:5]), lambda: m3.predict_f_gradient(X3[:5])):
        with pytest.raises(NotImplementedError, match="d = 3"):
            call()


# ------------------------------------------------------------------------------------------------ 7. cache
def test_cache_follows_theta(A):
    model, _, _, _ = _model(A, 4, 1, 128, 2, 1.0, 0.1, 0.01, N=4000, seed=6)
    X = np.linspace(0, 1, 50)
    m0, v0 = model.predict_f_gradient(X)
    c0 = model.predict_f_gradient_cov_device(X).cpu().numpy()
    model.kernel.lengthscales.assign(0.2)
    m1, v1 = model.predict_f_gradient(X)
    c1 = model.predict_f_gradient_cov_device(X).cpu().numpy()
    fresh, _, _, _ = _model(A, 4, 1, 128, 2, 1.0, 0.2, 0.01, N=4000, seed=6)
    fm, fv = fresh.predict_f_gradient(X)
    np.testing.assert_allclose(m1, fm, rtol=0, atol=1e-12 * np.max(np.abs(fm)))
    np.testing.assert_allclose(v1, fv, rtol=0, atol=1e-10 * 3.0 / 0.2 ** 2)
    np.testing.assert_allclose(c1, fresh.predict_f_gradient_cov_device(X).cpu().numpy(), rtol=0, atol=1e-10 * 3.0 / 0.2 ** 2)
    assert np.max(np.abs(v1 - v0)) > 1e-3 and np.max(np.abs(m1 - m0)) > 1e-6 and np.max(np.abs(c1 - c0)) > 1e-3
    model.close()
    fresh.close()
    c = Case(A, 3, [1, 2], 20, 12, [(1.0, 0.3), (0.9, 0.5)], 0.02, 3000, seed=9)
    Xq = c.points(30)
    g0 = c.model.predict_f_gradient(Xq)
    c.model.kernels[1].lengthscales.assign(0.4)
    g1 = c.model.predict_f_gradient(Xq)
    f = Case(A, 3, [1, 2], 20, 12, [(1.0, 0.3), (0.9, 0.4)], 0.02, 3000, seed=9)
    g2 = f.model.predict_f_gradient(Xq)
    np.testing.assert_allclose(g1[0], g2[0], rtol=0, atol=1e-12 * np.max(np.abs(g2[0])))
    np.testing.assert_allclose(g1[1], g2[1], rtol=0, atol=1e-10 * np.max(np.abs(g2[1])))
    assert np.max(np.abs(g1[1] - g0[1])) > 1e-3
    c.model.close()
    f.model.close()
