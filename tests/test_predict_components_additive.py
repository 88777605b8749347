"""GPU: posterior of the additive components f_i(x_i) and of the gradient d f / d x_i = f_i'(x_i) of GPR_additive
(asvgp_predict_components_additive on the cached W = P^-1 - blockdiag(K_i^-1) and alpha = P^-1 Kuf y / sigma2).  Yardsticks: the same
formulas dense in numpy (alpha = solve(P, b) / sigma2, dense P^-1 and Kuu from the oracle's elbo_additive, bases and derivative bases from
the oracle's evaluate_basis), sums against predict_f / predict_f_cov_device, GPR_1d at d = 1, finite differences of the model's own outputs,
and dense torch on the GPU at the probe's size.  Tolerances: DESIGN.md section 5.  Every comparison prints one "COMPERR" line (error over
its scale) for the record."""
import numpy as np
import pytest
import torch

from oracle import asvgp_oracle as O

pytestmark = pytest.mark.gpu

KINDS = {0: "Matern12", 1: "Matern32", 2: "Matern52"}
CK = {1: 3.0, 2: 5.0 / 3.0}                   # -k''(0) = c v / l^2
DOMS = ((0.0, 1.0), (-1.0, 2.0), (0.5, 1.5), (-2.0, 0.0))


@pytest.fixture(scope="module")
def A():
    import asvgp_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from asvgp_amd import _lib
    _lib.get_lib()
    return asvgp_amd


def report(what, err, scale):
    print("COMPERR %-64s %.3e" % (what, err / scale))
    return err / scale


def prior(kinds, th, p):
    """prior_i: v_i for the components, c_i v_i / l_i^2 for the gradient."""
    return np.array([v if p == 0 else CK[k] * v / l ** 2 for k, (v, l) in zip(kinds, th)])


class Case:
    """A GPR_additive model and its dense numpy yardstick of the components (p = 0) and the gradient (p = 1)."""

    def __init__(self, A, order, kinds, ms, th, s, N, seed=0, doms=None):
        d = len(ms)
        rng = np.random.default_rng(seed)
        doms = doms or [DOMS[i % len(DOMS)] for i in range(d)]
        X = np.stack([rng.uniform(a, b, N) for a, b in doms], 1)
        X = X[np.all([(X[:, i] > a) & (X[:, i] < b) for i, (a, b) in enumerate(doms)], 0)]
        y = sum(np.sin((3 + i % 4) * (X[:, i:i + 1] - a) / (b - a)) for i, (a, b) in enumerate(doms)) + 0.1 * rng.normal(size=(X.shape[0], 1))
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
        self.alpha = np.linalg.solve(parts["P"], parts["b"]).reshape(-1) / s
        self.W = np.linalg.inv(parts["P"]) - np.linalg.inv(parts["Kuu"])
        self.off = np.concatenate([[0], np.cumsum(ms)])

    def yardstick(self, Xq, p):
        n, d = Xq.shape[0], self.d
        Ph = [ob.evaluate_basis(Xq[:, i:i + 1], dx=p, sparse=False) for i, ob in enumerate(self.obases)]
        blk = lambda i: slice(self.off[i], self.off[i + 1])
        mean = np.stack([Ph[i].T @ self.alpha[blk(i)] for i in range(d)], 1)
        pr = prior(self.kinds, self.th, p)
        cov = np.empty((n, d, d))
        for i in range(d):
            for j in range(d):
                cov[:, i, j] = np.sum(Ph[i] * (self.W[blk(i), blk(j)] @ Ph[j]), 0) + (pr[i] if i == j else 0.0)
        return mean, cov

    def points(self, n, seed=1):
        """Per dimension: both ends, the first and last cells, knots and one ulp either side of them, then uniform points; the planted
        values rolled by the dimension so that they do not all share a row."""
        rng = np.random.default_rng(seed)
        cols = []
        for i, ((a, b), ob) in enumerate(zip(self.doms, self.obases)):
            mesh, dl = np.asarray(ob.mesh), ob.delta
            j = np.unique(np.linspace(1, mesh.size - 2, min(4, mesh.size - 2)).astype(int))
            knots = mesh[j]
            planted = np.concatenate([mesh[:1], mesh[-1:], [a + 0.3 * dl, b - 0.2 * dl], knots, np.nextafter(knots, -np.inf),
                                      np.nextafter(knots, np.inf)])
            planted = np.resize(planted, 16)
            cols.append(np.concatenate([np.roll(planted, 3 * i), rng.uniform(a, b, n - 16)]))
        return np.stack(cols, 1)

    def check(self, tag, Xq, p, mean, cov):
        rm, rc = self.yardstick(Xq, p)
        n, d = Xq.shape
        assert mean.shape == (n, d) and cov.shape == (n, d, d)
        assert report(tag + " mean", np.max(np.abs(mean - rm)), max(np.max(np.abs(rm)), 1e-300)) <= 1e-9
        pr = prior(self.kinds, self.th, p)
        sc = np.sqrt(np.outer(pr, pr))
        assert report(tag + " cov", np.max(np.abs(cov - rc) / sc), 1.0) <= 1e-8
        np.testing.assert_array_equal(cov, np.swapaxes(cov, 1, 2))


# ------------------------------------------------------------------------------------------------ 1. sweep against the dense yardstick
# components: the configurations of the cross-covariance sweep (test_posterior_cov_additive.SWEEP: orders 1 and 2 carry only the Materns
# their bases support, order 6 has no Matern-5/2); gradient: Matern-3/2 at orders 2-6 and Matern-5/2 at orders 3-5, mixed across
# dimensions; d = 1..4, unequal m_i, the different domains per dimension.
SWEEP_P0 = [(1, [0], [15], [0.3]), (2, [1, 0], [14, 11], [0.2, 0.8]), (3, [2, 1, 0], [13, 16, 10], [0.25, 0.5, 0.4]),
            (4, [1, 2, 0, 1], [16, 12, 13, 14], [0.3, 0.7, 0.5, 0.4]), (5, [2, 1], [17, 14], [0.4, 0.9]),
            (6, [1, 1, 1], [18, 15, 16], [0.3, 0.6, 0.5]), (2, [1, 1, 0, 1], [9, 12, 10, 11], [0.5, 0.4, 0.6, 0.3])]
SWEEP_P1 = [(2, [1, 1], [14, 11], [0.2, 0.8]), (3, [2, 1, 2], [13, 16, 10], [0.25, 0.5, 0.4]),
            (4, [1, 2, 2, 1], [16, 12, 13, 14], [0.3, 0.7, 0.5, 0.4]), (5, [2, 1], [17, 14], [0.4, 0.9]),
            (6, [1, 1, 1], [18, 15, 16], [0.3, 0.6, 0.5]), (3, [1], [20], [0.2]), (4, [2], [15], [0.3])]


@pytest.mark.parametrize("p,order,kinds,ms,ls", [(0,) + c for c in SWEEP_P0] + [(1,) + c for c in SWEEP_P1])
def test_sweep_against_dense_yardstick(A, p, order, kinds, ms, ls):
    th = [(1.2 - 0.2 * i, l) for i, l in enumerate(ls)]
    c = Case(A, order, kinds, ms, th, 0.02, 4000, seed=order + 10 * len(ms) + 100 * p)
    Xq = c.points(48, seed=2 + p)
    fn = c.model.predict_f_gradient if p else c.model.predict_f_components
    mean, cov = fn(Xq)
    c.check("%s order %d %s m=%s" % ("gradient" if p else "components", order, "/".join(KINDS[k] for k in kinds), ms), Xq, p, mean, cov)
    c.model.close()


def test_sixteen_dimensions(A):
    d = 16
    kinds = [1 + i % 2 for i in range(d)]
    ms = [8 + i % 4 for i in range(d)]
    th = [(0.5 + 0.05 * i, 0.3 + 0.02 * i) for i in range(d)]
    c = Case(A, 3, kinds, ms, th, 0.05, 3000, seed=16)
    Xq = c.points(40, seed=3)
    for p, fn in ((0, c.model.predict_f_components), (1, c.model.predict_f_gradient)):
        mean, cov = fn(Xq)
        c.check("d = 16 %s" % ("gradient" if p else "components"), Xq, p, mean, cov)
    c.model.close()


# ------------------------------------------------------------------------------------------------ 2. consistency with predict_f (p = 0)
@pytest.fixture(scope="module")
def small(A):
    c = Case(A, 3, [1, 2, 0], [20, 16, 12], [(1.3, 0.25), (0.6, 0.5), (0.9, 0.4)], 0.01, 6000, seed=9)
    yield c
    c.model.close()


def test_sums_match_predict_f(small):
    m = small.model
    X = small.points(64, seed=7)
    mean, cov = m.predict_f_components(X)
    mp, var = m.predict_f(X)
    assert report("sum_i mean vs predict_f mean", np.max(np.abs(mean.sum(1) - mp[:, 0])), np.max(np.abs(mp))) <= 1e-10
    tot = cov.sum((1, 2))
    assert report("sum_ij cov vs predict_f var", np.max(np.abs(tot - var[:, 0])), small.vs) <= 1e-10
    C = m.predict_f_cov_device(X).cpu().numpy()
    assert report("sum_ij cov vs diag predict_f_cov_device", np.max(np.abs(tot - np.diag(C))), small.vs) <= 1e-10
    np.testing.assert_array_equal(cov, np.swapaxes(cov, 1, 2))
    # a batch and its halves, bit for bit (torch input as well as numpy)
    Xt = torch.from_numpy(X).cuda()
    mb, cb = m.predict_f_components_device(Xt)
    m1, c1 = m.predict_f_components_device(Xt[:29])
    m2, c2 = m.predict_f_components_device(Xt[29:])
    assert torch.equal(torch.cat([m1, m2]), mb) and torch.equal(torch.cat([c1, c2]), cb)
    np.testing.assert_array_equal(mb.cpu().numpy(), mean)
    np.testing.assert_array_equal(cb.cpu().numpy(), cov)


@pytest.fixture(scope="module")
def grad(A):
    c = Case(A, 4, [1, 2, 1], [18, 14, 16], [(1.0, 0.3), (0.8, 0.5), (1.1, 0.4)], 0.02, 4000, seed=19)
    yield c
    c.model.close()


def test_gradient_halves_and_symmetry(grad):
    m = grad.model
    Xt = torch.from_numpy(grad.points(70, seed=4)).cuda()
    mb, cb = m.predict_f_gradient_device(Xt)
    m1, c1 = m.predict_f_gradient_device(Xt[:33])
    m2, c2 = m.predict_f_gradient_device(Xt[33:])
    assert torch.equal(torch.cat([m1, m2]), mb) and torch.equal(torch.cat([c1, c2]), cb)
    assert torch.equal(cb, cb.transpose(1, 2))


def test_empty_input(small, grad):
    for fn in (small.model.predict_f_components_device, grad.model.predict_f_gradient_device, grad.model.predict_f_components_device):
        for X in (np.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.float64, device="cuda")):
            mean, cov = fn(X)
            assert tuple(mean.shape) == (0, 3) and tuple(cov.shape) == (0, 3, 3)
            assert mean.is_cuda and cov.is_cuda and mean.dtype == cov.dtype == torch.float64
    mean, cov = small.model.predict_f_components(np.zeros((0, 3)))
    assert mean.shape == (0, 3) and cov.shape == (0, 3, 3)


# ------------------------------------------------------------------------------------------------ 3. d = 1 against GPR_1d
@pytest.mark.parametrize("order,kind,M", [(1, 0, 40), (3, 1, 60), (4, 2, 50)])
def test_one_dimension_against_gpr_1d(A, order, kind, M):
    """d = 1: the additive model on the 1-D model's data and theta.  GPR_1d reaches its posterior by banded HIP chains, not by dense
    torch inverses: its components are predict_f_device, its gradient predict_f_gradient_device."""
    v, l, s = 0.9, 0.2, 0.02
    rng = np.random.default_rng(order)
    x = rng.uniform(0.0, 1.0, 5000)
    x = x[(x > 0) & (x < 1)]
    y = (np.sin(7 * x) + 0.1 * rng.normal(size=x.shape[0])).reshape(-1, 1)
    B = getattr(A, "B%dSpline" % order)
    mk = lambda: getattr(A, KINDS[kind])(variance=v, lengthscales=l)
    m1 = A.GPR_1d((x.reshape(-1, 1), y), mk(), B(0, 1, M))
    ma = A.GPR_additive((x.reshape(-1, 1), y), [mk()], [B(0, 1, M)])
    for m in (m1, ma):
        m.likelihood.variance.assign(s)
    Xq = np.concatenate([[0.001, 0.999, 0.5], rng.uniform(0, 1, 97)]).reshape(-1, 1)
    tag = "d = 1 order %d %s M=%d" % (order, KINDS[kind], M)
    rm, rv = (t.cpu().numpy() for t in m1.predict_f_device(Xq))
    mean, cov = ma.predict_f_components(Xq)
    assert report(tag + " components mean vs GPR_1d", np.max(np.abs(mean[:, 0] - rm[:, 0])), np.max(np.abs(rm))) <= 1e-9
    assert report(tag + " components var vs GPR_1d", np.max(np.abs(cov[:, 0, 0] - rv[:, 0])), v) <= 1e-8
    if kind:
        rm, rv = (t.cpu().numpy() for t in m1.predict_f_gradient_device(Xq))
        mean, cov = ma.predict_f_gradient(Xq)
        pr = CK[kind] * v / l ** 2
        assert report(tag + " gradient mean vs GPR_1d", np.max(np.abs(mean[:, 0] - rm[:, 0])), np.max(np.abs(rm))) <= 1e-9
        assert report(tag + " gradient var vs GPR_1d", np.max(np.abs(cov[:, 0, 0] - rv[:, 0])), pr) <= 1e-8
    m1.close()
    ma.close()


# ------------------------------------------------------------------------------------------------ 4. finite differences (no oracle)
def test_finite_differences_of_the_models_own_outputs(A):
    kinds, th = [1, 2, 1], [(1.0, 0.3), (0.8, 0.5), (1.1, 0.4)]
    c = Case(A, 4, kinds, [24, 18, 20], th, 0.02, 5000, seed=23)
    m, d = c.model, c.d
    rng = np.random.default_rng(24)
    cols = []
    for ob in c.obases:                                         # >= 0.2 delta (>> 2h) from every knot in every dimension
        cells = rng.integers(0, np.asarray(ob.mesh).size - 1, 30)
        cols.append(np.asarray(ob.mesh)[cells] + ob.delta * rng.uniform(0.2, 0.8, cells.size))
    X = np.stack(cols, 1)
    n = X.shape[0]
    hs = [1e-5 * l for _, l in th]
    mean, cov = m.predict_f_gradient(X)
    for i in range(d):
        e = np.zeros(d)
        e[i] = hs[i]
        fp, _ = m.predict_f(X + e)
        fm, _ = m.predict_f(X - e)
        fd = (fp[:, 0] - fm[:, 0]) / (2 * hs[i])
        assert report("FD mean dimension %d" % i, np.max(np.abs(fd - mean[:, i])), np.max(np.abs(mean[:, i]))) <= 1e-6
    pr = prior(kinds, th, 1)
    a = np.arange(n)
    for i in range(d):
        for j in range(i + 1):
            ei, ej = np.zeros(d), np.zeros(d)
            ei[i], ej[j] = hs[i], hs[j]
            C = m.predict_f_cov_device(np.concatenate([X + ei, X - ei]), np.concatenate([X + ej, X - ej])).cpu().numpy()
            mixed = (C[a, a] - C[a, n + a] - C[n + a, a] + C[n + a, n + a]) / (4 * hs[i] * hs[j])
            assert report("FD cov (%d, %d)" % (i, j), np.max(np.abs(mixed - cov[:, i, j])), np.sqrt(pr[i] * pr[j])) <= 1e-4
    m.close()


# ------------------------------------------------------------------------------------------------ 5. the probe's size
def test_probe_size_against_dense_torch(A):
    """d = 8, m_i = 256 (M_tot = 2048), order 3, Matern-3/2, N = 100k: 2 000 points against the same formulas through dense torch on the
    GPU (dense bases, triangular solves against the dense factor and each K_i, products summed per pair)."""
    from asvgp_amd import utils
    rng = np.random.default_rng(17)
    N, d, mi = 100_000, 8, 256
    X = rng.uniform(0.0005, 0.9995, (N, d))
    y = (np.sin(6 * X).sum(1, keepdims=True) + 0.1 * rng.normal(size=(N, 1)))
    th, s = [(1.0 - 0.05 * i, 0.1 + 0.02 * i) for i in range(d)], 0.01
    model = A.GPR_additive((X, y), [A.Matern32(variance=v, lengthscales=l) for v, l in th], [A.B3Spline(0, 1, mi) for _ in range(d)])
    model.likelihood.variance.assign(s)
    Xq = np.concatenate([np.full((1, d), 0.001), np.full((1, d), 0.999), rng.uniform(0.001, 0.999, (1998, d))])
    f = model._factor()
    dev = f["L"].device
    alpha = torch.cholesky_solve(model.Kuf_y, f["L"])[:, 0] / s
    LKs = [torch.linalg.cholesky(utils.band_to_dense_sym(K)) for K in f["Ks"]]
    Xt = torch.from_numpy(Xq).to(dev)
    for p in (0, 1):
        mean, cov = (model.predict_f_gradient_device if p else model.predict_f_components_device)(Xq)
        Ph = [b.evaluate_basis(Xt[:, i:i + 1].contiguous(), dx=p, sparse=False) for i, b in enumerate(model.bases)]
        rm = torch.stack([Ph[i].t() @ alpha[i * mi:(i + 1) * mi] for i in range(d)], 1)
        Z = []
        for i in range(d):
            E = torch.zeros((d * mi, Xq.shape[0]), dtype=torch.float64, device=dev)
            E[i * mi:(i + 1) * mi] = Ph[i]
            Z.append(torch.linalg.solve_triangular(f["L"], E, upper=False))
        pr = prior([1] * d, th, p)
        rc = torch.empty((Xq.shape[0], d, d), dtype=torch.float64, device=dev)
        for i in range(d):
            for j in range(i):
                rc[:, i, j] = rc[:, j, i] = (Z[i] * Z[j]).sum(0)
            T = torch.linalg.solve_triangular(LKs[i], Ph[i], upper=False)
            rc[:, i, i] = pr[i] + (Z[i] * Z[i]).sum(0) - (T * T).sum(0)
        sc = torch.sqrt(torch.outer(torch.from_numpy(pr), torch.from_numpy(pr))).to(dev)
        tag = "probe size d=8 m=256 k=3 %s" % ("gradient" if p else "components")
        assert report(tag + " mean vs dense torch", float((mean - rm).abs().max()), float(rm.abs().max())) <= 1e-9
        assert report(tag + " cov vs dense torch", float(((cov - rc).abs() / sc).max()), 1.0) <= 1e-8
        del Z
    model.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(A):
    from asvgp_amd._lib import AsvgpError
    for kinds in ([0, 1, 2], [1, 2, 0], [2, 0, 1]):
        c = Case(A, 3, kinds, [12, 11, 10], [(1.0, 0.3), (0.8, 0.4), (0.9, 0.5)], 0.02, 2000, seed=30)
        X = c.points(20, seed=31)
        bad = kinds.index(0)
        for call in (lambda: c.model.predict_f_gradient_device(X), lambda: c.model.predict_f_gradient(X)):
            with pytest.raises(ValueError, match="Matern12") as ei:
                call()
            assert "dimension %d" % bad in str(ei.value)
        assert c.model._post_cov is None and c.model._post_alpha is None      # refused before W is built and before any launch
        mean, cov = c.model.predict_f_components(X)                           # the components of the same model are fine
        c.check("components with Matern-1/2 in dimension %d" % bad, X, 0, mean, cov)
        c.model.close()
    d = 17
    rng = np.random.default_rng(32)
    X = rng.uniform(0.01, 0.99, (600, d))
    m17 = A.GPR_additive((X, np.sin(X[:, :1])), [A.Matern32(variance=1.0, lengthscales=0.3) for _ in range(d)],
                         [A.B2Spline(0, 1, 6) for _ in range(d)])
    for call in (lambda: m17.predict_f_components_device(X[:5]), lambda: m17.predict_f_gradient_device(X[:5])):
        with pytest.raises(AsvgpError, match="d = 17"):
            call()
    m17.close()


# ------------------------------------------------------------------------------------------------ 7. cache
def test_cache_follows_theta(A):
    th = [(1.0, 0.3), (0.8, 0.5), (0.6, 0.4)]
    c = Case(A, 3, [1, 2, 1], [16, 13, 11], th, 0.02, 4000, seed=14)
    m = c.model
    X = c.points(30, seed=15)
    g0 = m.predict_f_gradient(X)
    c0 = m.predict_f_components(X)
    wptr, aptr = m._post_cov[1].data_ptr(), m._post_alpha[1].data_ptr()
    calls = []
    factor = m._factor
    m._factor = lambda: calls.append(1) or factor()
    g1, c1 = m.predict_f_gradient(X), m.predict_f_components(X)
    m.predict_f_cov_device(X)
    assert not calls                                                    # unchanged theta: neither W nor alpha is recomputed
    assert m._post_cov[1].data_ptr() == wptr and m._post_alpha[1].data_ptr() == aptr
    for a, b in zip(g0 + c0, g1 + c1):
        np.testing.assert_array_equal(a, b)
    m.kernels[1].lengthscales.assign(0.45)                             # one dimension's lengthscale
    g2, c2 = m.predict_f_gradient(X), m.predict_f_components(X)
    assert len(calls) == 1 and m._post_alpha[0] == m._post_cov[0]
    th2 = [(1.0, 0.3), (0.8, 0.45), (0.6, 0.4)]
    fresh = A.GPR_additive((c.X, c.y), c.mk(th2), c.mkbases())
    fresh.likelihood.variance.assign(0.02)
    fg, fc = fresh.predict_f_gradient(X), fresh.predict_f_components(X)
    for tag, got, ref, p in (("gradient", g2, fg, 1), ("components", c2, fc, 0)):
        pr = prior([1, 2, 1], th2, p)
        assert report("cache: %s mean vs fresh model" % tag, np.max(np.abs(got[0] - ref[0])), np.max(np.abs(ref[0]))) <= 1e-9
        assert report("cache: %s cov vs fresh model" % tag, np.max(np.abs(got[1] - ref[1]) / np.sqrt(np.outer(pr, pr))), 1.0) <= 1e-9
    assert np.max(np.abs(g2[0] - g0[0])) > 1e-6 and np.max(np.abs(g2[1] - g0[1])) > 1e-6
    fresh.close()
    m.phi_pass()                                                        # new statistics: W and alpha go with them
    assert m._post_cov is None and m._post_alpha is None
    g3 = m.predict_f_gradient(X)
    np.testing.assert_allclose(g3[0], g2[0], rtol=0, atol=1e-9 * np.max(np.abs(g2[0])))
    m.close()
    assert m._post_cov is None and m._post_alpha is None
