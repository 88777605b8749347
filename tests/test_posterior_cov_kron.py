"""GPU: full posterior covariance and posterior samples of GPR_kron (asvgp_kron_dense_inverse + asvgp_predict_cov_kron2d).
Yardstick: cov = K(X1, X2) + Phi1^T P^-1 Phi2 - (Phi_11^T K1^-1 Phi_12) o (Phi_21^T K2^-1 Phi_22), dense in numpy from the oracle's P
(elbo_kron), per-dimension Kuu (make_Kuu) and bases (evaluate_basis); at the config-4 size the same formula through dense torch on the
GPU.  Tolerances: DESIGN.md section 5."""
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
    r = np.abs(np.asarray(x).reshape(-1)[:, None] - np.asarray(y).reshape(-1)[None, :]) / l
    if kind == 0:
        return v * np.exp(-r)
    if kind == 1:
        sr = np.sqrt(3.0) * r
        return v * (1 + sr) * np.exp(-sr)
    sr = np.sqrt(5.0) * r
    return v * (1 + sr + r * r * 5 / 3) * np.exp(-sr)


def dense_sym(band, k):
    return O.unpack_banded_matrix_to_dense(O.symmetrise_band(band, k), k, k)


class Case:
    """A GPR_kron model and its dense numpy yardstick."""

    def __init__(self, A, order, kinds, m1, m2, th, s, N, dom=((0.0, 1.0), (-1.0, 2.0)), seed=0):
        rng = np.random.default_rng(seed)
        (a1, b1), (a2, b2) = dom
        X = np.stack([rng.uniform(a1, b1, N), rng.uniform(a2, b2, N)], 1)
        X = X[(X[:, 0] > a1) & (X[:, 0] < b1) & (X[:, 1] > a2) & (X[:, 1] < b2)]
        y = np.sin(6 * (X[:, :1] - a1) / (b1 - a1)) * np.cos(2 * X[:, 1:]) + 0.1 * rng.normal(size=(X.shape[0], 1))
        B = getattr(A, "B%dSpline" % order)
        mk = lambda: [getattr(A, KINDS[kinds[d]])(variance=th[d][0], lengthscales=th[d][1]) for d in range(2)]
        self.model = A.GPR_kron((X, y), mk(), [B(a1, b1, m1), B(a2, b2, m2)])
        self.model.likelihood.variance.assign(s)
        self.mk, self.X, self.y, self.dom = mk, X, y, dom
        self.obases = [O.Basis(order, a1, b1, m1), O.Basis(order, a2, b2, m2)]
        self.kinds, self.th, self.s, self.order = kinds, th, s, order
        self.vv = th[0][0] * th[1][0]
        _, parts = O.elbo_kron(self.obases, kinds, th, s, X, y)
        self.P = parts["P"]
        self.Pinv = np.linalg.inv(self.P)
        self.Ks = [dense_sym(O.make_Kuu(ob, kd, v, l), order) for ob, kd, (v, l) in zip(self.obases, kinds, th)]

    def phis(self, Xq):
        return [ob.evaluate_basis(Xq[:, d:d + 1], sparse=False) for d, ob in enumerate(self.obases)]

    def yardstick(self, X1, X2):
        P1, P2 = self.phis(X1), self.phis(X2)
        kr = lambda p: (p[0][:, None, :] * p[1][None, :, :]).reshape(-1, p[0].shape[1])
        out = np.ones((X1.shape[0], X2.shape[0]))
        qk = np.ones_like(out)
        for d in range(2):
            out *= matern(self.kinds[d], self.th[d][0], self.th[d][1], X1[:, d], X2[:, d])
            qk *= P1[d].T @ np.linalg.solve(self.Ks[d], P2[d])
        return out + kr(P1).T @ np.linalg.solve(self.P, kr(P2)) - qk

    def points(self, n, seed=1):
        """n points inside the domain, the first and last cells of both dimensions included."""
        rng = np.random.default_rng(seed)
        (a1, b1), (a2, b2) = self.dom
        d1, d2 = self.obases[0].delta, self.obases[1].delta
        edge = np.array([[a1 + 0.3 * d1, a2 + 0.5 * d2], [b1 - 0.2 * d1, b2 - 0.6 * d2], [a1 + 0.7 * d1, b2 - 0.1 * d2],
                         [b1 - 0.9 * d1, a2 + 0.05 * d2], [0.5 * (a1 + b1), a2 + 0.4 * d2], [b1 - 0.5 * d1, 0.5 * (a2 + b2)]])
        inner = np.stack([rng.uniform(a1, b1, n - len(edge)), rng.uniform(a2, b2, n - len(edge))], 1)
        return np.concatenate([edge, inner])


def sigma_and_seeds(model):
    """The dense Sigma of the cache and the selected-inverse blocks it was completed from."""
    Sig, _ = model._posterior_cov()
    f, (SigD, SigS, Bb) = model._post[1], model._post[2]
    return Sig.cpu().numpy(), SigD.cpu().numpy(), SigS.cpu().numpy(), Bb, f.get("twist")


def check_sigma(c, Sig, SigD, SigS, Bb, lay):
    M = c.P.shape[0]
    sc = np.max(np.abs(c.Pinv))
    np.testing.assert_allclose(Sig, c.Pinv, rtol=0, atol=1e-9 * sc)
    assert np.max(np.abs(Sig - Sig.T)) <= 1e-12 * np.max(np.abs(Sig))
    # the blocks the selected inverse holds are copied unchanged: diagonal blocks as they are, SigS at (b+1, b) and mirrored
    if lay is None:
        nb = SigD.shape[0]
        maps = [np.arange(nb * Bb)]
        stacks = [(SigD, SigS if nb > 1 else SigS[:0])]
    else:
        nb, padt, padb = lay["nb"], lay["padt"], lay["padb"]
        t = np.arange(nb * Bb)
        maps = [t - padt, M - 1 - (t - padb)]
        stacks = [(SigD[0], SigS[0]), (SigD[1], SigS[1])]
    for (D_, S_), mp in zip(stacks, maps):
        for b in range(D_.shape[0]):
            r = mp[b * Bb:(b + 1) * Bb]
            ok = (r >= 0) & (r < M)
            assert np.array_equal(Sig[np.ix_(r[ok], r[ok])], D_[b][np.ix_(ok, ok)])
        for b in range(S_.shape[0]):
            r, q = mp[(b + 1) * Bb:(b + 2) * Bb], mp[b * Bb:(b + 1) * Bb]
            okr, okq = (r >= 0) & (r < M), (q >= 0) & (q < M)
            blk = S_[b][np.ix_(okr, okq)]
            assert np.array_equal(Sig[np.ix_(r[okr], q[okq])], blk)
            assert np.array_equal(Sig[np.ix_(q[okq], r[okr])], blk.T)


# ------------------------------------------------------------------------------------------------ 1. sweep
# (order, kind1, kind2, m1, m2, l1, l2): every order, the three Materns and mixed pairs, m1 != m2, different domains.  (Order 6 with a
# Matern-1/2 factor makes cond(P) = 6e14, where numpy's inverse and its Cholesky inverse already differ by 6e-9 of the largest entry.)
SWEEP = [(1, 0, 0, 15, 12, 0.3, 0.6), (2, 1, 1, 14, 11, 0.2, 0.8), (3, 2, 2, 13, 16, 0.25, 0.5), (4, 1, 2, 16, 12, 0.3, 0.7),
         (5, 2, 1, 17, 14, 0.4, 0.9), (6, 1, 1, 18, 15, 0.3, 0.6)]


@pytest.mark.parametrize("order,k1,k2,m1,m2,l1,l2", SWEEP)
def test_sweep_cross_covariance(A, order, k1, k2, m1, m2, l1, l2):
    c = Case(A, order, [k1, k2], m1, m2, [(1.2, l1), (0.8, l2)], 0.02, 4000, seed=order)
    X1 = c.points(40, seed=2)
    X2 = c.points(25, seed=3)[::-1].copy()
    got = c.model.predict_f_cov_device(X1, X2).cpu().numpy()
    np.testing.assert_allclose(got, c.yardstick(X1, X2), rtol=0, atol=1e-8 * c.vv)
    check_sigma(c, *sigma_and_seeds(c.model))
    c.model.close()


# ------------------------------------------------------------------------------------------------ 2. both layouts
@pytest.mark.parametrize("order,m1,m2,N", [(2, 40, 12, 6000), (4, 26, 14, 7000), (1, 50, 31, 8000)])
def test_layouts(A, order, m1, m2, N):
    kind = 0 if order == 1 else 1
    c = Case(A, order, [kind, kind], m1, m2, [(1.1, 0.3), (0.7, 0.6)], 0.05, N, seed=m1)
    model = c.model
    X1 = c.points(60, seed=5)
    out = {}
    for tw in (True, False):
        model.twisted = tw
        assert (model._twist_layout() is not None) == tw
        Sig, SigD, SigS, Bb, lay = sigma_and_seeds(model)
        assert (lay is not None) == tw
        check_sigma(c, Sig, SigD, SigS, Bb, lay)
        cov = model.predict_f_cov_device(X1).cpu().numpy()
        np.testing.assert_allclose(cov, c.yardstick(X1, X1), rtol=0, atol=1e-8 * c.vv)
        _, var = model.predict_f(X1)
        np.testing.assert_allclose(np.diag(cov), var[:, 0], rtol=0, atol=1e-10)
        out[tw] = Sig
    assert np.max(np.abs(out[True] - out[False])) <= 1e-10 * np.max(np.abs(out[False]))
    model.close()


@pytest.mark.parametrize("order,m1,m2,N", [(2, 23, 7, 5000), (1, 63, 31, 8000)])
def test_twisted_layout_with_a_whole_padding_block(A, order, m1, m2, N):
    """M + Bb = 1 mod 2 Bb: the default two-sided layout pads the bottom stack by a whole block (padb = Bb), which the factorisation
    accepts - so must the dense inverse."""
    kind = 0 if order == 1 else 1
    c = Case(A, order, [kind, kind], m1, m2, [(1.1, 0.3), (0.7, 0.6)], 0.05, N, seed=m2)
    model = c.model
    lay = model._twist_layout()
    assert lay is not None and lay["padb"] == lay["Bb"], lay
    Sig, SigD, SigS, Bb, lay2 = sigma_and_seeds(model)
    assert lay2 == lay
    check_sigma(c, Sig, SigD, SigS, Bb, lay)
    X1 = c.points(50, seed=6)
    cov = model.predict_f_cov_device(X1).cpu().numpy()
    np.testing.assert_allclose(cov, c.yardstick(X1, X1), rtol=0, atol=1e-8 * c.vv)
    _, var = model.predict_f(X1)
    np.testing.assert_allclose(np.diag(cov), var[:, 0], rtol=0, atol=1e-10)
    model.close()


# ------------------------------------------------------------------------------------------------ 3. consistency, PSD
@pytest.fixture(scope="module")
def small(A):
    c = Case(A, 3, [1, 2], 20, 16, [(1.3, 0.25), (0.6, 0.5)], 0.01, 6000, seed=9)
    yield c
    c.model.close()


def test_consistency(small):
    m = small.model
    X1, X2 = small.points(30, seed=7), small.points(45, seed=8)
    C = m.predict_f_cov_device(X1).cpu().numpy()
    _, var = m.predict_f(X1)
    np.testing.assert_allclose(np.diag(C), var[:, 0], rtol=0, atol=1e-10)
    assert np.max(np.abs(C - C.T)) <= 1e-12 * small.vv
    C12 = m.predict_f_cov_device(X1, X2).cpu().numpy()
    Call = m.predict_f_cov_device(np.concatenate([X1, X2])).cpu().numpy()
    np.testing.assert_allclose(C12, Call[:30, 30:], rtol=0, atol=1e-14)
    mean, cov = m.predict_f_full_cov(X1)
    assert mean.shape == (30, 1) and cov.shape == (1, 30, 30) and not cov.flags.writeable
    np.testing.assert_array_equal(cov[0], C)
    with pytest.raises(NotImplementedError):          # predict_f itself stays the reference's
        m.predict_f(X1, full_cov=True)


def test_psd(A, small):
    # Matern-1/2 in both dimensions, interior points: the yardstick is PSD, so is the result to 1e-9 v1 v2
    c = Case(A, 2, [0, 0], 18, 14, [(1.0, 0.3), (1.5, 0.6)], 0.02, 5000, seed=4)
    X = c.points(120, seed=6)[6:]
    C = c.model.predict_f_cov_device(X).cpu().numpy()
    assert np.linalg.eigvalsh(0.5 * (C + C.T)).min() >= -1e-9 * c.vv
    c.model.close()
    # Matern-3/2 / 5/2 with points in the end cells: the posterior of the reference's inner products is itself indefinite there
    # (found on the 1-D model), so the gate is the yardstick's own smallest eigenvalue - 1e-9 v1 v2
    X = small.points(120, seed=10)
    ref = np.linalg.eigvalsh(small.yardstick(X, X)).min()
    C = small.model.predict_f_cov_device(X).cpu().numpy()
    assert np.linalg.eigvalsh(0.5 * (C + C.T)).min() >= min(ref, 0.0) - 1e-9 * small.vv


# ------------------------------------------------------------------------------------------------ 4. samples
# (interior points: near the domain ends the Matern-3/2 x 5/2 posterior of `small` is indefinite, see test_psd)
def interior(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.1, 0.9, n), rng.uniform(-0.7, 1.7, n)], 1)


def test_samples_shapes_and_seed(small):
    m = small.model
    X = interior(12, 11)
    f = m.predict_f_samples(X, num_samples=5, seed=1)
    assert f.shape == (5, 12, 1) and np.all(np.isfinite(f))
    assert m.predict_f_samples(X, seed=1).shape == (12, 1)
    assert m.predict_f_samples(X, num_samples=3, full_cov=False, seed=1).shape == (3, 12, 1)
    np.testing.assert_array_equal(m.predict_f_samples(X, num_samples=5, seed=7), m.predict_f_samples(X, num_samples=5, seed=7))
    assert not np.array_equal(m.predict_f_samples(X, num_samples=5, seed=7), m.predict_f_samples(X, num_samples=5, seed=8))


def test_samples_moments(small):
    m = small.model
    X = interior(20, 12)
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


def test_samples_duplicates_without_jitter(small):
    from asvgp_amd.banded import NotPositiveDefiniteError
    X = np.repeat(interior(14, 13), 3, axis=0)    # every point three times: cov is singular
    assert np.all(np.isfinite(small.model.predict_f_samples(X, num_samples=4, seed=0)))
    with pytest.raises(NotPositiveDefiniteError, match="jitter"):
        small.model.predict_f_samples(X, num_samples=4, jitter=0.0, seed=0)


# ------------------------------------------------------------------------------------------------ 5. cache, d != 2
def test_cache_follows_theta_and_close_frees(A):
    th = [(1.0, 0.3), (0.8, 0.5)]
    c = Case(A, 2, [1, 1], 16, 13, th, 0.02, 4000, seed=14)
    m = c.model
    X = c.points(30, seed=15)
    m.predict_f(X)
    assert "G" not in m._post[1]                                  # predict_f alone keeps no G
    c0 = m.predict_f_cov_device(X).cpu().numpy()
    assert "G" not in m._post[1]                                  # dropped once Sigma is built
    ptr = m._post_cov[1].data_ptr()
    np.testing.assert_array_equal(m.predict_f_cov_device(X).cpu().numpy(), c0)
    assert m._post_cov[1].data_ptr() == ptr                       # unchanged theta: the cached Sigma
    prev = c0
    for change in (lambda: m.kernels[0].lengthscales.assign(0.35), lambda: m.kernels[1].lengthscales.assign(0.45),
                   lambda: m.likelihood.variance.assign(0.03)):
        key = m._post_cov[0]
        change()
        cur = m.predict_f_cov_device(X).cpu().numpy()
        assert m._post_cov[0] != key
        assert np.max(np.abs(cur - prev)) > 1e-6
        prev = cur
    fresh = Case(A, 2, [1, 1], 16, 13, [(1.0, 0.35), (0.8, 0.45)], 0.03, 4000, seed=14)
    np.testing.assert_allclose(prev, fresh.model.predict_f_cov_device(X).cpu().numpy(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(prev, fresh.yardstick(X, X), rtol=0, atol=1e-8 * fresh.vv)
    m._post_cov = None                                            # Sigma rebuilt from a posterior that no longer holds G
    np.testing.assert_allclose(m.predict_f_cov_device(X).cpu().numpy(), prev, rtol=0, atol=1e-12)
    m.close()
    assert m._post_cov is None
    fresh.model.close()


def test_three_dimensions_not_implemented(A):
    rng = np.random.default_rng(16)
    X = rng.uniform(0.01, 0.99, (500, 3))
    y = np.sin(3 * X[:, :1]) + 0.1 * rng.normal(size=(500, 1))
    m = A.GPR_kron((X, y), [A.Matern12(variance=1.0, lengthscales=0.3) for _ in range(3)], [A.B1Spline(0, 1, 6) for _ in range(3)])
    for call in (lambda: m.predict_f_cov_device(X[:5]), lambda: m.predict_f_full_cov(X[:5]), lambda: m.predict_f_samples(X[:5], full_cov=False)):
        with pytest.raises(NotImplementedError, match="d = 3"):
            call()


# ------------------------------------------------------------------------------------------------ 6. the config-4 size
def test_config4_size_against_dense_torch(A):
    """128 x 128, k = 4, N = 200k (twisted by default): 2 000 test points against the same formula through dense torch on the GPU
    (P densified from the block band, dense Cholesky solves), and the diagonal against predict_f."""
    rng = np.random.default_rng(17)
    N, m1, m2 = 200_000, 128, 128
    X = rng.uniform(0.0005, 0.9995, (N, 2))
    y = np.sin(8 * X[:, :1]) * np.cos(5 * X[:, 1:]) + 0.1 * rng.normal(size=(N, 1))
    th, s = [(1.1, 0.1), (0.9, 0.15)], 0.01
    mk = lambda: [A.Matern32(variance=th[d][0], lengthscales=th[d][1]) for d in range(2)]
    model = A.GPR_kron((X, y), mk(), [A.B4Spline(0, 1, m1), A.B4Spline(0, 1, m2)])
    model.likelihood.variance.assign(s)
    assert model._twist_layout() is not None
    Xq = np.concatenate([[[0.001, 0.002], [0.999, 0.998], [0.003, 0.997]], rng.uniform(0.001, 0.999, (1997, 2))])
    got = model.predict_f_cov_device(Xq)
    _, var = model.predict_f(Xq)
    np.testing.assert_allclose(torch.diagonal(got).cpu().numpy(), var[:, 0], rtol=0, atol=1e-10)
    dev = got.device
    ob = [O.Basis(4, 0, 1, m1), O.Basis(4, 0, 1, m2)]
    Ks = [torch.from_numpy(dense_sym(O.make_Kuu(b, 1, v, l), 4)).to(dev) for b, (v, l) in zip(ob, th)]
    P = model.KufKfu_dense / s + torch.kron(Ks[0], Ks[1])
    Xt = torch.from_numpy(Xq).to(dev)
    Phi = model._dense_rows(Xt)                                          # (M_tot, n) dim-0 major
    L = torch.linalg.cholesky(P)
    Z = torch.linalg.solve_triangular(L, Phi, upper=False)
    del P, L
    ref = Z.t() @ Z
    del Z
    q = torch.ones_like(ref)
    for d, b in enumerate(model.bases):
        Pd = b.evaluate_basis(Xt[:, d:d + 1].contiguous(), sparse=False)
        q *= Pd.t() @ torch.linalg.solve(Ks[d], Pd)
    kk = torch.from_numpy(matern(1, th[0][0], th[0][1], Xq[:, 0], Xq[:, 0]) * matern(1, th[1][0], th[1][1], Xq[:, 1], Xq[:, 1])).to(dev)
    ref = kk + ref - q
    assert float((got - ref).abs().max()) <= 1e-8 * th[0][0] * th[1][0]
    model.close()
