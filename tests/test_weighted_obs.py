"""GPU: per-observation noise weights of GPR_1d and GPR_kron (d = 2): asvgp_phi_accumulate_1d_weighted, the two weighted Kronecker
entries, asvgp_set_weight_sums and the Python surface.  Observation i has noise variance sigma2 / w_i; a row with w_i = 0 is absent.
Yardsticks: a direct fp64 numpy accumulation of the weighted statistics written here, the EXISTING unweighted path on replicated /
masked / rescaled data, the oracle's long-double bound fed with the weighted statistics plus the closed-form terms of the model
(include/asvgp_hip.h), a dense numpy bound for the Kronecker model.  Tolerances: DESIGN.md section 5.
Every comparison prints one "WERR" line (error over its scale) for the record."""
import os

import numpy as np
import pytest
import torch

from oracle import asvgp_oracle as O

pytestmark = pytest.mark.gpu

WEIGHTED_BAND_SCATTER = 11                    # asvgp_phi_last_algorithm after the weighted 1-D entry: the general kernel
WEIGHTED_MOMENTS = 16                         # ... the register-moment kernel (D = 1, N >= 2, M <= 2048, aligned x / y / w, exact linspace mesh)


def expected_algorithm(N, M, D, f32mesh, unaligned):
    return WEIGHTED_MOMENTS if (D == 1 and N >= 2 and M <= 2048 and not f32mesh and not unaligned) else WEIGHTED_BAND_SCATTER


@pytest.fixture(scope="module")
def A():
    import asvgp_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from asvgp_amd import _lib
    _lib.get_lib()
    return asvgp_amd


@pytest.fixture(scope="module")
def S(golden_dir):
    return np.load(os.path.join(golden_dir, "snelson_fixtures.npz"))


def report(what, err, scale):
    r = float(err) / float(scale) if scale else float(err)
    print("WERR %-72s %.3e" % (what, r))
    return r


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


# ------------------------------------------------------------------------------------------------ yardsticks written here
def weighted_stats_1d(ob, x, y, w):
    """A_w (lower band), b_w, yy_w and [sum w, sum log w, N+] by direct fp64 accumulation (oracle.sufficient_stats_direct with a weight)."""
    k, M = ob.order, ob.m
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(x.shape[0], -1)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    idx = O.neighbour_index(ob.mesh, x)
    t = (x - ob.mesh[idx]) / ob.delta
    vals = O.piece_values(k, t)               # piece i -> row idx + k - i
    band = np.zeros((k + 1, M))
    rhs = np.zeros((M, y.shape[1]))
    for i in range(k + 1):
        for d in range(y.shape[1]):
            rhs[:, d] += np.bincount(idx + k - i, weights=w * vals[i] * y[:, d], minlength=M)
        for j in range(i, k + 1):
            band[j - i] += np.bincount(idx + k - j, weights=w * vals[i] * vals[j], minlength=M)
    pos = w > 0
    return band, rhs, float(np.sum(w[:, None] * y * y)), (float(np.sum(w)), float(np.sum(np.log(w[pos]))), int(np.sum(pos)))


def weighted_oracle_1d(ob, kind, band, rhs, yy, ws, v, l, s, extended=True):
    """ELBO_w and its gradient: the oracle's bound on the weighted statistics with N+ rows + the closed-form terms of the model."""
    sw, lam, npos = ws
    f = O.elbo_grad_1d_extended if extended else O.elbo_grad_1d
    r = f(ob, kind, band, rhs, yy, npos, v, l, s)
    e, g = r[0], np.array(r[1], dtype=np.float64)
    D = rhs.shape[1]
    e = e + 0.5 * D * lam - 0.5 * (sw - npos) * v / s
    g[0] -= 0.5 * (sw - npos) / s
    g[2] += 0.5 * (sw - npos) * v / s ** 2
    return e, g


def khatri_rao(obases, X):
    """dense (m1 m2, N) Khatri-Rao design matrix, dim-0 major"""
    P1 = obases[0].evaluate_basis(X[:, :1], sparse=False)
    P2 = obases[1].evaluate_basis(X[:, 1:], sparse=False)
    return (P1[:, None, :] * P2[None, :, :]).reshape(-1, X.shape[0])


def weighted_kron_dense(obases, kinds, thetas, s, X, y, w):
    """Dense numpy ELBO_w of the Kronecker model (the steps of oracle.elbo_kron on Phi W Phi^T, Phi W y, sum w y^2) + its statistics."""
    Phi = khatri_rao(obases, X)
    Aw = (Phi * w[None, :]) @ Phi.T
    bw = Phi @ (w[:, None] * y)
    yy = float(np.sum(w[:, None] * y * y))
    pos = w > 0
    npos, sw, lam = int(pos.sum()), float(w.sum()), float(np.log(w[pos]).sum())
    Ks = [O.band_to_dense_sym(O.make_Kuu(bs, kd, v, l)) for bs, kd, (v, l) in zip(obases, kinds, thetas)]
    Kuu = np.kron(Ks[0], Ks[1])
    LK = np.linalg.cholesky(Kuu)
    LP = np.linalg.cholesky(Aw / s + Kuu)
    c = np.linalg.solve(LP, bw) / s
    vprod = float(np.prod([v for v, _ in thetas]))
    tr = np.trace(np.linalg.solve(Kuu, Aw))
    e = (-0.5 * npos * np.log(2 * np.pi * s) - np.sum(np.log(np.diag(LP))) + np.sum(np.log(np.diag(LK))) - 0.5 * yy / s + 0.5 * np.sum(c * c)
         - 0.5 * sw * vprod / s + 0.5 * tr / s + 0.5 * lam)
    return float(e), Aw, bw, yy, (sw, lam, npos)


def sparse_to_blockband(Asp, k, m1, m2):
    """the block-band layout of asvgp_phi_accumulate_kron2d (n_off x M_tot, lower triangle) of a sparse symmetric M_tot x M_tot matrix"""
    M = m1 * m2
    offs = [(0, d2) for d2 in range(k + 1)] + [(d1, d2) for d1 in range(1, k + 1) for d2 in range(-k, k + 1)]
    out = np.zeros((len(offs), M))
    i1, i2 = np.divmod(np.arange(M), m2)
    Asp = Asp.tocsr()
    for o, (d1, d2) in enumerate(offs):
        ok = (i1 + d1 < m1) & (i2 + d2 >= 0) & (i2 + d2 < m2)
        c = np.arange(M)[ok]
        out[o, c] = np.asarray(Asp[c + d1 * m2 + d2, c]).reshape(-1)
    return out


def elbo_tol(e, N, v, s, yy, bcr=False):
    """the tolerance of the existing Kronecker / sharded tests (tests/test_gpu_parity.py elbo_tol)"""
    return 1e-9 * abs(e) + (5e-10 if bcr else 2e-11) * (0.5 * N * v / s + 0.5 * yy / s)


def make_weights(rng, n, kind):
    if kind == "decades":                    # log-uniform over 12 decades, a third exactly 0
        w = 10.0 ** rng.uniform(-6, 6, n)
        w[rng.random(n) < 1 / 3] = 0.0
    elif kind == "integer":
        w = rng.integers(0, 4, n).astype(np.float64)
    elif kind == "lognormal":
        w = np.exp(rng.normal(size=n))
    else:
        raise ValueError(kind)
    return w


def make_x(rng, n, a, b, layout):
    lo, hi = a + 1e-9 * (b - a), b - 1e-9 * (b - a)
    if layout == "clustered":                # a few narrow clusters: whole wavefronts inside one cell, and empty cells
        c = rng.uniform(lo, hi, 7)
        x = np.clip(c[rng.integers(0, 7, n)] + 1e-4 * (b - a) * rng.normal(size=n), lo, hi)
    else:
        x = rng.uniform(lo, hi, n)
    return np.sort(x) if layout == "sorted" else x


def run_weighted_1d(A, ob, x_t, y_t, w_t, D, algo=0, handle=None):
    """asvgp_phi_accumulate_1d_weighted through the C-ABI on device tensors (any alignment) -> (band, rhs, yy, wstats, algorithm)"""
    from asvgp_amd import _lib
    lib = _lib.get_lib()
    k, M = ob.order, ob.m
    h = handle or _lib.Handle()
    h.set_phi_algorithm(algo)
    mesh = dev(ob.mesh)
    stats = torch.full(((k + 1) * M + M * D + 1,), 7.0, dtype=torch.float64, device="cuda")     # (the entry overwrites it)
    wst = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    wsb = lib.asvgp_phi_weighted_workspace_bytes(M, k, D)
    assert wsb >= lib.asvgp_phi_workspace_bytes(M, k, D)
    ws = torch.empty(wsb // 8, dtype=torch.float64, device="cuda")
    N = x_t.shape[0]
    rc = lib.asvgp_phi_accumulate_1d_weighted(h.ptr, x_t.data_ptr(), y_t.data_ptr(), w_t.data_ptr(), N, D, mesh.data_ptr(), mesh.shape[0],
                                              float(ob.delta), k, M, stats.data_ptr(), wst.data_ptr(), ws.data_ptr(), wsb, _lib.stream_ptr())
    torch.cuda.synchronize()
    if rc:
        return rc, lib.asvgp_last_error_string().decode()
    st = stats.cpu().numpy()
    return st[:(k + 1) * M].reshape(k + 1, M), st[(k + 1) * M:-1].reshape(M, D), float(st[-1]), wst.cpu().numpy(), h.phi_last_algorithm()


def check_stats(tag, got, ref):
    band, rhs, yy, wst = got
    rband, rrhs, ryy, (sw, lam, npos) = ref
    assert report(tag + " A_w", np.max(np.abs(band - rband)), max(np.max(np.abs(rband)), 1e-300)) <= 1e-12
    assert report(tag + " b_w", np.max(np.abs(rhs - rrhs)), max(np.max(np.abs(rrhs)), 1e-300)) <= 1e-12
    assert report(tag + " yy_w", abs(yy - ryy), max(abs(ryy), 1e-300)) <= 1e-12
    assert report(tag + " sum w", abs(wst[0] - sw), max(abs(sw), 1e-300)) <= 1e-12
    assert wst[2] == npos


def check_lambda(tag, got_lam, w):
    pos = w[w > 0]
    scale = max(float(np.sum(np.abs(np.log(pos)))), 1e-300)
    assert report(tag + " sum log w", abs(got_lam - float(np.sum(np.log(pos)))), scale) <= 1e-12


# ------------------------------------------------------------------------------------------------ 1. statistics
# (order, M, N, D, float32-linspace mesh?, layout, weights, unaligned slices?)
STAT_CASES = [
    (1, 8, 1, 1, False, "unsorted", "integer", False),
    (2, 8, 777, 3, True, "sorted", "decades", True),
    (3, 100, 30_000, 1, True, "unsorted", "decades", False),
    (4, 2048, 300_000, 1, False, "unsorted", "decades", False),
    (4, 2048, 300_000, 1, False, "sorted", "decades", False),
    (4, 257, 100_001, 3, True, "clustered", "integer", True),
    (5, 5000, 200_000, 1, False, "unsorted", "decades", True),
    (6, 5000, 50_000, 3, True, "clustered", "decades", False),
    (6, 40, 4099, 1, False, "sorted", "integer", True),
    (1, 8, 2, 1, False, "unsorted", "integer", False),
    (1, 700, 20_001, 1, False, "clustered", "decades", False),
    (2, 2048, 150_000, 1, False, "unsorted", "integer", False),
    (3, 100, 30_000, 1, False, "sorted", "decades", False),
    (4, 12, 5000, 1, False, "unsorted", "decades", False),
    (4, 2048, 300_001, 1, False, "clustered", "decades", False),
    (5, 1024, 200_000, 1, False, "unsorted", "decades", False),
    (6, 2048, 100_000, 1, False, "sorted", "integer", False),
    (6, 40, 4099, 1, False, "clustered", "decades", False),
]


@pytest.mark.parametrize("order,M,N,D,f32mesh,layout,wkind,unaligned", STAT_CASES)
def test_weighted_statistics_1d(A, order, M, N, D, f32mesh, layout, wkind, unaligned):
    rng = np.random.default_rng(1000 * order + M + N)
    a, b = (0.0, 1.0) if f32mesh else (0, 1)
    ob = O.Basis(order, a, b, M)
    x = make_x(rng, N, 0.0, 1.0, layout)
    y = np.stack([np.sin(9 * (d + 1) * x) for d in range(D)], 1) + 0.3 * rng.normal(size=(N, D))
    w = make_weights(rng, N, wkind)
    if N == 1:
        w[:] = 2.0
    off = 1 if unaligned else 0               # slices that start 8 bytes into a 16-byte aligned allocation
    xb, yb, wb = (torch.zeros(n + off, dtype=torch.float64, device="cuda") for n in (N, N * D, N))
    xb[off:], yb[off:], wb[off:] = dev(x), dev(y.reshape(-1)), dev(w)
    xt, yt, wt = xb[off:], yb[off:], wb[off:]
    if unaligned:
        assert xt.data_ptr() % 16 == 8
    got = run_weighted_1d(A, ob, xt, yt, wt, D)
    assert got[4] == expected_algorithm(N, M, D, f32mesh, unaligned)
    tag = "1-D k=%d M=%d N=%d D=%d %s %s%s" % (order, M, N, D, layout, wkind, " unaligned" if unaligned else "")
    ref = weighted_stats_1d(ob, x, y, w)
    check_stats(tag + " (kernel %d)" % got[4], got[:4], ref)
    check_lambda(tag, got[3][1], w)
    # algorithm 1 forces the general kernel, whatever the shape; algorithm 6 the register-moment kernel where it applies (else refused)
    again = run_weighted_1d(A, ob, xt, yt, wt, D, algo=1)
    assert again[4] == WEIGHTED_BAND_SCATTER
    check_stats(tag + " (kernel 11 forced)", again[:4], ref)
    check_lambda(tag + " (kernel 11 forced)", again[3][1], w)
    forced = run_weighted_1d(A, ob, xt, yt, wt, D, algo=6)
    if got[4] == WEIGHTED_MOMENTS:
        assert forced[4] == WEIGHTED_MOMENTS
    else:
        assert forced[0] == -2 and "register moments" in forced[1]


def test_weighted_statistics_1d_headline_shape(A):
    """N = 10M, M = 2048, k = 4, D = 1, weights log-uniform over 12 decades with a third of them 0; and N = 0."""
    rng = np.random.default_rng(10)
    N, M = 10_000_000, 2048
    ob = O.Basis(4, 0, 1, M)
    x = make_x(rng, N, 0.0, 1.0, "unsorted")
    y = np.sin(20 * x) + 0.1 * rng.normal(size=N)
    w = make_weights(rng, N, "decades")
    ref = weighted_stats_1d(ob, x, y, w)
    for algo, kernel in ((0, WEIGHTED_MOMENTS), (1, WEIGHTED_BAND_SCATTER)):
        got = run_weighted_1d(A, ob, dev(x), dev(y), dev(w), 1, algo=algo)
        assert got[4] == kernel
        check_stats("1-D headline N=10M M=2048 (kernel %d)" % kernel, got[:4], ref)
        check_lambda("1-D headline N=10M M=2048 (kernel %d)" % kernel, got[3][1], w)
    xs = np.sort(x)
    got = run_weighted_1d(A, ob, dev(xs), dev(y), dev(w), 1)
    assert got[4] == WEIGHTED_MOMENTS
    check_stats("1-D headline N=10M M=2048 sorted (kernel 16)", got[:4], weighted_stats_1d(ob, xs, y, w))
    e = torch.zeros(2, dtype=torch.float64, device="cuda")
    got0 = run_weighted_1d(A, ob, e[:0], e[:0], e[:0], 1)
    assert not got0[0].any() and not got0[1].any() and got0[2] == 0.0 and not got0[3].any()


KRON_STAT_CASES = [(2, 9, 7, 400, "integer"), (3, 20, 24, 5000, "decades"), (4, 14, 16, 3000, "decades"), (3, 128, 128, 200_000, "decades"),
                   (4, 128, 100, 100_000, "integer")]


@pytest.mark.parametrize("order,m1,m2,N,wkind", KRON_STAT_CASES)
def test_weighted_statistics_kron(A, order, m1, m2, N, wkind):
    """Both weighted Kronecker entries against the direct accumulation (scipy sparse Khatri-Rao rows, fp64)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(m1 * 131 + m2)
    X = np.stack([rng.uniform(0.001, 0.999, N), rng.uniform(-0.999, 1.999, N)], axis=1)
    y = np.sin(12 * X[:, :1]) * np.cos(3 * X[:, 1:]) + 0.1 * rng.normal(size=(N, 1))
    w = make_weights(rng, N, wkind)
    B = getattr(A, "B%dSpline" % order)
    bases = [B(0, 1, m1), B(-1, 2, m2)]
    obases = [O.Basis(order, 0, 1, m1), O.Basis(order, -1, 2, m2)]
    Kuf = O.make_kvs_sparse([bs.evaluate_basis(X[:, i:i + 1]) for i, bs in enumerate(obases)]).tocsr()
    Aw = sparse_to_blockband(Kuf @ sp.diags(w) @ Kuf.T, order, m1, m2)
    bw = np.asarray(Kuf @ (w[:, None] * y))
    yy = float(np.sum(w[:, None] * y * y))
    pos = w > 0
    model = A.GPR_kron((X, y), [A.Matern32(), A.Matern32()], bases, weights=w)
    for name, sorted_cells in (("cell-sorted", True), ("per point", False)):
        model._stats.fill_(7.0)
        model._wstats.fill_(7.0)
        model._phi_pass_local(sorted_cells=sorted_cells)
        tag = "kron %s k=%d %dx%d N=%d %s" % (name, order, m1, m2, N, wkind)
        assert report(tag + " A_w", np.max(np.abs(model.KufKfu_blockband.cpu().numpy() - Aw)), np.max(np.abs(Aw))) <= 1e-12
        assert report(tag + " b_w", np.max(np.abs(model.Kuf_y.cpu().numpy() - bw)), np.max(np.abs(bw))) <= 1e-12
        assert report(tag + " yy_w", abs(model.tr_yTy.item() - yy), yy) <= 1e-12
        wst = model._wstats.cpu().numpy()
        assert report(tag + " sum w", abs(wst[0] - w.sum()), w.sum()) <= 1e-12
        check_lambda(tag, wst[1], w)
        assert wst[2] == pos.sum() == model.num_data


# ------------------------------------------------------------------------------------------------ 2. replication identity
def _predictions_match(tag, mw, mr, X):
    """predict_f_device, predict_f_cov_device, predict_f_gradient_device of two models that must be the same posterior, at the tolerances
    of those methods' own tests (1e-8 absolute on mean / variance / covariance; gradient mean 1e-9 of its scale, variance 1e-8 of the prior)."""
    m1, v1 = mw.predict_f_device(X)
    m2, v2 = mr.predict_f_device(X)
    assert report(tag + " predict_f mean", (m1 - m2).abs().max().item(), 1.0) <= 1e-8
    assert report(tag + " predict_f var", (v1 - v2).abs().max().item(), 1.0) <= 1e-8
    c1, c2 = mw.predict_f_cov_device(X), mr.predict_f_cov_device(X)
    assert report(tag + " predict_f_cov", (c1 - c2).abs().max().item(), 1.0) <= 1e-8
    g1, g2 = mw.predict_f_gradient_device(X), mr.predict_f_gradient_device(X)
    assert report(tag + " gradient mean", (g1[0] - g2[0]).abs().max().item(), max(g2[0].abs().max().item(), 1e-300)) <= 1e-9
    assert report(tag + " gradient var", (g1[1] - g2[1]).abs().max().item(), max(g2[1].abs().max().item(), 1e-300)) <= 1e-8


@pytest.mark.parametrize("order,kind,M,D", [(4, "Matern32", 64, 1), (3, "Matern52", 30, 2), (5, "Matern32", 200, 1)])
def test_replication_identity_1d(A, order, kind, M, D):
    rng = np.random.default_rng(5 + order)
    N, v, l, s = 4000, 1.3, 0.2, 0.05
    x = rng.uniform(1e-6, 1 - 1e-6, N)
    y = np.stack([np.sin(7 * (d + 1) * x) for d in range(D)], 1) + 0.2 * rng.normal(size=(N, D))
    r = rng.integers(0, 4, N)
    xr, yr = np.repeat(x, r), np.repeat(y, r, axis=0)
    B = getattr(A, "B%dSpline" % order)
    mw = A.GPR_1d((x.reshape(-1, 1), y), getattr(A, kind)(variance=v, lengthscales=l), B(0, 1, M), weights=r)
    mr = A.GPR_1d((xr.reshape(-1, 1), yr), getattr(A, kind)(variance=v, lengthscales=l), B(0, 1, M))
    assert mw._h.phi_last_algorithm() == (WEIGHTED_MOMENTS if D == 1 else WEIGHTED_BAND_SCATTER) and mr._h.phi_last_algorithm() in (1, 3, 5, 6)
    for m in (mw, mr):
        m.likelihood.variance.assign(s)
    tag = "replication 1-D k=%d %s M=%d D=%d" % (order, kind, M, D)
    for name, a, b in (("A", mw.KufKfu, mr.KufKfu), ("b", mw.Kuf_y, mr.Kuf_y), ("yy", mw.tr_yTy, mr.tr_yTy)):
        assert report(tag + " " + name, (a - b).abs().max().item(), b.abs().max().item()) <= 1e-12
    sw, npos, lam = float(r.sum()), int((r > 0).sum()), float(np.log(r[r > 0]).sum())
    assert mw.num_data == npos and mr.num_data == r.sum()
    assert abs(mw.weight_sum - sw) <= 1e-12 * sw and abs(mw.log_weight_sum - lam) <= 1e-12 * np.abs(np.log(r[r > 0])).sum()
    ew, er = mw.elbo().item(), mr.elbo().item()
    want = 0.5 * D * (sw - npos) * np.log(2 * np.pi * s) + 0.5 * D * lam
    assert report(tag + " ELBO_w - ELBO_rep", abs((ew - er) - want), abs(er)) <= 1e-9
    _predictions_match(tag, mw, mr, dev(np.linspace(0.01, 0.99, 50)))


def _blocks_match_kron(tag, mw, mr):
    """A (block band), b and yy of two Kronecker models, each to 1e-12 of ITS OWN largest entry"""
    for name, a, b in (("A", mw.KufKfu_blockband, mr.KufKfu_blockband), ("b", mw.Kuf_y, mr.Kuf_y), ("yy", mw.tr_yTy, mr.tr_yTy)):
        assert report(tag + " statistics " + name, (a - b).abs().max().item(), b.abs().max().item()) <= 1e-12


def test_replication_identity_kron(A):
    rng = np.random.default_rng(21)
    N, s, order, m1, m2 = 3000, 0.05, 3, 12, 14
    X = np.stack([rng.uniform(0.001, 0.999, N), rng.uniform(-0.999, 1.999, N)], axis=1)
    y = np.sin(6 * X[:, :1]) * np.cos(3 * X[:, 1:]) + 0.1 * rng.normal(size=(N, 1))
    r = rng.integers(0, 4, N)
    mk = lambda: [A.Matern32(variance=1.1, lengthscales=0.3), A.Matern52(variance=0.7, lengthscales=0.6)]
    bases = lambda: [A.B3Spline(0, 1, m1), A.B3Spline(-1, 2, m2)]
    mw = A.GPR_kron((X, y), mk(), bases(), weights=r.reshape(-1, 1))
    mr = A.GPR_kron((np.repeat(X, r, axis=0), np.repeat(y, r, axis=0)), mk(), bases())
    for m in (mw, mr):
        m.likelihood.variance.assign(s)
    tag = "replication kron 12x14"
    _blocks_match_kron(tag, mw, mr)
    sw, npos, lam = float(r.sum()), int((r > 0).sum()), float(np.log(r[r > 0]).sum())
    assert mw.num_data == npos
    ew, er = float(mw.elbo()), float(mr.elbo())
    want = 0.5 * (sw - npos) * np.log(2 * np.pi * s) + 0.5 * lam
    assert report(tag + " ELBO_w - ELBO_rep", abs((ew - er) - want), abs(er)) <= 1e-9
    e2, _ = mw.elbo_and_grad()
    assert abs(e2 - ew) <= 1e-9 * abs(ew)
    Xs = dev(np.stack([rng.uniform(0.01, 0.99, 40), rng.uniform(-0.99, 1.99, 40)], axis=1))
    _predictions_match(tag, mw, mr, Xs)


# ------------------------------------------------------------------------------------------------ 3. scale identity
@pytest.mark.parametrize("c", [0.25, 7.5])
def test_scale_identity(A, c):
    """w = c everywhere is the unweighted model at noise variance sigma2 / c."""
    rng = np.random.default_rng(3)
    N, M, v, l, s = 20_000, 128, 0.9, 0.1, 0.04
    x = rng.uniform(1e-6, 1 - 1e-6, N)
    y = (np.sin(20 * x) + 0.2 * rng.normal(size=N)).reshape(-1, 1)
    mw = A.GPR_1d((x.reshape(-1, 1), y), A.Matern32(variance=v, lengthscales=l), A.B4Spline(0, 1, M), weights=np.full(N, c))
    mu = A.GPR_1d((x.reshape(-1, 1), y), A.Matern32(variance=v, lengthscales=l), A.B4Spline(0, 1, M))
    mw.likelihood.variance.assign(s)
    mu.likelihood.variance.assign(s / c)
    gw, gu = mw.elbo_and_grad().cpu().numpy(), mu.elbo_and_grad().cpu().numpy()
    # log N(y | 0, Q + (s/c) I) is the same density: the weighted bound carries its 1/2 N log c in the N+ / Lambda terms
    tag = "scale identity c=%g" % c
    assert report(tag + " ELBO", abs(gw[0] - gu[0]), abs(gu[0])) <= 1e-9
    assert report(tag + " d/dv", abs(gw[1] - gu[1]), abs(gu[1])) <= 1e-6
    assert report(tag + " d/dl", abs(gw[2] - gu[2]), abs(gu[2])) <= 1e-6
    assert report(tag + " d/ds", abs(gw[3] - gu[3] / c), abs(gu[3] / c)) <= 1e-6


# ------------------------------------------------------------------------------------------------ 4. general weights
@pytest.mark.parametrize("order,kind,kname,M,N,l", [(4, 1, "Matern32", 40, 400, 0.2), (3, 2, "Matern52", 30, 3000, 0.3), (2, 0, "Matern12", 25, 2000, 0.2),
                                                    (4, 1, "Matern32", 1024, 100_000, 0.02), (5, 2, "Matern52", 200, 50_000, 0.1)])
def test_general_weights_against_long_double_oracle(A, order, kind, kname, M, N, l):
    rng = np.random.default_rng(40 + M)
    v, s = 1.2, 0.03
    x = rng.uniform(1e-6, 1 - 1e-6, N)
    y = (np.sin(15 * x) + 0.2 * rng.normal(size=N)).reshape(-1, 1)
    w = make_weights(rng, N, "lognormal")
    w[rng.random(N) < 1 / 7] = 0.0
    model = A.GPR_1d((x.reshape(-1, 1), y), getattr(A, kname)(variance=v, lengthscales=l), getattr(A, "B%dSpline" % order)(0, 1, M), weights=w)
    model.likelihood.variance.assign(s)
    ob = O.Basis(order, 0, 1, M)
    band, rhs, yy, ws = weighted_stats_1d(ob, x, y, w)
    oe, og = weighted_oracle_1d(ob, kind, band, rhs, yy, ws, v, l, s)
    tag = "general weights k=%d %s M=%d N=%d" % (order, kname, M, N)
    got = np.array(model.elbo_and_grad().tolist())
    host = np.array(model.elbo_and_grad_host())
    for name, g in (("elbo_and_grad", got), ("elbo_and_grad_host", host)):
        assert report(tag + " %s ELBO" % name, abs(g[0] - oe), abs(oe)) <= 1e-9
        assert report(tag + " %s gradient" % name, np.max(np.abs(g[1:4] - og) / np.abs(og)), 1.0) <= 1e-6
    assert report(tag + " elbo()", abs(model.elbo().item() - oe), abs(oe)) <= 1e-9
    assert abs(model.training_loss().item() + model.maximum_log_likelihood_objective().item()) <= 1e-12 * abs(oe)
    if order == 4:                              # (the fused matrix-core launch: where today's tests assert these agreements)
        _launch_paths_agree(tag, model, got, host, must_apply=(M == 1024))
    # the split launch reads the same scalars
    model.launch_prior_chain()
    split = model.launch_data_chain()[:4].cpu().numpy()
    assert report(tag + " data chain ELBO", abs(split[0] - oe), abs(oe)) <= 1e-9


def _launch_paths_agree(tag, model, dev_r, host_r, must_apply):
    """The launch paths of a weighted model agree with each other exactly as tests/test_gpu_parity.py asserts for an unweighted one:
    the host-read results (one-call step, result mirror) equal elbo_and_grad bit for bit
    (test_host_result_mirror_gives_the_stream_path_numbers), the launch-ahead pair equals launch_elbo_host to rtol 1e-12
    (test_launch_ahead_of_theta_gives_the_ordinary_launch_numbers).  Returns the launch-ahead result (None where that launch does not apply)."""
    dev_r, host_r = [float(v) for v in dev_r], [float(v) for v in host_r]
    report(tag + " elbo_and_grad_host vs elbo_and_grad (must be 0)", np.max(np.abs(np.array(host_r) - np.array(dev_r))), 1.0)
    assert host_r == dev_r
    mirror = model.read_elbo_host(model.launch_elbo_host())
    assert mirror == dev_r
    tok = model.launch_elbo_ahead()
    if tok is None:
        assert not must_apply, "the launch-ahead path applies at k = 4, D = 1, 1024 <= M <= 2048"
        return None
    model.publish_theta()
    ahead = model.read_elbo_host(tok)
    report(tag + " launch-ahead vs launch_elbo_host", np.max(np.abs(np.array(ahead) - np.array(mirror)) / np.abs(np.array(mirror))), 1.0)
    np.testing.assert_allclose(ahead, mirror, rtol=1e-12)
    return ahead


def test_general_weights_headline_shape_all_launch_paths(A):
    """N = 10M, M = 2048, k = 4, theta = (1, 0.05, 0.01), log-normal weights: elbo_and_grad, elbo_and_grad_host and the launch-ahead pair
    against the long-double oracle, and against each other."""
    rng = np.random.default_rng(77)
    N, M, v, l, s = 10_000_000, 2048, 1.0, 0.05, 0.01
    x = rng.uniform(1e-9, 1 - 1e-9, N)
    y = (np.sin(20 * x) + 0.1 * rng.normal(size=N)).reshape(-1, 1)
    w = make_weights(rng, N, "lognormal")
    model = A.GPR_1d((x.reshape(-1, 1), y), A.Matern32(variance=v, lengthscales=l), A.B4Spline(0, 1, M), weights=w)
    model.likelihood.variance.assign(s)
    ob = O.Basis(4, 0, 1, M)
    band, rhs, yy, ws = weighted_stats_1d(ob, x, y, w)
    oe, og = weighted_oracle_1d(ob, 1, band, rhs, yy, ws, v, l, s)
    dev_r = model.elbo_and_grad().tolist()
    host_r = model.elbo_and_grad_host()
    ahead = _launch_paths_agree("headline weighted", model, dev_r, host_r, must_apply=True)
    for name, g in (("elbo_and_grad", dev_r), ("elbo_and_grad_host", host_r), ("launch-ahead", ahead)):
        g = np.asarray(g)
        assert report("headline weighted %s ELBO" % name, abs(g[0] - oe), abs(oe)) <= 1e-9
        assert report("headline weighted %s gradient" % name, np.max(np.abs(g[1:4] - og) / np.abs(og)), 1.0) <= 1e-6


@pytest.mark.parametrize("order,m1,m2,N", [(3, 8, 9, 300), (4, 14, 16, 2000), (2, 10, 7, 500)])
def test_general_weights_kron_against_dense_numpy(A, order, m1, m2, N):
    rng = np.random.default_rng(m1 * 100 + m2 + 1)
    X = np.stack([rng.uniform(0.001, 0.999, N), rng.uniform(-0.999, 1.999, N)], axis=1)
    y = np.sin(12 * X[:, :1]) * np.cos(3 * X[:, 1:]) + 0.1 * rng.normal(size=(N, 1))
    w = make_weights(rng, N, "lognormal")
    w[rng.random(N) < 1 / 7] = 0.0
    B = getattr(A, "B%dSpline" % order)
    th, s = [(1.1, 0.3), (0.7, 0.6)], 0.05
    kerns = [A.Matern32(variance=th[0][0], lengthscales=th[0][1]), A.Matern32(variance=th[1][0], lengthscales=th[1][1])]
    model = A.GPR_kron((X, y), kerns, [B(0, 1, m1), B(-1, 2, m2)], weights=w)
    model.likelihood.variance.assign(s)
    obases = [O.Basis(order, 0, 1, m1), O.Basis(order, -1, 2, m2)]
    oe, Aw, bw, yy, (sw, lam, npos) = weighted_kron_dense(obases, [1, 1], th, s, X, y, w)
    tag = "general weights kron k=%d %dx%d" % (order, m1, m2)
    e = float(model.elbo())
    tol = elbo_tol(oe, max(sw, npos), th[0][0] * th[1][0], s, yy, bcr=True)
    report(tag + " ELBO (over its tolerance)", abs(e - oe), tol)
    assert abs(e - oe) <= tol
    e2, g = model.elbo_and_grad()
    assert abs(e2 - oe) <= tol
    # gradient: central differences of the model's own elbo in the constrained parameters
    params = model.trainable_parameters
    for i, p in enumerate(params):
        x0 = float(p)
        h = 1e-5 * x0
        p.assign(x0 + h); ep = float(model.elbo())
        p.assign(x0 - h); em = float(model.elbo())
        p.assign(x0)
        fd = (ep - em) / (2 * h)
        assert report(tag + " d/dtheta[%d] vs central differences" % i, abs(g[i] - fd), abs(fd)) <= 1e-5


# ------------------------------------------------------------------------------------------------ 5. masking
def test_masking_1d(A):
    rng = np.random.default_rng(8)
    N, M, v, l, s = 30_000, 256, 1.0, 0.05, 0.02
    x = rng.uniform(1e-6, 1 - 1e-6, N)
    y = (np.sin(20 * x) + 0.1 * rng.normal(size=N)).reshape(-1, 1)
    keep = rng.random(N) >= 1 / 3
    mw = A.GPR_1d((x.reshape(-1, 1), y), A.Matern32(variance=v, lengthscales=l), A.B4Spline(0, 1, M), weights=keep.astype(np.float64))
    mk = A.GPR_1d((x[keep].reshape(-1, 1), y[keep]), A.Matern32(variance=v, lengthscales=l), A.B4Spline(0, 1, M))
    for m in (mw, mk):
        m.likelihood.variance.assign(s)
    assert mw.num_data == mk.num_data == int(keep.sum())
    assert mw.weight_sum == float(keep.sum()) and mw.log_weight_sum == 0.0
    sw, sk = mw._stats.cpu().numpy(), mk._stats.cpu().numpy()
    k1 = 5 * M
    for name, sl in (("A", slice(0, k1)), ("b", slice(k1, k1 + M)), ("yy", slice(k1 + M, None))):
        assert report("masking 1-D " + name, np.max(np.abs(sw[sl] - sk[sl])), np.max(np.abs(sk[sl]))) <= 1e-12
    ew, ek = mw.elbo_and_grad().cpu().numpy(), mk.elbo_and_grad().cpu().numpy()
    assert report("masking 1-D ELBO", abs(ew[0] - ek[0]), abs(ek[0])) <= 1e-9
    assert report("masking 1-D gradient", np.max(np.abs(ew[1:] - ek[1:]) / np.abs(ek[1:])), 1.0) <= 1e-6
    _predictions_match("masking 1-D", mw, mk, dev(np.linspace(0.01, 0.99, 64)))


def test_masking_kron(A):
    rng = np.random.default_rng(9)
    N, s = 6000, 0.05
    X = rng.uniform(0.001, 0.999, (N, 2))
    y = np.sin(5 * X[:, :1]) + X[:, 1:] ** 2 + 0.1 * rng.normal(size=(N, 1))
    keep = rng.random(N) >= 1 / 3
    mk_ = lambda: ([A.Matern32(variance=1.2, lengthscales=0.4), A.Matern32(variance=0.8, lengthscales=0.5)], [A.B3Spline(0, 1, 11), A.B3Spline(0, 1, 10)])
    mw = A.GPR_kron((X, y), *mk_(), weights=keep.astype(np.float64))
    mk = A.GPR_kron((X[keep], y[keep]), *mk_())
    for m in (mw, mk):
        m.likelihood.variance.assign(s)
    assert mw.num_data == mk.num_data == int(keep.sum())
    _blocks_match_kron("masking kron", mw, mk)
    ew, ek = float(mw.elbo()), float(mk.elbo())
    assert report("masking kron ELBO", abs(ew - ek), abs(ek)) <= 1e-9
    Xs = dev(rng.uniform(0.01, 0.99, (50, 2)))
    _predictions_match("masking kron", mw, mk, Xs)


# ------------------------------------------------------------------------------------------------ 6. w = 1 / None
def test_unit_weights_equal_no_weights(A):
    rng = np.random.default_rng(6)
    N, M = 50_000, 512
    x = rng.uniform(1e-6, 1 - 1e-6, N)
    y = (np.sin(20 * x) + 0.1 * rng.normal(size=N)).reshape(-1, 1)
    mk = lambda **kw: A.GPR_1d((x.reshape(-1, 1), y), A.Matern32(variance=1.0, lengthscales=0.05), A.B4Spline(0, 1, M), **kw)
    m1, m0 = mk(weights=torch.ones(N)), mk(weights=None)
    assert m0.weights is None and m0.weight_sum is None and m0.num_data == N
    assert m0._h.phi_last_algorithm() in (1, 3, 5, 6) and m1._h.phi_last_algorithm() == WEIGHTED_MOMENTS
    assert m1.weights.is_cuda and m1.weights.dtype == torch.float64 and m1.num_data == N and m1.weight_sum == N and m1.log_weight_sum == 0.0
    for m in (m1, m0):
        m.likelihood.variance.assign(0.01)
    for name, a, b in (("A", m1.KufKfu, m0.KufKfu), ("b", m1.Kuf_y, m0.Kuf_y), ("yy", m1.tr_yTy, m0.tr_yTy)):
        assert report("w = 1 statistics " + name, (a - b).abs().max().item(), b.abs().max().item()) <= 1e-12
    e1, e0 = m1.elbo_and_grad().cpu().numpy(), m0.elbo_and_grad().cpu().numpy()
    assert report("w = 1 ELBO", abs(e1[0] - e0[0]), abs(e0[0])) <= 1e-9
    X2 = rng.uniform(0.001, 0.999, (4000, 2))
    y2 = np.sin(5 * X2[:, :1]) + X2[:, 1:] ** 2 + 0.1 * rng.normal(size=(4000, 1))
    kk = lambda **kw: A.GPR_kron((X2, y2), [A.Matern32(), A.Matern32()], [A.B3Spline(0, 1, 11), A.B3Spline(0, 1, 10)], **kw)
    k1, k0 = kk(weights=np.ones((4000, 1))), kk()
    _blocks_match_kron("w = 1 kron", k1, k0)
    assert report("w = 1 kron ELBO", abs(float(k1.elbo()) - float(k0.elbo())), abs(float(k0.elbo()))) <= 1e-9


# ------------------------------------------------------------------------------------------------ 7. predict_y / predict_log_density
def test_predict_y_and_log_density_with_weights(A):
    rng = np.random.default_rng(12)
    N, D = 3000, 2
    x = rng.uniform(1e-6, 1 - 1e-6, N)
    y = np.stack([np.sin(7 * x), np.cos(5 * x)], 1) + 0.1 * rng.normal(size=(N, D))
    model = A.GPR_1d((x.reshape(-1, 1), y), A.Matern32(variance=1.0, lengthscales=0.2), A.B4Spline(0, 1, 40), weights=make_weights(rng, N, "lognormal"))
    model.likelihood.variance.assign(0.02)
    Xn = rng.uniform(0.01, 0.99, (200, 1))
    Yn = np.stack([np.sin(7 * Xn[:, 0]), np.cos(5 * Xn[:, 0])], 1)
    wn = np.exp(rng.normal(size=200))
    mean, var = model.predict_f(Xn)
    for wts, noise in ((None, 0.02), (wn, 0.02 / wn.reshape(-1, 1)), (torch.from_numpy(wn).cuda(), 0.02 / wn.reshape(-1, 1))):
        my, vy = model.predict_y(Xn, weights=wts) if wts is not None else model.predict_y(Xn)
        assert report("predict_y mean", np.max(np.abs(my - mean)), 1.0) == 0.0
        assert report("predict_y var", np.max(np.abs(vy - (var + noise))), 1.0) <= 1e-15
        ld = model.predict_log_density((Xn, Yn), weights=wts) if wts is not None else model.predict_log_density((Xn, Yn))
        ref = np.sum(-0.5 * (np.log(2 * np.pi * (var + noise)) + (Yn - mean) ** 2 / (var + noise)), axis=-1)
        assert ld.shape == (200,)
        assert report("predict_log_density", np.max(np.abs(ld - ref)), np.max(np.abs(ref))) <= 1e-14
    with pytest.raises(ValueError):
        model.predict_y(Xn, weights=np.zeros(200))
    with pytest.raises(ValueError):
        model.predict_y(Xn, weights=np.ones(3))


# ------------------------------------------------------------------------------------------------ 8. loud failures
def test_loud_failures(A):
    from asvgp_amd import _lib
    rng = np.random.default_rng(1)
    N = 5000
    x = rng.uniform(1e-6, 1 - 1e-6, N)
    y = np.sin(9 * x).reshape(-1, 1)
    mk = lambda w: A.GPR_1d((x.reshape(-1, 1), y), A.Matern32(), A.B4Spline(0, 1, 40), weights=w)
    for bad in (-1.0, np.nan, np.inf, -np.inf):
        w = np.ones(N)
        w[1234] = bad
        with pytest.raises(ValueError, match="row 1234"):
            mk(w)
        X2 = np.stack([x, x[::-1]], 1)
        with pytest.raises(ValueError, match="row 1234"):
            A.GPR_kron((X2, y), [A.Matern32(), A.Matern32()], [A.B3Spline(0, 1, 10), A.B3Spline(0, 1, 11)], weights=w)
        # through the C-ABI directly: yy_w = NaN, nothing silently dropped
        ob = O.Basis(4, 0, 1, 40)
        for algo, kernel in ((0, WEIGHTED_MOMENTS), (1, WEIGHTED_BAND_SCATTER)):
            got = run_weighted_1d(A, ob, dev(x), dev(y), dev(w), 1, algo=algo)
            assert got[4] == kernel and np.isnan(got[2])
        y3 = np.concatenate([y, 2 * y, -y], 1)                     # D = 3: the general kernel's per-column launches
        got = run_weighted_1d(A, ob, dev(x), dev(y3.reshape(-1)), dev(w), 3)
        assert got[4] == WEIGHTED_BAND_SCATTER and np.isnan(got[2])
        km = A.GPR_kron((X2, y), [A.Matern32(), A.Matern32()], [A.B3Spline(0, 1, 10), A.B3Spline(0, 1, 11)], weights=np.ones(N))
        km.weights[1234] = bad
        km._sorted = None
        for sorted_cells in (True, False):
            km._phi_pass_local(sorted_cells=sorted_cells)
            assert torch.isnan(km.tr_yTy).item()
    with pytest.raises(ValueError, match="shape"):
        mk(np.ones(N - 1))
    # a row with w = 0 may hold any finite y
    w = np.ones(N)
    w[7] = 0.0
    y_big = y.copy()
    y_big[7] = 1e300
    m = A.GPR_1d((x.reshape(-1, 1), y_big), A.Matern32(), A.B4Spline(0, 1, 40), weights=w)
    assert np.isfinite(m._stats.cpu().numpy()).all() and m.num_data == N - 1
    # the fixed-point algorithms have no weighted form
    ob = O.Basis(4, 0, 1, 40)
    for algo in (3, 5):
        rc, msg = run_weighted_1d(A, ob, dev(x), dev(y), dev(np.ones(N)), 1, algo=algo)
        assert rc == -2 and "fixed point" in msg                      # ASVGP_ERR_UNSUPPORTED
    # the models that have no weighted Phi pass refuse before anything is launched
    X3 = rng.uniform(0.01, 0.99, (100, 3))
    with pytest.raises(NotImplementedError, match="d = 2"):
        A.GPR_kron((X3, y[:100]), [A.Matern32()] * 3, [A.B3Spline(0, 1, 10)] * 3, weights=np.ones(100))
    with pytest.raises(NotImplementedError, match="GPR_additive"):
        A.GPR_additive((X3[:, :2], y[:100]), [A.Matern32(), A.Matern32()], [A.B3Spline(0, 1, 10), A.B3Spline(0, 1, 11)], weights=np.ones(100))
    # asvgp_set_weight_sums checks its arguments on the host
    h = _lib.Handle()
    lib = _lib.get_lib()
    assert lib.asvgp_set_weight_sums(h.ptr, 10.5, 10.0, 0.0) == -1 and lib.asvgp_set_weight_sums(h.ptr, 10.0, -1.0, 0.0) == -1
    assert lib.asvgp_set_weight_sums(h.ptr, 10.0, 12.0, float("nan")) == -1
    assert lib.asvgp_set_weight_sums(h.ptr, 10.0, 12.0, 0.5) == 0 and lib.asvgp_set_weight_sums(h.ptr, -1.0, 0.0, 0.0) == 0


# ------------------------------------------------------------------------------------------------ 9. two ranks on one GPU over gloo
def _weighted_problem():
    rng = np.random.default_rng(2025)
    N, M = 120_001, 256
    x = rng.uniform(1e-9, 1 - 1e-9, N)
    y = (np.sin(20 * x) + 0.1 * rng.normal(size=N)).reshape(-1, 1)
    w = make_weights(rng, N, "decades")
    N2 = 6001
    X2 = rng.uniform(0.001, 0.999, (N2, 2))
    y2 = np.sin(5 * X2[:, :1]) + X2[:, 1:] ** 2 + 0.1 * rng.normal(size=(N2, 1))
    w2 = make_weights(rng, N2, "integer")
    return N, M, x, y, w, X2, y2, w2


def _build_weighted(A, x, y, w, M, X2, y2, w2, pg=None):
    kw = dict(process_group=pg) if pg is not None else {}
    m = A.GPR_1d((x.reshape(-1, 1), y), A.Matern32(variance=1.0, lengthscales=0.05), A.B4Spline(0, 1, M), weights=w, **kw)
    m.likelihood.variance.assign(0.01)
    mk = A.GPR_kron((X2, y2), [A.Matern32(), A.Matern32()], [A.B3Spline(0, 1, 11), A.B3Spline(0, 1, 10)], weights=w2, **kw)
    return m, mk


def _weighted_shard_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)                       # both ranks share the one GPU of the test box; gloo moves the band
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import asvgp_amd as A
    from asvgp_amd.dist import shard_bounds
    N, M, x, y, w, X2, y2, w2 = _weighted_problem()
    lo, hi = shard_bounds(N, world, rank)
    lo2, hi2 = shard_bounds(X2.shape[0], world, rank)
    m, mk = _build_weighted(A, x[lo:hi], y[lo:hi], w[lo:hi], M, X2[lo2:hi2], y2[lo2:hi2], w2[lo2:hi2], pg=dist.group.WORLD)
    r = m.elbo_and_grad().cpu().numpy()
    m.phi_pass()                                   # (re-running the pass all-reduces again; the weight sums stay the global ones)
    r_again = m.elbo_and_grad().cpu().numpy()
    assert np.allclose(r_again, r, rtol=1e-9, atol=0), (r_again, r)
    q.put((rank, (m.num_data, m.weight_sum, m.log_weight_sum), m._stats.cpu().numpy(), r,
           (mk.num_data, mk.weight_sum, mk.log_weight_sum, float(mk.elbo()))))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharded_weighted_model_matches_single_rank(A):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31600 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_weighted_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    N, M, x, y, w, X2, y2, w2 = _weighted_problem()
    single, sk = _build_weighted(A, x, y, w, M, X2, y2, w2)
    r1 = single.elbo_and_grad().cpu().numpy()
    s1 = single._stats.cpu().numpy()
    ek = float(sk.elbo())
    lscale = float(np.sum(np.abs(np.log(w[w > 0]))))
    for rank, (n_glob, sw, lam), stats, r, extra in res:
        assert n_glob == single.num_data == int((w > 0).sum())
        assert report("two ranks sum w", abs(sw - single.weight_sum), single.weight_sum) <= 1e-12
        assert report("two ranks sum log w", abs(lam - single.log_weight_sum), lscale) <= 1e-12
        assert report("two ranks statistics", np.max(np.abs(stats - s1)), np.max(np.abs(s1))) <= 1e-12
        assert abs(r[0] - r1[0]) <= elbo_tol(r1[0], single.weight_sum, 1.0, 0.01, float(s1[-1]), bcr=True)
        np.testing.assert_allclose(r[1:4], r1[1:4], rtol=1e-6)
        assert extra[0] == sk.num_data and extra[1] == sk.weight_sum and abs(extra[2] - sk.log_weight_sum) <= 1e-12 * max(abs(sk.log_weight_sum), 1.0)
        assert abs(extra[3] - ek) <= 1e-9 * abs(ek)


# ------------------------------------------------------------------------------------------------ 10. fit() on the Snelson fixture
def test_fit_snelson_with_weights(A, S):
    """weights 1: the notebook golden, as tests/test_gpu_parity.py::test_notebook_golden_end_to_end; weights 0 on every second row: the
    fit of the model built from the other rows."""
    X, Y = np.asarray(S["X"]), np.asarray(S["Y"])
    model = A.GPR_1d((X, Y), A.Matern32(), A.B3Spline(-3.5, 10.5, 100), weights=np.ones(X.shape[0]))
    model.fit()
    e = model.elbo().item()
    assert report("Snelson fit, w = 1, vs the notebook golden", abs(e - float(S["golden_elbo_asvgp"])), 1.0) < 1e-7
    np.testing.assert_allclose(model.theta(), [0.798145059, 1.026880136, 0.080066643], rtol=5e-5)
    w = np.ones(X.shape[0])
    w[1::2] = 0.0
    mw = A.GPR_1d((X, Y), A.Matern32(), A.B3Spline(-3.5, 10.5, 100), weights=w)
    mh = A.GPR_1d((X[0::2], Y[0::2]), A.Matern32(), A.B3Spline(-3.5, 10.5, 100))
    mw.fit()
    mh.fit()
    assert report("Snelson fit, every second row masked, ELBO", abs(mw.elbo().item() - mh.elbo().item()), 1.0) < 1e-7
    np.testing.assert_allclose(mw.theta(), mh.theta(), rtol=5e-5)
