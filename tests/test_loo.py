"""GPU: closed-form leave-one-out predictions of GPR_1d (asvgp_posterior_prepare_loo_1d, asvgp_loo_1d) and GPR_kron (d = 2), and the
Python surface loo_predict_f_device / loo_predict_f / loo_log_density_device / loo_scores.

Yardsticks, written here: a dense numpy posterior from O.evaluate_basis and O.make_Kuu (Khatri-Rao rows for the Kronecker model), the
formulas of include/asvgp_hip.h on it, and BRUTE FORCE - the same dense posterior recomputed with w_i set to 0 and evaluated at x_i.
The mid-size case takes its posterior from the oracle's band routines instead, as O.predict_f_1d_banded does.

Tolerances.  delta_i = 1e-8 / (1 - h_i)^2 per row, h_i from the yardstick: 1e-8 absolute is this project's gate for
predict_f means and variances, and the formulas amplify an error in mu, g or h by at most (1 - h)^-2.  logdens against the Gaussian formula
applied to the kernel's own (mean, var): 1e-12 max(1, |value|).  scores against float sums of the per-row outputs: 1e-12 of sum |terms|.
max_leverage against the yardstick: 1e-6 (h = w g / sigma2 carries g's 1e-8 times w / sigma2, which stays below 1e2 in every case here).
Every comparison prints one "LERR" line (error over its gate or scale) for the record.

Size thresholds of asvgp_loo_1d's launch plan (csrc/row_scores.hip), each taken from both sides below:
  STAGE_MIN_N = 65 536   from here on the tables are staged in LDS, whole or split into ranges of mesh cells
  WRAP_N      = 262 144  the grid has at most this many threads (per range of cells), staged or not: beyond it the grid-stride loop wraps
  M = 1696 / 1697 (k = 4, D = 1)   the largest tables staged whole (8 (2 (k+1) (M + 1) + (M + 1) D + n_mesh + 64) bytes within
                         160 KiB - 512) / the smallest split into two ranges of cells; up to 4 ranges (2 for orders 5 and 6), beyond
                         that (k = 6, D = 1, M = 2500) the tables are read through the caches at every N
and the staged kernel runs 1024 threads per workgroup for orders 1..4, 512 for orders 5 and 6."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import asvgp_oracle as O

pytestmark = pytest.mark.gpu

STAGE_MIN_N = 65536
WRAP_N = 262144
KNAMES = {0: "Matern12", 1: "Matern32", 2: "Matern52"}


@pytest.fixture(scope="module")
def A():
    import asvgp_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from asvgp_amd import _lib
    _lib.get_lib()
    return asvgp_amd


def report(what, err, scale):
    r = float(err) / float(scale) if scale else float(err)
    print("LERR %-84s %.3e" % (what, r))
    return r


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def lognormal_weights(rng, n, zeros=True):
    w = np.exp(rng.normal(size=n))
    if zeros:
        w[rng.random(n) < 1 / 7] = 0.0
    return w


def make_x(rng, n, layout):
    lo, hi = 0.02, 0.98                       # (inside the boundary layer of the spline features, where phi^T Kuu^-1 phi exceeds k(x, x))
    if layout == "clustered":                 # a few narrow clusters: whole wavefronts inside one cell, and empty cells
        c = rng.uniform(lo, hi, 7)
        x = np.clip(c[rng.integers(0, 7, n)] + 1e-4 * rng.normal(size=n), lo, hi)
    else:
        x = rng.uniform(lo, hi, n)
    return np.sort(x) if layout == "sorted" else x


# ------------------------------------------------------------------------------------------------ yardsticks written here
def quad_rows(PhiT, S, chunk=32768):
    """phi_i^T S phi_i for every row phi_i^T of the sparse (N, M) matrix PhiT and a dense symmetric S, a chunk of rows at a time"""
    out = np.empty(PhiT.shape[0])
    for a in range(0, PhiT.shape[0], chunk):
        P = PhiT[a:a + chunk]
        out[a:a + chunk] = np.asarray(P.multiply(P @ S).sum(axis=1)).reshape(-1)
    return out


class Dense:
    """The dense posterior of a Gaussian linear model in the features: P = Kuu + Phi W Phi^T / s, alpha = P^-1 Phi W y / s.
    Phi: scipy sparse (M, N) (the Khatri-Rao rows for the Kronecker model); Kd: dense Kuu; prior: k(x, x)."""

    def __init__(self, Phi, Kd, prior, s, y, w):
        self.PhiT = Phi.T.tocsr()
        self.Kd, self.prior, self.s, self.y, self.w = Kd, float(prior), float(s), y, w
        self.Kinv = np.linalg.inv(Kd)
        self.qK = quad_rows(self.PhiT, self.Kinv)
        self.Pinv, self.alpha = self.solve(w)
        self.mu, self.g, self.var = self.at(self.Pinv, self.alpha)

    def solve(self, w):
        PhiW = self.PhiT.T.multiply(w[None, :]).tocsr()
        P = self.Kd + (PhiW @ self.PhiT).toarray() / self.s
        Pinv = np.linalg.inv(P)
        return Pinv, Pinv @ (PhiW @ self.y) / self.s

    def at(self, Pinv, alpha, rows=None):
        PhiT = self.PhiT if rows is None else self.PhiT[rows]
        qK = self.qK if rows is None else self.qK[rows]
        g = quad_rows(PhiT, Pinv)
        return PhiT @ alpha, g, self.prior + g - qK

    def formula(self):
        return closed_form(self.mu, self.g, self.var, self.y, self.w, self.s)

    def brute(self, i):
        """(mean (D,), var) of f(x_i) from the posterior recomputed with w_i = 0"""
        w = self.w.copy()
        w[i] = 0.0
        Pinv, alpha = self.solve(w)
        mu, _, var = self.at(Pinv, alpha, rows=[i])
        return mu[0], var[0]


def closed_form(mu, g, var, y, w, s):
    """(mean (N, D), var (N,), logdens (N,), h (N,)) of the left-out rows from the full posterior's mu, g and var (include/asvgp_hip.h)"""
    h = w * g / s
    mean = (mu - h[:, None] * y) / (1 - h)[:, None]
    vloo = var + g * h / (1 - h)
    return mean, vloo, gauss_logdens(y, mean, vloo, s, w), h


def gauss_logdens(y, mean, var, s, w):
    """sum_d log N(y_id | mean_id, var_i + s / w_i); a row with w_i = 0 takes noise variance s"""
    noise = np.where(w > 0, s / np.where(w > 0, w, 1.0), s)
    s2 = (np.asarray(var).reshape(-1) + noise)[:, None]
    return np.sum(-0.5 * (np.log(2 * np.pi * s2) + (y - mean) ** 2 / s2), axis=1)


def dense_1d(ob, kind, v, l, s, x, y, w):
    Phi = ob.evaluate_basis(x.reshape(-1, 1), sparse=True)
    return Dense(Phi, O.band_to_dense_sym(O.make_Kuu(ob, kind, v, l)), v, s, y, w)


def khatri_rao_sparse(obases, X):
    """sparse (m1 m2, N) Khatri-Rao design matrix, dim-0 major"""
    import scipy.sparse as sp
    P1 = obases[0].evaluate_basis(X[:, :1], sparse=False)
    P2 = obases[1].evaluate_basis(X[:, 1:], sparse=False)
    return sp.csr_matrix((P1[:, None, :] * P2[None, :, :]).reshape(-1, X.shape[0]))


def dense_kron(obases, kinds, thetas, s, X, y, w):
    Ks = [O.band_to_dense_sym(O.make_Kuu(bs, kd, v, l)) for bs, kd, (v, l) in zip(obases, kinds, thetas)]
    return Dense(khatri_rao_sparse(obases, X), np.kron(Ks[0], Ks[1]), float(np.prod([v for v, _ in thetas])), s, y, w)


def delta_gate(h):
    return 1e-8 / (1 - h) ** 2


def check_rows(tag, mean, var, ref_mean, ref_var, h, rows=None):
    """|error| <= delta_i per row, for the mean (every output column) and the variance"""
    gate = delta_gate(h if rows is None else h[rows])
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    em = np.max(np.abs(pick(mean) - ref_mean) / gate[:, None])
    ev = np.max(np.abs(pick(np.asarray(var).reshape(-1)) - np.asarray(ref_var).reshape(-1)) / gate)
    assert report(tag + " mean (over delta_i)", em, 1.0) <= 1.0
    assert report(tag + " variance (over delta_i)", ev, 1.0) <= 1.0


def logdens_gate(y, mean, var, s, w, delta):
    """first-order bound on the change of the log density when mean and variance each move by delta_i:
    sum_d |r_d| / s2 * delta + (D / s2 + sum_d r_d^2 / s2^2) / 2 * delta,  r = y - mean, s2 = var + noise"""
    noise = np.where(w > 0, s / np.where(w > 0, w, 1.0), s)
    s2 = np.asarray(var).reshape(-1) + noise
    r = np.abs(y - mean)
    return (np.sum(r, axis=1) / s2 + 0.5 * (y.shape[1] / s2 + np.sum(r * r, axis=1) / s2 ** 2)) * delta


def check_logdens(tag, ld, y, mean, var, s, w):
    ref = gauss_logdens(y, mean, var, s, w)
    assert report(tag + " logdens vs the Gaussian formula on the kernel's own moments",
                  np.max(np.abs(ld - ref) / np.maximum(1.0, np.abs(ref))), 1.0) <= 1e-12


def check_scores(tag, sc, ld, y, mean, w, h_ref):
    """scores = [n, sum logdens, sum squared error, max h] against float sums of the per-row outputs over the rows with w > 0"""
    pos = w > 0
    assert sc[0] == pos.sum()
    assert report(tag + " scores: sum logdens", abs(sc[1] - np.sum(ld[pos])), max(np.sum(np.abs(ld[pos])), 1e-300)) <= 1e-12
    sq = ((y - mean) ** 2)[pos]
    assert report(tag + " scores: sum squared error", abs(sc[2] - np.sum(sq)), max(np.sum(sq), 1e-300)) <= 1e-12
    assert report(tag + " scores: max leverage", abs(sc[3] - (np.max(h_ref[pos]) if pos.any() else 0.0)), 1.0) <= 1e-6


def sliced(t, off):
    """a copy of t that starts 8 * off bytes into a fresh 16-byte aligned allocation"""
    buf = torch.zeros(t.numel() + off, dtype=torch.float64, device="cuda")
    buf[off:] = t.reshape(-1)
    out = buf[off:]
    if off:
        assert out.data_ptr() % 16 == 8
    return out


def loo_call(model, xt, yt, wt, N, D, want="mvls", off=0):
    """asvgp_loo_1d through the C-ABI on device tensors (any alignment) with the model's tables -> dict of numpy outputs"""
    from asvgp_amd import _lib
    lib = _lib.get_lib()
    alpha, W, Pinv = model._posterior_loo()
    b = model.basis
    ws = torch.empty(lib.asvgp_loo_workspace_bytes(b.m, b.order, D) // 8, dtype=torch.float64, device="cuda")
    out = {c: sliced(torch.full((n,), 7.0, dtype=torch.float64, device="cuda"), off) if c in want else None
           for c, n in (("m", N * D), ("v", N), ("l", N), ("s", 4))}
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.asvgp_loo_1d(model._h.ptr, ptr(xt), ptr(yt), ptr(wt), N, D, b.mesh.data_ptr(), b.mesh.shape[0], b.delta_np, b.order, b.m,
                          alpha.data_ptr(), W.data_ptr(), Pinv.data_ptr(), float(model.kernel.variance), float(model.likelihood.variance),
                          ptr(out["m"]), ptr(out["v"]), ptr(out["l"]), ptr(out["s"]), ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.asvgp_last_error_string().decode()
    res = {c: None if t is None else t.cpu().numpy() for c, t in out.items()}
    if res["m"] is not None:
        res["m"] = res["m"].reshape(N, D)
    return res


def problem_1d(seed, order, kind, M, N, D, s, layout="unsorted", weights=True, f32mesh=False, l=0.2, v=1.2):
    rng = np.random.default_rng(seed)
    x = make_x(rng, N, layout)
    y = np.stack([np.sin(9 * (d + 1) * x) for d in range(D)], 1) + 0.3 * rng.normal(size=(N, D))
    w = lognormal_weights(rng, N) if weights else None
    if w is not None and N <= 2:
        w[:] = 1.7
    a, b = (0.0, 1.0) if f32mesh else (0, 1)
    return dict(order=order, kind=kind, M=M, N=N, D=D, s=s, l=l, v=v, x=x, y=y, w=w, ab=(a, b))


def build_1d(A, p, w="own", **kw):
    w = p["w"] if isinstance(w, str) else w
    m = A.GPR_1d((p["x"].reshape(-1, 1), p["y"]), getattr(A, KNAMES[p["kind"]])(variance=p["v"], lengthscales=p["l"]),
                 getattr(A, "B%dSpline" % p["order"])(p["ab"][0], p["ab"][1], p["M"]), weights=w, **kw)
    m.likelihood.variance.assign(p["s"])
    return m


def yardstick_1d(p):
    ob = O.Basis(p["order"], p["ab"][0], p["ab"][1], p["M"])
    w = p["w"] if p["w"] is not None else np.ones(p["N"])
    return dense_1d(ob, p["kind"], p["v"], p["l"], p["s"], p["x"], p["y"], w), w


# ------------------------------------------------------------------------------------------------ 1. formula and brute force, 1-D
CASE1 = [(4, 1, 40, 400, 1, 0.03, True), (3, 2, 30, 300, 2, 0.05, False), (2, 0, 25, 200, 1, 0.03, True)]


def case1_problem(i):
    order, kind, M, N, D, s, weighted = CASE1[i]
    return problem_1d(100 + i, order, kind, M, N, D, s, weights=weighted)


@pytest.mark.parametrize("case", range(len(CASE1)))
def test_formula_and_brute_force_1d(A, case):
    p = case1_problem(case)
    model = build_1d(A, p)
    ref, w = yardstick_1d(p)
    fm, fv, fl, h = ref.formula()
    tag = "1-D k=%d %s M=%d N=%d D=%d" % (p["order"], KNAMES[p["kind"]], p["M"], p["N"], p["D"])
    report(tag + " yardstick max leverage", np.max(h), 1.0)
    mean_t, var_t = model.loo_predict_f_device()
    assert mean_t.shape == (p["N"], p["D"]) and var_t.shape == (p["N"], 1) and mean_t.is_cuda
    mean, var = mean_t.cpu().numpy(), var_t.cpu().numpy().reshape(-1)
    check_rows(tag + " vs formula", mean, var, fm, fv, h)
    brute = [ref.brute(i) for i in range(p["N"])]
    bm, bv = np.array([b[0] for b in brute]), np.array([b[1] for b in brute])
    check_rows(tag + " vs brute force (every row)", mean, var, bm, bv, h)
    assert report(tag + " formula yardstick vs brute force", max(np.max(np.abs(fm - bm) * (1 - h)[:, None]), np.max(np.abs(fv - bv) * (1 - h))), 1.0) <= 1e-12
    hm, hv = model.loo_predict_f()
    assert isinstance(hm, np.ndarray) and np.array_equal(hm, mean) and np.array_equal(hv.reshape(-1), var)
    ld = model.loo_log_density_device()
    assert ld.shape == (p["N"],) and ld.is_cuda
    ld = ld.cpu().numpy()
    check_logdens(tag, ld, p["y"], mean, var, p["s"], w)
    assert report(tag + " logdens vs the yardstick's (over the first-order image of delta_i)",
                  np.max(np.abs(ld - fl) / logdens_gate(p["y"], fm, fv, p["s"], w, delta_gate(h))), 1.0) <= 1.0
    sc = model.loo_scores()
    assert all(isinstance(sc[k], float) for k in ("n", "log_density", "sq_err", "max_leverage", "nlpd", "rmse"))
    check_scores(tag, [sc["n"], sc["log_density"], sc["sq_err"], sc["max_leverage"]], ld, p["y"], mean, w, h)
    assert sc["nlpd"] == -sc["log_density"] / sc["n"] and sc["rmse"] == math.sqrt(sc["sq_err"] / (sc["n"] * p["D"]))
    # rows with w_i = 0 are absent already: the ordinary prediction, and not counted
    zero = np.flatnonzero(w == 0)
    assert sc["n"] == p["N"] - zero.size
    if p["w"] is not None:
        assert zero.size > 0
        pm, pv = model.predict_f_device(p["x"][zero].reshape(-1, 1))
        assert report(tag + " rows with w = 0 vs predict_f_device", max(np.max(np.abs(pm.cpu().numpy() - mean[zero])),
                                                                        np.max(np.abs(pv.cpu().numpy().reshape(-1) - var[zero]))), 1.0) <= 1e-8
    # the tables: alpha and W are those of asvgp_posterior_prepare_1d bit for bit, Pinv_band is band(P^-1)
    alpha, W, Pinv = model._posterior_loo()
    a0, W0 = model._posterior()
    assert torch.equal(alpha, a0) and torch.equal(W, W0)
    k = p["order"]
    Pb = np.stack([np.concatenate([np.diagonal(ref.Pinv, -d), np.zeros(d)]) for d in range(k + 1)])
    assert report(tag + " Pinv_band vs dense P^-1", np.max(np.abs(Pinv.cpu().numpy() - Pb)), np.max(np.abs(Pb))) <= 1e-9


# ------------------------------------------------------------------------------------------------ 2. kernel shapes, 1-D
# (order, M, N, D, layout, weighted, sliced 8 bytes into a 16-byte allocation?, float32-linspace mesh?)
SHAPES = [
    (2, 8, 1, 1, "unsorted", True, False, False),
    (2, 8, 2, 1, "unsorted", False, False, False),
    (4, 40, 4099, 1, "sorted", True, True, False),
    (6, 40, 4099, 3, "clustered", True, False, False),
    (5, 257, 20_001, 1, "unsorted", False, False, True),
    # the thresholds of the launch plan, from both sides
    (4, 40, STAGE_MIN_N - 1, 1, "unsorted", True, False, False),      # tables through the caches
    (4, 40, STAGE_MIN_N, 1, "unsorted", True, True, False),           # staged, 1024 threads
    (4, 40, WRAP_N, 1, "unsorted", False, False, False),              # the largest grid that does not wrap
    (4, 40, WRAP_N + 1, 2, "sorted", True, False, False),             # one row past it
    (6, 40, STAGE_MIN_N + 4465, 1, "unsorted", True, False, False),   # staged, 512 threads (orders 5 and 6)
    (4, 1696, STAGE_MIN_N + 4465, 1, "unsorted", True, False, False), # the largest tables staged whole
    (4, 1697, STAGE_MIN_N + 4465, 1, "unsorted", True, False, False), # two ranges of cells
    (4, 2048, WRAP_N + 1, 1, "sorted", False, False, False),          # the headline's tables: two ranges, and the grid wraps
    (3, 4500, STAGE_MIN_N, 3, "clustered", True, True, False),        # four ranges, D = 3, a short last range, ranges without rows
    (6, 2500, WRAP_N + 1, 1, "unsorted", False, False, False),        # tables too large for two ranges: not staged, and the grid wraps
]


@pytest.mark.parametrize("order,M,N,D,layout,weighted,unaligned,f32mesh", SHAPES)
def test_kernel_shapes_1d(A, order, M, N, D, layout, weighted, unaligned, f32mesh):
    # (order 5 takes Matern-5/2; the order-6 basis carries the static bands of Matern-1/2 and 3/2 only, as the reference's does)
    kind = 2 if order == 5 else (0 if order == 2 else 1)
    p = problem_1d(1000 * order + M + N, order, kind, M, N, D, 0.05, layout=layout, weights=weighted, f32mesh=f32mesh,
                   l=0.2 if M < 1000 else 20.0 / M)
    model = build_1d(A, p)
    if M >= 1000:                             # (two dense M x M inverses take seconds here: the same formulas on the oracle's band routines)
        w = np.ones(N) if p["w"] is None else p["w"]
        fm, fv, _, h = closed_form(*banded_yardstick(O.Basis(order, p["ab"][0], p["ab"][1], M), kind, p["v"], p["l"], p["s"], p["x"], p["y"], w),
                                   p["y"], w, p["s"])
    else:
        ref, w = yardstick_1d(p)
        fm, fv, _, h = ref.formula()
    tag = "shape k=%d M=%d N=%d D=%d %s%s%s%s" % (order, M, N, D, layout, " weighted" if weighted else "", " unaligned" if unaligned else "",
                                                  " f32 mesh" if f32mesh else "")
    report(tag + " yardstick max leverage", np.max(h), 1.0)
    off = 1 if unaligned else 0
    xt, yt = sliced(dev(p["x"]), off), sliced(dev(p["y"]), off)
    wt = sliced(dev(p["w"]), off) if weighted else None
    full = loo_call(model, xt, yt, wt, N, D, "mvls", off)
    check_rows(tag, full["m"], full["v"], fm, fv, h)
    check_logdens(tag, full["l"], p["y"], full["m"], full["v"], p["s"], w)
    check_scores(tag, full["s"], full["l"], p["y"], full["m"], w, h)
    only = loo_call(model, xt, yt, wt, N, D, "s", off)                # scores only: nothing of size N is written
    again = loo_call(model, xt, yt, wt, N, D, "s", off)
    assert only["s"].tobytes() == full["s"].tobytes() == again["s"].tobytes()
    mix = loo_call(model, xt, yt, wt, N, D, "mls", off)               # var NULL
    assert mix["v"] is None and np.array_equal(mix["m"], full["m"]) and np.array_equal(mix["l"], full["l"])
    assert mix["s"].tobytes() == full["s"].tobytes()
    one = loo_call(model, xt, yt, wt, N, D, "v", off)                 # a single per-row output, no scores
    assert np.array_equal(one["v"], full["v"])


def test_empty_batch_zeroes_scores(A):
    p = problem_1d(5, 4, 1, 40, 50, 1, 0.05)
    model = build_1d(A, p)
    got = loo_call(model, None, None, None, 0, 1, "s")
    assert np.array_equal(got["s"], np.zeros(4))


# ------------------------------------------------------------------------------------------------ 3. through the library's own weights
def test_matches_model_refitted_with_weight_zero(A):
    p = case1_problem(0)
    model = build_1d(A, p)
    ref, w = yardstick_1d(p)
    h = ref.formula()[3]
    mean, var = (t.cpu().numpy() for t in model.loo_predict_f_device())
    rows = np.flatnonzero(w > 0)[::37][:8]
    assert rows.size == 8
    for i in rows:
        wi = w.copy()
        wi[i] = 0.0
        refit = build_1d(A, p, w=wi)
        pm, pv = (t.cpu().numpy() for t in refit.predict_f_device(p["x"][i:i + 1].reshape(-1, 1)))
        err = max(np.max(np.abs(pm[0] - mean[i])), abs(pv[0, 0] - var[i, 0]))
        assert report("refit with w[%d] = 0 vs the LOO row (over delta_i)" % i, err, delta_gate(h[i])) <= 1.0


# ------------------------------------------------------------------------------------------------ 4. high leverage
def high_leverage_problem():
    rng = np.random.default_rng(4)
    N, M = 80, 64
    x = np.sort(rng.uniform(0.02, 0.98, N))
    y = (np.sin(9 * x) + 0.01 * rng.normal(size=N)).reshape(-1, 1)
    return dict(order=4, kind=1, M=M, N=N, D=1, s=1e-4, l=HIGH_L, v=1.2, x=x, y=y, w=None, ab=(0, 1))


HIGH_L = 0.095                # Matern-3/2 lengthscale at which the yardstick's max h is 0.9990


def test_high_leverage(A):
    p = high_leverage_problem()
    model = build_1d(A, p)
    ref, w = yardstick_1d(p)
    fm, fv, _, h = ref.formula()
    hmax = float(np.max(h))
    report("high leverage: yardstick max h", hmax, 1.0)
    assert 0.998 <= hmax < 1.0
    mean, var = (t.cpu().numpy() for t in model.loo_predict_f_device())
    check_rows("high leverage k=4 M=64 N=80 s=1e-4", mean, var.reshape(-1), fm, fv, h)
    sc = model.loo_scores()
    assert report("high leverage: max_leverage vs yardstick", abs(sc["max_leverage"] - hmax), 1.0) <= 1e-6
    # nothing is clamped: the row of the largest leverage carries the formula's 1 / (1 - h) factor in full
    i = int(np.argmax(h))
    assert var[i, 0] - ref.var[i] >= 0.5 * ref.g[i] * h[i] / (1 - h[i]) and sc["max_leverage"] > 0.998


# ------------------------------------------------------------------------------------------------ 5. mid-size, against the oracle's band routines
def banded_yardstick(ob, kind, v, l, s, x, y, w):
    """(mu, g, var) per training row through band quantities only, as O.predict_f_1d_banded: band(P^-1), band(Kuu^-1) and alpha from the
    oracle's band Cholesky / selected inverse / triangular solves on the directly accumulated weighted statistics."""
    k, M = ob.order, ob.m
    idx = O.neighbour_index(ob.mesh, x)
    vals = O.piece_values(k, (x - ob.mesh[idx]) / ob.delta)         # piece i -> row idx + k - i
    band = np.zeros((k + 1, M))
    rhs = np.zeros((M, y.shape[1]))
    for i in range(k + 1):
        for d in range(y.shape[1]):
            rhs[:, d] += np.bincount(idx + k - i, weights=w * vals[i] * y[:, d], minlength=M)
        for j in range(i, k + 1):
            band[j - i] += np.bincount(idx + k - j, weights=w * vals[i] * vals[j], minlength=M)
    Kuu = O.make_Kuu(ob, kind, v, l)
    SK = O.inverse_from_cholesky_band(O.cholesky_band(Kuu))
    LP = O.cholesky_band(band / s + Kuu)
    SP = O.inverse_from_cholesky_band(LP)
    alpha = O.solve_triang_mat(LP, O.solve_triang_mat(LP, rhs) / s, transpose_left=True)
    mu = np.zeros((x.shape[0], y.shape[1]))
    g = np.zeros(x.shape[0])
    qK = np.zeros(x.shape[0])
    for i in range(k + 1):
        ri = idx + k - i
        mu += vals[i][:, None] * alpha[ri]
        for j in range(k + 1):
            rj = idx + k - j
            hi, lo = np.maximum(ri, rj), np.minimum(ri, rj)
            g += vals[i] * vals[j] * SP[hi - lo, lo]
            qK += vals[i] * vals[j] * SK[hi - lo, lo]
    return mu, g, v + g - qK


MIDSIZE_GATE = 1e-8       # predict_f_device's own error against this yardstick at this shape stays inside 1e-8


def test_midsize_against_band_oracle(A):
    order, kind, M, N, l, v, s = 4, 1, 1024, 100_000, 0.02, 1.2, 0.03
    rng = np.random.default_rng(40 + M)
    x = rng.uniform(0.02, 0.98, N)
    y = (np.sin(15 * x) + 0.2 * rng.normal(size=N)).reshape(-1, 1)
    w = lognormal_weights(rng, N)
    p = dict(order=order, kind=kind, M=M, N=N, D=1, s=s, l=l, v=v, x=x, y=y, w=w, ab=(0, 1))
    model = build_1d(A, p)
    mu, g, var0 = banded_yardstick(O.Basis(order, 0, 1, M), kind, v, l, s, x, y, w)
    h = w * g / s
    report("mid-size: yardstick max leverage", np.max(h), 1.0)
    pm, pv = (t.cpu().numpy() for t in model.predict_f_device(x.reshape(-1, 1)))
    e0 = max(np.max(np.abs(pm - mu)), np.max(np.abs(pv.reshape(-1) - var0)))
    report("mid-size: predict_f_device's own error against the band yardstick (absolute)", e0, 1.0)
    gate = MIDSIZE_GATE / (1 - h) ** 2
    fm, fv, _, _ = closed_form(mu, g, var0, y, w, s)
    mean, var = (t.cpu().numpy() for t in model.loo_predict_f_device())
    assert report("mid-size k=4 M=1024 N=100000 mean (over its gate)", np.max(np.abs(mean - fm) / gate[:, None]), 1.0) <= 1.0
    assert report("mid-size k=4 M=1024 N=100000 variance (over its gate)", np.max(np.abs(var.reshape(-1) - fv) / gate), 1.0) <= 1.0
    ld = model.loo_log_density_device().cpu().numpy()
    check_logdens("mid-size", ld, y, mean, var.reshape(-1), s, w)
    sc = model.loo_scores()
    check_scores("mid-size", [sc["n"], sc["log_density"], sc["sq_err"], sc["max_leverage"]], ld, y, mean, w, h)


# ------------------------------------------------------------------------------------------------ 6. Kronecker
def kron_problem(order, m1, m2, N, weighted=True):
    rng = np.random.default_rng(m1 * 100 + m2 + 1)
    X = np.stack([rng.uniform(0.03, 0.97, N), rng.uniform(-0.91, 1.91, N)], axis=1)     # (off the boundary layer, as make_x)
    y = np.sin(12 * X[:, :1]) * np.cos(3 * X[:, 1:]) + 0.1 * rng.normal(size=(N, 1))
    w = lognormal_weights(rng, N) if weighted else None
    return X, y, w


KRON_TH, KRON_S = [(1.1, 0.3), (0.7, 0.6)], 0.05


def build_kron(A, order, m1, m2, X, y, w, **kw):
    B = getattr(A, "B%dSpline" % order)
    kerns = [A.Matern32(variance=KRON_TH[0][0], lengthscales=KRON_TH[0][1]), A.Matern32(variance=KRON_TH[1][0], lengthscales=KRON_TH[1][1])]
    model = A.GPR_kron((X, y), kerns, [B(0, 1, m1), B(-1, 2, m2)], weights=w, **kw)
    model.likelihood.variance.assign(KRON_S)
    return model


def kron_yardstick(order, m1, m2, X, y, w):
    obases = [O.Basis(order, 0, 1, m1), O.Basis(order, -1, 2, m2)]
    wd = w if w is not None else np.ones(X.shape[0])
    return dense_kron(obases, [1, 1], KRON_TH, KRON_S, X, y, wd), wd


def check_kron_outputs(tag, model, ref, w, y, h, fm, fv):
    mean, var = (t.cpu().numpy() for t in model.loo_predict_f_device())
    assert mean.shape == var.shape == (y.shape[0], 1)
    check_rows(tag + " vs formula", mean, var, fm, fv, h)
    ld = model.loo_log_density_device().cpu().numpy()
    check_logdens(tag, ld, y, mean, var.reshape(-1), KRON_S, w)
    sc = model.loo_scores()
    check_scores(tag, [sc["n"], sc["log_density"], sc["sq_err"], sc["max_leverage"]], ld, y, mean, w, h)
    assert sc["nlpd"] == -sc["log_density"] / sc["n"] and sc["rmse"] == math.sqrt(sc["sq_err"] / sc["n"])
    return mean, var, ld


@pytest.mark.parametrize("order,m1,m2,N,weighted", [(3, 8, 9, 300, True), (4, 14, 16, 2000, True), (3, 8, 9, 300, False)])
def test_kron_formula_and_brute_force(A, order, m1, m2, N, weighted):
    X, y, w0 = kron_problem(order, m1, m2, N, weighted)
    model = build_kron(A, order, m1, m2, X, y, w0)
    ref, w = kron_yardstick(order, m1, m2, X, y, w0)
    fm, fv, _, h = ref.formula()
    tag = "kron k=%d %dx%d N=%d%s" % (order, m1, m2, N, " weighted" if weighted else "")
    report(tag + " yardstick max leverage", np.max(h), 1.0)
    mean, var, _ = check_kron_outputs(tag, model, ref, w, y, h, fm, fv)
    rows = np.flatnonzero(w > 0)[::max(1, N // 30)][:25]
    assert rows.size == 25
    brute = [ref.brute(i) for i in rows]
    check_rows(tag + " vs brute force (25 rows)", mean, var, np.array([b[0] for b in brute]), np.array([b[1] for b in brute]), h, rows=rows)
    zero = np.flatnonzero(w == 0)
    if weighted:
        pm, pv = model.predict_f_device(X[zero])
        assert report(tag + " rows with w = 0 vs predict_f_device", max(np.max(np.abs(pm.cpu().numpy() - mean[zero])),
                                                                        np.max(np.abs(pv.cpu().numpy() - var[zero]))), 1.0) <= 1e-8


@pytest.mark.parametrize("order,m1,m2,N", [(3, 12, 14, 3000), (3, 16, 14, 3000)])
def test_kron_both_layouts(A, order, m1, m2, N):
    """12 x 14 (168 columns, super-blocks of 64) has no two-sided factorisation: fewer than the 3 super-blocks per side it needs, so forcing
    it leaves the one-sided layout.  16 x 14 (224 columns) is the smallest grid of the same family that has both, and both are taken."""
    X, y, w0 = kron_problem(order, m1, m2, N)
    model = build_kron(A, order, m1, m2, X, y, w0)
    ref, w = kron_yardstick(order, m1, m2, X, y, w0)
    fm, fv, _, h = ref.formula()
    tag = "kron k=%d %dx%d N=%d" % (order, m1, m2, N)
    got = {}
    for tw in (False, True):                  # one-sided band Cholesky / two-sided factorisation, forced as the existing Kronecker tests do
        model.twisted = tw
        has = model._twist_layout() is not None
        assert has == (tw and m1 == 16)
        got[has] = check_kron_outputs(tag + " twisted=%s" % has, model, ref, w, y, h, fm, fv)
        assert (model._post[1].get("twist") is not None) == has
    if m1 == 16:
        for name, a, b in zip(("mean", "variance", "logdens"), got[False], got[True]):
            assert report(tag + " both layouts agree: " + name, np.max(np.abs(a - b)), 1.0) <= 1e-10
    model.twisted = None
    auto = model.loo_predict_f_device()[0].cpu().numpy()
    assert np.array_equal(auto, got[model._twist_layout() is not None][0])


# ------------------------------------------------------------------------------------------------ 7. two ranks on one GPU over gloo
def shard_problem():
    return problem_1d(2025, 4, 1, 256, 20_001, 1, 0.01, l=0.05, v=1.0)


def _loo_shard_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)                       # both ranks share the one GPU of the test box; gloo moves the band
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import asvgp_amd as A
    from asvgp_amd.dist import shard_bounds
    p = shard_problem()
    lo, hi = shard_bounds(p["N"], world, rank)
    local = dict(p, x=p["x"][lo:hi], y=p["y"][lo:hi], w=p["w"][lo:hi], N=hi - lo)
    m = build_1d(A, local, process_group=dist.group.WORLD)
    sc = m.loo_scores()
    mean, var = (t.cpu().numpy() for t in m.loo_predict_f_device())
    q.put((rank, lo, hi, sc, mean, var, m.loo_log_density_device().cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(A):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33600 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_loo_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    p = shard_problem()
    single = build_1d(A, p)
    mean, var = (t.cpu().numpy() for t in single.loo_predict_f_device())
    return p, res, single.loo_scores(), mean, var, single.loo_log_density_device().cpu().numpy()


def test_two_rank_sharded_scores_and_rows_match_single_rank(two_ranks):
    p, res, s1, mean, var, ld = two_ranks
    ref, w = yardstick_1d(p)
    gate = delta_gate(ref.formula()[3])
    assert sorted(r[0] for r in res) == [0, 1]
    for rank, lo, hi, sc, m, v, l in res:
        assert sc["n"] == s1["n"] == float((w > 0).sum())
        for k in ("log_density", "sq_err", "nlpd", "rmse"):
            assert report("two ranks (rank %d) %s" % (rank, k), abs(sc[k] - s1[k]), abs(s1[k])) <= 1e-12
        # each rank's rows are the matching slice of the single-rank outputs (the two posteriors differ by the rounding of the all-reduce)
        assert report("two ranks (rank %d) mean rows (over delta_i)" % rank, np.max(np.abs(m - mean[lo:hi]) / gate[lo:hi, None]), 1.0) <= 1.0
        assert report("two ranks (rank %d) variance rows (over delta_i)" % rank, np.max(np.abs(v - var[lo:hi]) / gate[lo:hi, None]), 1.0) <= 1.0
        lgate = logdens_gate(p["y"], mean, var, p["s"], w, gate)[lo:hi]
        assert report("two ranks (rank %d) logdens rows (over the first-order image of delta_i)" % rank, np.max(np.abs(l - ld[lo:hi]) / lgate), 1.0) <= 1.0
    assert res[0][3] == res[1][3]                  # every rank returns the same global scores


def test_two_rank_sharded_max_leverage_equals_single_rank(two_ranks):
    """Exact equality of max_leverage between the sharded and the single-rank model, as the issue sets it.  It holds only when the two
    posteriors are bit-identical, and they are not in general.  (1) The Phi pass sums the points of a cell in the arrival order of its
    rank atomics (csrc/phi_sort.hpp: "reproducible to rounding (a few ulp ...)"), so even two builds of the SAME model differ in the
    last bits of the statistics.  (2) The sharded statistics are the all-reduced sum of two partial passes, the single-rank ones a sum in
    another order.  h = w g / sigma2 inherits the last-bit difference of band(P^-1).  Measured on one MI355X in four runs of the same
    build: |difference| = 0, 2.8e-17, 2.8e-17 and 1.7e-16 (0.23525936587834312 on the ranks every time; 0.23525936587834312, ...315,
    ...315, ...329 on the single rank).  The leave-one-out kernel itself is bit-reproducible on given tables (test_kernel_shapes_1d);
    nothing in it can make two separately accumulated posteriors equal to the bit, so this test fails whenever the last bits show."""
    _, res, s1, _, _, _ = two_ranks
    for rank, _, _, sc, _, _, _ in res:
        report("two ranks (rank %d) max_leverage - single rank's (absolute)" % rank, abs(sc["max_leverage"] - s1["max_leverage"]), 1.0)
        assert sc["max_leverage"] == s1["max_leverage"]


# ------------------------------------------------------------------------------------------------ 8. loud failures
LOO_METHODS = ("loo_predict_f_device", "loo_predict_f", "loo_log_density_device", "loo_scores")


def test_loud_failures(A):
    from asvgp_amd.banded import NotPositiveDefiniteError
    rng = np.random.default_rng(1)
    X3 = rng.uniform(0.01, 0.99, (100, 3))
    y = np.sin(9 * X3[:, :1])
    add = A.GPR_additive((X3[:, :2], y), [A.Matern32(), A.Matern32()], [A.B3Spline(0, 1, 10), A.B3Spline(0, 1, 11)])
    k3 = A.GPR_kron((X3, y), [A.Matern32()] * 3, [A.B3Spline(0, 1, 10)] * 3)
    for model in (add, k3):
        for name in LOO_METHODS:
            with pytest.raises(NotImplementedError, match=name):
                getattr(model, name)()
    # a P that is not positive definite is reported, not streamed
    p = case1_problem(0)
    bad = build_1d(A, p)
    bad._stats[20] = -1.0e9                                          # diagonal entry 20 of the KufKfu band
    with pytest.raises(NotPositiveDefiniteError):
        bad.loo_scores()
    X, yk, w = kron_problem(3, 8, 9, 300)
    badk = build_kron(A, 3, 8, 9, X, yk, w)
    badk._stats[:badk.noff * badk.Mtot].mul_(-1.0)
    with pytest.raises(NotPositiveDefiniteError):
        badk.loo_scores()
