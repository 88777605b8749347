"""GPU: held-out scores in one streaming pass (asvgp_score_1d; score / predict_log_density_device / predict_y_device on every model class),
set_weights and kfold_scores of GPR_1d and GPR_kron (d = 2).

Yardsticks, written here in the style of tests/test_loo.py: a dense numpy posterior from O.evaluate_basis and O.make_Kuu (Khatri-Rao rows
for the Kronecker model) evaluated at the held-out rows with the formulas of include/asvgp_hip.h; from M = 1000 on the same formulas on
the oracle's band routines, as O.predict_f_1d_banded does.

Tolerances (tests/test_loo.py).  Mean and variance: 1e-8 absolute.  logdens against the Gaussian formula on the
kernel's own moments: 1e-12 max(1, |value|); against the yardstick: the first-order image of 1e-8 (logdens_gate).  Scores against float sums
of the per-row outputs: 1e-12 of sum |terms|; counts exact.  Sums of a fold against a yardstick: the summed first-order images of 1e-8,
  |d logdens| <= (sum_d |r_d| / s2 + (D / s2 + sum_d r_d^2 / s2^2) / 2) delta      (logdens_gate)
  |d sq_err|  <= 2 sum_d |r_d| delta                                                (sq = sum_d r_d^2, r = y - mean moves by delta)
  |d chi2|    <= (2 sum_d |r_d| / s2 + sum_d r_d^2 / s2^2) delta                    (chi2 = sq / s2, mean and s2 each move by delta)
plus the 1e-12 sum |terms| of the summation itself.  Every comparison prints one "SERR" line (error over its gate or scale).

Size thresholds of asvgp_score_1d's launch plan (csrc/row_scores.hip), each taken from both sides below:
  STAGE_MIN_N = 65 536   from here on the tables are staged in LDS, whole or split into ranges of mesh cells
  WRAP_N      = 262 144  the grid has at most this many threads (per range of cells): beyond it the grid-stride loop wraps
  M = 2907 / 2908 (k = 4, D = 1)   the largest tables staged whole (8 ((k+1) M + M D + n_mesh + 64) bytes within 160 KiB - 512) / the
                         smallest split into two ranges; up to 4 ranges (2 for orders 5 and 6); beyond that (k = 6, D = 3, M = 3500) the
                         tables are read through the caches at every N
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
GATE = 1e-8


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
    print("SERR %-92s %.3e" % (what, r))
    return r


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def lognormal_weights(rng, n, zeros=True):
    w = np.exp(rng.normal(size=n))
    if zeros:
        w[rng.random(n) < 1 / 7] = 0.0
    return w


def make_x(rng, n, layout="unsorted"):
    lo, hi = 0.02, 0.98
    if layout == "clustered":                 # a few narrow clusters: whole wavefronts inside one cell, and empty cells
        c = rng.uniform(lo, hi, 7)
        x = np.clip(c[rng.integers(0, 7, n)] + 1e-4 * rng.normal(size=n), lo, hi)
    else:
        x = rng.uniform(lo, hi, n)
    return np.sort(x) if layout == "sorted" else x


def make_y(rng, x, D):
    return np.stack([np.sin(9 * (d + 1) * x) for d in range(D)], 1) + 0.3 * rng.normal(size=(x.shape[0], D))


# ------------------------------------------------------------------------------------------------ yardsticks written here
def quad_rows(PhiT, S_, chunk=32768):
    """phi_i^T S phi_i for every row phi_i^T of the sparse (N, M) matrix PhiT and a dense symmetric S, a chunk of rows at a time"""
    out = np.empty(PhiT.shape[0])
    for a in range(0, PhiT.shape[0], chunk):
        P = PhiT[a:a + chunk]
        out[a:a + chunk] = np.asarray(P.multiply(P @ S_).sum(axis=1)).reshape(-1)
    return out


class Dense:
    """The dense posterior of a Gaussian linear model in the features: P = Kuu + Phi W Phi^T / s, alpha = P^-1 Phi W y / s.
    Phi: scipy sparse (M, N) of the TRAINING rows (the Khatri-Rao rows for the Kronecker model); Kd: dense Kuu; prior: k(x, x)."""

    def __init__(self, Phi, Kd, prior, s, y, w):
        PhiT = Phi.T.tocsr()
        self.prior, self.s = float(prior), float(s)
        self.Kinv = np.linalg.inv(Kd)
        PhiW = PhiT.T.multiply(w[None, :]).tocsr()
        self.Pinv = np.linalg.inv(Kd + (PhiW @ PhiT).toarray() / s)
        self.alpha = self.Pinv @ (PhiW @ y) / s

    def at(self, Phi_new):
        """(mu (n, D), g (n,), var (n,)) at the rows whose features are the columns of Phi_new"""
        PhiT = Phi_new.T.tocsr()
        g = quad_rows(PhiT, self.Pinv)
        return PhiT @ self.alpha, g, self.prior + g - quad_rows(PhiT, self.Kinv)


def noise_of(w, s):
    return np.where(w > 0, s / np.where(w > 0, w, 1.0), s)


def gauss_logdens(y, mean, var, s, w):
    """sum_d log N(y_id | mean_id, var_i + s / w_i); a row with w_i = 0 takes noise variance s"""
    s2 = (np.asarray(var).reshape(-1) + noise_of(w, s))[:, None]
    return np.sum(-0.5 * (np.log(2 * np.pi * s2) + (y - mean) ** 2 / s2), axis=1)


def row_gates(y, mean, var, s, w, delta=GATE):
    """first-order bounds per row on the change of (logdens, sq, chi2) when mean and variance each move by delta (module docstring)"""
    s2 = np.asarray(var).reshape(-1) + noise_of(w, s)
    r = np.abs(y - mean)
    r1, r2 = np.sum(r, axis=1), np.sum(r * r, axis=1)
    return ((r1 / s2 + 0.5 * (y.shape[1] / s2 + r2 / s2 ** 2)) * delta, 2 * r1 * delta, (2 * r1 / s2 + r2 / s2 ** 2) * delta)


def logdens_gate(y, mean, var, s, w, delta=GATE):
    return row_gates(y, mean, var, s, w, delta)[0]


def score_sums(y, mean, var, s, w):
    """the yardstick's [n, sum logdens, sum sq, sum chi2] over w > 0, their gates (summed first-order images of 1e-8 + 1e-12 sum |terms|)"""
    pos = w > 0
    ld = gauss_logdens(y, mean, var, s, w)
    sq = np.sum((y - mean) ** 2, axis=1)
    chi = sq / (np.asarray(var).reshape(-1) + noise_of(w, s))
    gl, gs, gc = row_gates(y, mean, var, s, w)
    vals = [float(pos.sum()), np.sum(ld[pos]), np.sum(sq[pos]), np.sum(chi[pos])]
    gates = [0.0] + [np.sum(g[pos]) + 1e-12 * np.sum(np.abs(t[pos])) for g, t in ((gl, ld), (gs, sq), (gc, chi))]
    return vals, gates


def check_sums(tag, sc, vals, gates):
    assert sc["n"] == vals[0], (tag, sc["n"], vals[0])
    for key, v, g in zip(("log_density", "sq_err", "chi2"), vals[1:], gates[1:]):
        assert report(tag + " " + key + " (over the summed first-order image of 1e-8)", abs(sc[key] - v), g) <= 1.0


def check_derived(sc, D):
    n = sc["n"]
    assert all(isinstance(sc[k], float) for k in ("n", "log_density", "sq_err", "chi2", "nlpd", "rmse", "mean_chi2"))
    assert sc["nlpd"] == -sc["log_density"] / n and sc["rmse"] == math.sqrt(sc["sq_err"] / (n * D)) and sc["mean_chi2"] == sc["chi2"] / (n * D)


def check_logdens_own(tag, ld, y, mean, var, s, w):
    ref = gauss_logdens(y, mean, var, s, w)
    assert report(tag + " logdens vs the Gaussian formula on the kernel's own moments",
                  np.max(np.abs(ld - ref) / np.maximum(1.0, np.abs(ref))), 1.0) <= 1e-12


def check_scores_own(tag, sc, ld, y, mean, var, s, w):
    """scores = [n, sum logdens, sum sq, sum chi2] against float sums of the per-row outputs over the rows with w > 0"""
    pos = w > 0
    assert sc[0] == pos.sum()
    sq = np.sum((y - mean) ** 2, axis=1)
    chi = sq / (np.asarray(var).reshape(-1) + noise_of(w, s))
    for name, got, terms in (("sum logdens", sc[1], ld[pos]), ("sum squared error", sc[2], sq[pos]), ("sum chi2", sc[3], chi[pos])):
        assert report(tag + " scores: " + name, abs(got - np.sum(terms)), max(np.sum(np.abs(terms)), 1e-300)) <= 1e-12


def dense_1d(ob, kind, v, l, s, x, y, w):
    return Dense(ob.evaluate_basis(x.reshape(-1, 1), sparse=True), O.band_to_dense_sym(O.make_Kuu(ob, kind, v, l)), v, s, y, w)


def khatri_rao_sparse(obases, X):
    """sparse (m1 m2, N) Khatri-Rao design matrix, dim-0 major"""
    import scipy.sparse as sp
    P1 = obases[0].evaluate_basis(X[:, :1], sparse=False)
    P2 = obases[1].evaluate_basis(X[:, 1:], sparse=False)
    return sp.csr_matrix((P1[:, None, :] * P2[None, :, :]).reshape(-1, X.shape[0]))


def banded_yardstick(ob, kind, v, l, s, x, y, w, xnew):
    """(mu, var) at xnew through band quantities only, as O.predict_f_1d_banded: band(P^-1), band(Kuu^-1) and alpha from the oracle's band
    Cholesky / selected inverse / triangular solves on the directly accumulated weighted statistics of the training rows (x, y, w)."""
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
    idx = O.neighbour_index(ob.mesh, xnew)
    vals = O.piece_values(k, (xnew - ob.mesh[idx]) / ob.delta)
    mu = np.zeros((xnew.shape[0], y.shape[1]))
    q = np.zeros(xnew.shape[0])
    for i in range(k + 1):
        ri = idx + k - i
        mu += vals[i][:, None] * alpha[ri]
        for j in range(k + 1):
            rj = idx + k - j
            hi, lo = np.maximum(ri, rj), np.minimum(ri, rj)
            q += vals[i] * vals[j] * (SP[hi - lo, lo] - SK[hi - lo, lo])
    return mu, v + q


def sliced(t, off):
    """a copy of t that starts 8 * off bytes into a fresh 16-byte aligned allocation"""
    buf = torch.zeros(t.numel() + off, dtype=torch.float64, device="cuda")
    buf[off:] = t.reshape(-1)
    out = buf[off:]
    if off:
        assert out.data_ptr() % 16 == 8
    return out


class Guarded:
    """an output of n doubles inside a sentinel-filled allocation (8 bytes into a 16-byte slot when off = 1): whatever the call does not
    own must still hold the sentinel afterwards"""
    SENTINEL = 7.0

    def __init__(self, n, off):
        self.n, self.start = n, 1 if off else 2
        self.buf = torch.full((n + 4,), self.SENTINEL, dtype=torch.float64, device="cuda")
        self.view = self.buf[self.start:self.start + n]
        assert self.view.data_ptr() % 16 == (8 if off else 0)

    def result(self, asked):
        b = self.buf.cpu().numpy()
        assert np.all(b[:self.start] == self.SENTINEL) and np.all(b[self.start + self.n:] == self.SENTINEL)
        if not asked:
            assert np.all(b == self.SENTINEL)
            return None
        return b[self.start:self.start + self.n].copy()


def score_call(model, xt, yt, wt, N, D, want="mvls", off=0):
    """asvgp_score_1d through the C-ABI on device tensors (any alignment) with the model's tables -> dict of numpy outputs.  Every output
    has a sentinel-filled buffer; the ones not asked for are passed as NULL and must stay untouched, as must the guards of the others."""
    from asvgp_amd import _lib
    lib = _lib.get_lib()
    alpha, W = model._posterior()
    b = model.basis
    ws = torch.empty(lib.asvgp_score_workspace_bytes(b.m, b.order, D) // 8, dtype=torch.float64, device="cuda")
    out = {c: Guarded(n, off) for c, n in (("m", N * D), ("v", N), ("l", N), ("s", 4))}
    ptr = lambda c: out[c].view.data_ptr() if c in want else None
    tp = lambda t: None if t is None else t.data_ptr()
    rc = lib.asvgp_score_1d(model._h.ptr, tp(xt), tp(yt), tp(wt), N, D, b.mesh.data_ptr(), b.mesh.shape[0], b.delta_np, b.order, b.m,
                            alpha.data_ptr(), W.data_ptr(), float(model.kernel.variance), float(model.likelihood.variance),
                            ptr("m"), ptr("v"), ptr("l"), ptr("s"), ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.asvgp_last_error_string().decode()
    res = {c: g.result(c in want) for c, g in out.items()}
    if res["m"] is not None:
        res["m"] = res["m"].reshape(N, D)
    return res


def problem_1d(seed, order, kind, M, N, D, s, weights=True, f32mesh=False, l=0.2, v=1.2, n_new=150, layout="unsorted", new_weights=True):
    rng = np.random.default_rng(seed)
    x = make_x(rng, N)
    y = make_y(rng, x, D)
    w = lognormal_weights(rng, N) if weights else None
    xn = make_x(rng, n_new, layout)
    yn = make_y(rng, xn, D)
    wn = lognormal_weights(rng, n_new) if new_weights else None
    if wn is not None and n_new <= 2:
        wn[:] = 1.7
    a, b = (0.0, 1.0) if f32mesh else (0, 1)
    return dict(order=order, kind=kind, M=M, N=N, D=D, s=s, l=l, v=v, x=x, y=y, w=w, ab=(a, b), xn=xn, yn=yn, wn=wn)


def build_1d(A, p, w="own", x=None, y=None, **kw):
    w = p["w"] if isinstance(w, str) else w
    x, y = (p["x"], p["y"]) if x is None else (x, y)
    m = A.GPR_1d((x.reshape(-1, 1), y), getattr(A, KNAMES[p["kind"]])(variance=p["v"], lengthscales=p["l"]),
                 getattr(A, "B%dSpline" % p["order"])(p["ab"][0], p["ab"][1], p["M"]), weights=w, **kw)
    m.likelihood.variance.assign(p["s"])
    return m


def obasis(p):
    return O.Basis(p["order"], p["ab"][0], p["ab"][1], p["M"])


def ones_if_none(w, n):
    return np.ones(n) if w is None else w


def yardstick_1d(p, xnew, x=None, y=None, w=None):
    """(mu, var) of the dense posterior of the training rows (default: the problem's) at xnew"""
    x, y, w = (p["x"], p["y"], p["w"]) if x is None else (x, y, w)
    ob = obasis(p)
    ref = dense_1d(ob, p["kind"], p["v"], p["l"], p["s"], x, y, ones_if_none(w, x.shape[0]))
    mu, _, var = ref.at(ob.evaluate_basis(xnew.reshape(-1, 1), sparse=True))
    return mu, var


# ------------------------------------------------------------------------------------------------ 1. formula, 1-D, small
CASE1 = [(4, 1, 40, 400, 1, 0.03), (3, 2, 30, 300, 2, 0.05), (2, 0, 25, 200, 1, 0.03)]


@pytest.mark.parametrize("trained_weighted", [True, False])
@pytest.mark.parametrize("case", range(len(CASE1)))
def test_formula_1d(A, case, trained_weighted):
    order, kind, M, N, D, s = CASE1[case]
    p = problem_1d(100 + case, order, kind, M, N, D, s, weights=trained_weighted)
    model = build_1d(A, p)
    xn, yn = p["xn"], p["yn"]
    mu, var = yardstick_1d(p, xn)
    tag0 = "1-D k=%d %s M=%d N=%d D=%d%s" % (order, KNAMES[kind], M, N, D, " trained weighted" if trained_weighted else "")
    pm, pv = (t.cpu().numpy() for t in model.predict_f_device(xn.reshape(-1, 1)))
    xt, yt = dev(xn), dev(yn)
    for wn in (p["wn"], None):
        tag = tag0 + (" held-out weighted" if wn is not None else "")
        w = ones_if_none(wn, xn.shape[0])
        if wn is not None:
            assert (w == 0).sum() > 0
        full = score_call(model, xt, yt, None if wn is None else dev(wn), xn.shape[0], D)
        assert report(tag + " mean vs yardstick", np.max(np.abs(full["m"] - mu)), GATE) <= 1.0
        assert report(tag + " variance vs yardstick", np.max(np.abs(full["v"] - var)), GATE) <= 1.0
        assert report(tag + " mean vs predict_f_device", np.max(np.abs(full["m"] - pm)), GATE) <= 1.0
        assert report(tag + " variance vs predict_f_device", np.max(np.abs(full["v"] - pv.reshape(-1))), GATE) <= 1.0
        ld_t = model.predict_log_density_device((xn.reshape(-1, 1), yn), weights=wn)
        assert ld_t.is_cuda and ld_t.shape == (xn.shape[0],)
        ld = ld_t.cpu().numpy()
        assert np.array_equal(ld, full["l"])
        check_logdens_own(tag, ld, yn, full["m"], full["v"], s, w)
        assert report(tag + " logdens vs the yardstick's (over the first-order image of 1e-8)",
                      np.max(np.abs(ld - gauss_logdens(yn, mu, var, s, w)) / logdens_gate(yn, mu, var, s, w)), 1.0) <= 1.0
        sc = model.score((xn.reshape(-1, 1), yn), weights=wn)
        check_derived(sc, D)
        arr = [sc["n"], sc["log_density"], sc["sq_err"], sc["chi2"]]
        assert np.array(arr).tobytes() == full["s"].tobytes()
        check_scores_own(tag, arr, ld, yn, full["m"], full["v"], s, w)
        check_sums(tag + " score vs yardstick:", sc, *score_sums(yn, mu, var, s, w))
        assert sc["n"] == (w > 0).sum()
        # the device forms of predict_y / predict_log_density against the existing host routes (which take positive weights only)
        pos = w > 0
        wp = None if wn is None else wn[pos]
        ym, yv = model.predict_y_device(xn[pos].reshape(-1, 1), weights=wp)
        hm, hv = model.predict_y(xn[pos].reshape(-1, 1), weights=wp)
        assert ym.is_cuda and yv.is_cuda and ym.shape == (pos.sum(), D) and yv.shape == (pos.sum(), 1)
        assert np.array_equal(ym.cpu().numpy(), np.asarray(hm))
        assert report(tag + " predict_y_device variance vs predict_y (relative)", np.max(np.abs(yv.cpu().numpy() - np.asarray(hv)) / np.asarray(hv)), 1.0) <= 1e-15
        hl = np.asarray(model.predict_log_density((xn[pos].reshape(-1, 1), yn[pos]), weights=wp))
        assert report(tag + " predict_log_density_device vs predict_log_density", np.max(np.abs(ld[pos] - hl) / np.maximum(1.0, np.abs(hl))), 1.0) <= 1e-12
        if wn is not None:      # a row with weight 0 takes noise variance sigma2
            zv = model.predict_y_device(xn[~pos].reshape(-1, 1), weights=wn[~pos])[1].cpu().numpy()
            assert np.array_equal(zv, pv[~pos] + s)


# ------------------------------------------------------------------------------------------------ 2. kernel shapes through the C-ABI
# (order, M, N, D, layout, weighted, sliced 8 bytes into a 16-byte allocation?, float32-linspace mesh?)
SHAPES = [
    (2, 8, 1, 1, "unsorted", True, False, False),
    (2, 8, 2, 1, "unsorted", False, False, False),
    (1, 12, 1031, 3, "unsorted", True, False, False),
    (2, 12, 1031, 3, "clustered", False, True, False),
    (3, 40, 4099, 3, "sorted", True, True, False),
    (4, 40, 4099, 3, "clustered", True, False, False),
    (5, 257, 20_001, 3, "unsorted", False, False, True),
    (6, 40, 4099, 3, "clustered", True, False, False),
    # the thresholds of the launch plan, from both sides
    (4, 40, STAGE_MIN_N - 1, 1, "unsorted", True, False, False),      # tables through the caches
    (4, 40, STAGE_MIN_N, 1, "unsorted", True, True, False),           # staged, 1024 threads
    (4, 40, WRAP_N, 1, "unsorted", False, False, False),              # the largest grid that does not wrap
    (4, 40, WRAP_N + 1, 2, "sorted", True, False, False),             # one row past it
    (6, 40, STAGE_MIN_N + 4465, 1, "unsorted", True, False, False),   # staged, 512 threads (orders 5 and 6)
    (4, 2048, STAGE_MIN_N + 4465, 1, "unsorted", True, False, False), # the headline's tables: staged whole
    (4, 2907, STAGE_MIN_N + 4465, 1, "unsorted", True, False, False), # the largest tables staged whole
    (4, 2908, STAGE_MIN_N + 4465, 1, "clustered", False, False, False), # two ranges of cells
    (3, 4500, STAGE_MIN_N, 3, "clustered", True, True, False),        # several ranges, D = 3, a short last range, ranges without rows
    (6, 3500, WRAP_N + 1, 3, "unsorted", False, False, False),        # tables too large for two ranges: not staged, and the grid wraps
]
N_TRAIN_SHAPES = 700


@pytest.mark.parametrize("order,M,N,D,layout,weighted,unaligned,f32mesh", SHAPES)
def test_kernel_shapes_1d(A, order, M, N, D, layout, weighted, unaligned, f32mesh):
    # (order 5 takes Matern-5/2; the order-6 basis carries the static bands of Matern-1/2 and 3/2 only, as the reference's does)
    kind = 2 if order == 5 else (0 if order <= 2 else 1)
    p = problem_1d(1000 * order + M + N, order, kind, M, N_TRAIN_SHAPES, D, 0.05, weights=True, f32mesh=f32mesh,
                   l=0.2 if M < 1000 else 20.0 / M, n_new=N, layout=layout, new_weights=weighted)
    model = build_1d(A, p)
    xn, yn, s = p["xn"], p["yn"], p["s"]
    w = ones_if_none(p["wn"], N)
    if M >= 1000:                             # (two dense M x M inverses take seconds here: the same formulas on the oracle's band routines)
        mu, var = banded_yardstick(obasis(p), kind, p["v"], p["l"], s, p["x"], p["y"], p["w"], xn)
    else:
        mu, var = yardstick_1d(p, xn)
    tag = "shape k=%d M=%d N=%d D=%d %s%s%s%s" % (order, M, N, D, layout, " weighted" if weighted else "", " unaligned" if unaligned else "",
                                                  " f32 mesh" if f32mesh else "")
    off = 1 if unaligned else 0
    xt, yt = sliced(dev(xn), off), sliced(dev(yn), off)
    wt = sliced(dev(p["wn"]), off) if weighted else None
    full = score_call(model, xt, yt, wt, N, D, "mvls", off)
    assert report(tag + " mean vs yardstick", np.max(np.abs(full["m"] - mu)), GATE) <= 1.0
    assert report(tag + " variance vs yardstick", np.max(np.abs(full["v"] - var)), GATE) <= 1.0
    check_logdens_own(tag, full["l"], yn, full["m"], full["v"], s, w)
    assert report(tag + " logdens vs the yardstick's (over the first-order image of 1e-8)",
                  np.max(np.abs(full["l"] - gauss_logdens(yn, mu, var, s, w)) / logdens_gate(yn, mu, var, s, w)), 1.0) <= 1.0
    check_scores_own(tag, full["s"], full["l"], yn, full["m"], full["v"], s, w)
    only = score_call(model, xt, yt, wt, N, D, "s", off)              # scores only: nothing of size N is written
    again = score_call(model, xt, yt, wt, N, D, "mvls", off)
    assert only["s"].tobytes() == full["s"].tobytes() == again["s"].tobytes()
    assert all(again[c].tobytes() == full[c].tobytes() for c in "mvl")
    mix = score_call(model, xt, yt, wt, N, D, "ml", off)              # var and scores NULL
    assert np.array_equal(mix["m"], full["m"]) and np.array_equal(mix["l"], full["l"])
    one = score_call(model, xt, yt, wt, N, D, "v", off)               # a single per-row output
    assert np.array_equal(one["v"], full["v"])


def test_empty_batch_zeroes_scores(A):
    p = problem_1d(5, 4, 1, 40, 50, 1, 0.05)
    model = build_1d(A, p)
    got = score_call(model, None, None, None, 0, 1, "s")
    assert np.array_equal(got["s"], np.zeros(4))
    sc = model.score((np.zeros((0, 1)), np.zeros((0, 1))))
    assert sc["n"] == 0 and sc["log_density"] == 0 and all(math.isnan(sc[k]) for k in ("nlpd", "rmse", "mean_chi2"))


# ------------------------------------------------------------------------------------------------ 3. Kronecker (d = 2)
KRON_TH, KRON_S = [(1.1, 0.3), (0.7, 0.6)], 0.05


def kron_problem(order, m1, m2, N, weighted=True, n_new=500):
    rng = np.random.default_rng(m1 * 100 + m2 + 7)
    def draw(n):
        X = np.stack([rng.uniform(0.03, 0.97, n), rng.uniform(-0.91, 1.91, n)], axis=1)
        return X, np.sin(12 * X[:, :1]) * np.cos(3 * X[:, 1:]) + 0.1 * rng.normal(size=(n, 1))
    X, y = draw(N)
    w = lognormal_weights(rng, N) if weighted else None
    Xn, yn = draw(n_new)
    return X, y, w, Xn, yn, lognormal_weights(rng, n_new)


def build_kron(A, order, m1, m2, X, y, w, **kw):
    B = getattr(A, "B%dSpline" % order)
    kerns = [A.Matern32(variance=KRON_TH[0][0], lengthscales=KRON_TH[0][1]), A.Matern32(variance=KRON_TH[1][0], lengthscales=KRON_TH[1][1])]
    model = A.GPR_kron((X, y), kerns, [B(0, 1, m1), B(-1, 2, m2)], weights=w, **kw)
    model.likelihood.variance.assign(KRON_S)
    return model


def kron_yardstick(order, m1, m2, X, y, w, Xn):
    obases = [O.Basis(order, 0, 1, m1), O.Basis(order, -1, 2, m2)]
    Ks = [O.band_to_dense_sym(O.make_Kuu(bs, 1, v, l)) for bs, (v, l) in zip(obases, KRON_TH)]
    ref = Dense(khatri_rao_sparse(obases, X), np.kron(Ks[0], Ks[1]), float(np.prod([v for v, _ in KRON_TH])), KRON_S, y, ones_if_none(w, X.shape[0]))
    mu, _, var = ref.at(khatri_rao_sparse(obases, Xn))
    return mu, var


def check_composed(tag, model, Xn, yn, wn, s, mu=None, var=None):
    """score / predict_log_density_device / predict_y_device of a model that composes them from its own predict_f_device: the Gaussian
    formula on those moments (1e-12 rule), and, where a yardstick is given, the yardstick's gates"""
    n, D = Xn.shape[0], yn.shape[1]
    w = ones_if_none(wn, n)
    pm, pv = (t.cpu().numpy() for t in model.predict_f_device(Xn))
    ld_t = model.predict_log_density_device((Xn, yn), weights=wn)
    assert ld_t.is_cuda and ld_t.shape == (n,)
    ld = ld_t.cpu().numpy()
    check_logdens_own(tag, ld, yn, pm, pv, s, w)
    ym, yv = (t.cpu().numpy() for t in model.predict_y_device(Xn, weights=wn))
    assert np.array_equal(ym, pm) and np.array_equal(yv, pv + noise_of(w, s)[:, None] if wn is not None else pv + s)
    sc = model.score((Xn, yn), weights=wn)
    check_derived(sc, D)
    check_scores_own(tag, [sc["n"], sc["log_density"], sc["sq_err"], sc["chi2"]], ld, yn, pm, pv, s, w)
    if mu is not None:
        assert report(tag + " mean vs yardstick", np.max(np.abs(pm - mu)), GATE) <= 1.0
        assert report(tag + " variance vs yardstick", np.max(np.abs(pv.reshape(-1) - var)), GATE) <= 1.0
        assert report(tag + " logdens vs the yardstick's (over the first-order image of 1e-8)",
                      np.max(np.abs(ld - gauss_logdens(yn, mu, var, s, w)) / logdens_gate(yn, mu, var, s, w)), 1.0) <= 1.0
        check_sums(tag + " score vs yardstick:", sc, *score_sums(yn, mu, var, s, w))
    return sc


@pytest.mark.parametrize("order,m1,m2", [(3, 12, 14), (4, 14, 16)])
def test_kron_formula(A, order, m1, m2):
    """Both grids are below the 3 super-blocks per side that the two-sided factorisation needs (tests/test_loo.py::test_kron_both_layouts),
    so _twist_layout() can only choose the one-sided layout here, forced or not; both settings are run and must agree to the bit."""
    X, y, w0, Xn, yn, wn = kron_problem(order, m1, m2, 3000)
    model = build_kron(A, order, m1, m2, X, y, w0)
    mu, var = kron_yardstick(order, m1, m2, X, y, w0, Xn)
    got = []
    for tw in (False, True):
        model.twisted = tw
        model._post = None
        assert model._twist_layout() is None
        tag = "kron k=%d %dx%d N=3000 twisted=%s" % (order, m1, m2, tw)
        got.append(check_composed(tag + " held-out weighted", model, Xn, yn, wn, KRON_S, mu, var))
        check_composed(tag, model, Xn, yn, None, KRON_S, mu, var)
    for key in ("n", "log_density", "sq_err", "chi2"):
        assert report("kron %dx%d both settings agree: %s" % (m1, m2, key), abs(got[0][key] - got[1][key]), abs(got[1][key])) <= 1e-12


# ------------------------------------------------------------------------------------------------ 4. the models that compose, and refuse
def test_fallback_models(A):
    rng = np.random.default_rng(1)
    X3 = rng.uniform(0.01, 0.99, (100, 3))
    y = np.sin(9 * X3[:, :1])
    Xn = rng.uniform(0.01, 0.99, (60, 3))
    yn = np.sin(9 * Xn[:, :1]) + 0.1 * rng.normal(size=(60, 1))
    wn = lognormal_weights(rng, 60)
    add = A.GPR_additive((X3[:, :2], y), [A.Matern32(), A.Matern32()], [A.B3Spline(0, 1, 10), A.B3Spline(0, 1, 11)])
    k3 = A.GPR_kron((X3, y), [A.Matern32()] * 3, [A.B3Spline(0, 1, 10)] * 3)
    for name, model, Xh in (("GPR_additive", add, Xn[:, :2]), ("GPR_kron d=3", k3, Xn)):
        s = float(model.likelihood.variance)
        check_composed(name + " held-out weighted", model, Xh, yn, wn, s)
        check_composed(name, model, Xh, yn, None, s)
        with pytest.raises(NotImplementedError, match="set_weights"):
            model.set_weights(np.ones(100))
        with pytest.raises(NotImplementedError, match="kfold_scores"):
            model.kfold_scores(np.arange(100) % 2)


# ------------------------------------------------------------------------------------------------ 5. set_weights
def compare_models(tag, m, fresh, Xn, grad, y, w, s, weight_sum_exact=True):
    s0, s1 = m._stats.cpu().numpy(), fresh._stats.cpu().numpy()
    assert report(tag + " statistics", np.max(np.abs(s0 - s1)), np.max(np.abs(s1))) <= 1e-12
    assert m.num_data == fresh.num_data
    if weight_sum_exact:
        assert m.weight_sum == fresh.weight_sum
    assert report(tag + " log_weight_sum", abs(m.log_weight_sum - fresh.log_weight_sum), max(abs(fresh.log_weight_sum), 1.0)) <= 1e-12
    e0, g0 = grad(m)
    e1, g1 = grad(fresh)
    assert report(tag + " ELBO", abs(e0 - e1), abs(e1)) <= 1e-9
    np.testing.assert_allclose(g0, g1, rtol=1e-6)
    for a, b, name in zip(m.predict_f_device(Xn), fresh.predict_f_device(Xn), ("mean", "variance")):
        assert report(tag + " predict_f_device " + name, float((a - b).abs().max()), GATE) <= 1.0
    # leave-one-out: rows at 1e-8 (no wider than the delta_i of tests/test_loo.py), the sums at the summed first-order images of 1e-8
    (m0, v0), (m1, v1) = ([t.cpu().numpy() for t in mm.loo_predict_f_device()] for mm in (m, fresh))
    assert report(tag + " loo rows: mean", np.max(np.abs(m0 - m1)), GATE) <= 1.0
    assert report(tag + " loo rows: variance", np.max(np.abs(v0 - v1)), GATE) <= 1.0
    l0, l1 = m.loo_scores(), fresh.loo_scores()
    assert l0["n"] == l1["n"]
    gl, gs, _ = row_gates(y, m1, v1.reshape(-1), s, w)
    pos = w > 0
    assert report(tag + " loo_scores log_density", abs(l0["log_density"] - l1["log_density"]), np.sum(gl[pos]) + 1e-12 * abs(l1["log_density"])) <= 1.0
    assert report(tag + " loo_scores sq_err", abs(l0["sq_err"] - l1["sq_err"]), np.sum(gs[pos]) + 1e-12 * abs(l1["sq_err"])) <= 1.0
    assert report(tag + " loo_scores max_leverage", abs(l0["max_leverage"] - l1["max_leverage"]), 1.0) <= 1e-6


@pytest.mark.parametrize("D", [1, 2])
def test_set_weights_1d(A, D):
    """D = 1 takes the register-moment weighted Phi pass, D = 2 the band-scatter one"""
    p = problem_1d(50 + D, 4, 1, 64, 3000, D, 0.04)
    rng = np.random.default_rng(9)
    w2 = lognormal_weights(rng, p["N"])
    model = build_1d(A, p)
    model.predict_f_device(p["xn"].reshape(-1, 1)), model.loo_scores()             # (fill the theta-keyed caches that must be dropped)
    handle, stats, wt = model._h, model._stats, model.weights
    model.set_weights(w2.reshape(-1, 1))
    assert model._h is handle and model._stats is stats and model.weights is wt and np.array_equal(wt.cpu().numpy(), w2)
    assert model._post is None and model._post_loo is None and model._post_cov is None
    fresh = build_1d(A, p, w=w2)
    grad = lambda m: (lambda r: (r[0], r[1:4]))(m.elbo_and_grad().cpu().numpy())
    compare_models("set_weights GPR_1d D=%d" % D, model, fresh, p["xn"].reshape(-1, 1), grad, p["y"], w2, p["s"])
    # loud failures leave the model unchanged
    before = (model._stats.clone(), model.weights.clone(), model.num_data, model.weight_sum, model.log_weight_sum)
    bad = w2.copy()
    bad[17] = np.nan
    with pytest.raises(ValueError, match="row 17"):
        model.set_weights(bad)
    with pytest.raises(ValueError, match="shape"):
        model.set_weights(w2[:-1])
    assert torch.equal(model._stats, before[0]) and torch.equal(model.weights, before[1])
    assert (model.num_data, model.weight_sum, model.log_weight_sum) == before[2:]
    plain = build_1d(A, p, w=None)
    with pytest.raises(ValueError, match="without weights"):
        plain.set_weights(w2)


def test_set_weights_kron(A):
    X, y, w1, Xn, _, _ = kron_problem(3, 11, 10, 4000)
    w2 = lognormal_weights(np.random.default_rng(10), 4000)
    model = build_kron(A, 3, 11, 10, X, y, w1)
    model.predict_f_device(Xn)
    sorted_before = model._sorted
    Xs, perm = model._sorted[0], model._sort_perm
    model.set_weights(w2)
    assert model._sorted is sorted_before and model._sorted[0] is Xs and model._sort_perm is perm       # reused, not rebuilt
    assert np.array_equal(model._sorted[3].cpu().numpy(), w2[perm.cpu().numpy()]) and model._post is None
    fresh = build_kron(A, 3, 11, 10, X, y, w2)
    grad = lambda m: (lambda r: (float(r[0]), np.asarray(r[1])))(m.elbo_and_grad())
    # (weight_sum's exact equality is test_set_weights_kron_weight_sum_equals_fresh_model's)
    compare_models("set_weights GPR_kron 11x10", model, fresh, Xn, grad, y, w2, KRON_S, weight_sum_exact=False)
    bad = w2.copy()
    bad[5] = -1.0
    before = model._stats.clone()
    with pytest.raises(ValueError, match="row 5"):
        model.set_weights(bad)
    assert torch.equal(model._stats, before) and np.array_equal(model.weights.cpu().numpy(), w2)
    with pytest.raises(ValueError, match="without weights"):
        build_kron(A, 3, 11, 10, X, y, None).set_weights(w2)


def test_set_weights_kron_weight_sum_equals_fresh_model(A):
    """Exact equality of weight_sum between GPR_kron.set_weights(w2) and a fresh GPR_kron built with w2, as the issue sets it.  It holds
    only when the two weighted Phi passes add up sum w in the same order, and they need not: the Kronecker weighted kernels
    (csrc/kron_weighted.hpp) add every workgroup's partial sum of w into wstats with a floating-point atomic, in arrival order, so even two
    fresh builds of the SAME model can differ in the last bit.  set_weights runs that very kernel on the very same sorted rows; nothing in
    it can fix the order of another launch's atomics.  Measured on one MI355X in three runs of the same build: equal in two;
    5467.110999027443 after set_weights against 5467.110999027442 fresh (one ulp, 1.7e-16 relative) in the other.  num_data (a sum of
    ones: exact in any order) is equal every time, and GPR_1d's sums, reduced in a fixed order, are too (test_set_weights_1d).  This
    test fails whenever the last bit shows."""
    X, y, w1, _, _, _ = kron_problem(3, 11, 10, 4000)
    w2 = lognormal_weights(np.random.default_rng(10), 4000)
    model = build_kron(A, 3, 11, 10, X, y, w1)
    model.set_weights(w2)
    fresh = build_kron(A, 3, 11, 10, X, y, w2)
    report("set_weights GPR_kron weight_sum - fresh model's (relative)", abs(model.weight_sum - fresh.weight_sum), fresh.weight_sum)
    assert model.num_data == fresh.num_data
    assert model.weight_sum == fresh.weight_sum


# ------------------------------------------------------------------------------------------------ 6. K-fold against explicit models
def model_state(m):
    th = [(p._u, p._value) for p in m.trainable_parameters]
    if m.weights is None:
        return (m._stats.clone(), None, None, m.num_data, th)
    return (m._stats.clone(), m.weights.clone(), m._wstats.clone(), (m.num_data, m.weight_sum, m.log_weight_sum), th)


def assert_state_unchanged(m, st):
    assert torch.equal(m._stats, st[0])
    if st[1] is not None:
        assert torch.equal(m.weights, st[1]) and torch.equal(m._wstats, st[2])
        assert (m.num_data, m.weight_sum, m.log_weight_sum) == st[3]
        if getattr(m, "_sorted", None) is not None and len(m._sorted) == 4:
            assert torch.equal(m._sorted[3], m.weights[m._sort_perm])
    else:
        assert m.num_data == st[3] and m.weights is None
    assert [(p._u, p._value) for p in m.trainable_parameters] == st[4]


def check_total(res):
    tot = res["total"]
    for key in ("n", "log_density", "sq_err", "chi2"):
        assert tot[key] == sum(f[key] for f in res["folds"])
    assert tot["nlpd"] == -tot["log_density"] / tot["n"]


@pytest.mark.parametrize("weighted", [True, False])
def test_kfold_1d_against_explicit_models(A, weighted):
    N, M, K = 3000, 64, 5
    p = problem_1d(60, 4, 1, M, N, 1, 0.04, weights=weighted)
    rng = np.random.default_rng(61)
    folds = rng.integers(0, K, N)
    model = build_1d(A, p)
    st = model_state(model)
    res = model.kfold_scores(folds)
    assert_state_unchanged(model, st)
    assert len(res["folds"]) == K
    check_total(res)
    w = ones_if_none(p["w"], N)
    for f in range(K):
        tr, te = folds != f, folds == f
        tag = "k-fold GPR_1d%s fold %d" % (" weighted" if weighted else "", f)
        mu, var = yardstick_1d(p, p["x"][te], p["x"][tr], p["y"][tr], w[tr])
        vals, gates = score_sums(p["y"][te], mu, var, p["s"], w[te])
        check_sums(tag + " vs the dense posterior of the complement:", res["folds"][f], vals, gates)
        check_derived(res["folds"][f], 1)
        fresh = build_1d(A, p, w=w[tr] if weighted else None, x=p["x"][tr], y=p["y"][tr])
        sc = fresh.score((p["x"][te].reshape(-1, 1), p["y"][te]), weights=w[te] if weighted else None)
        check_sums(tag + " vs a fresh model on the complement:", res["folds"][f], [sc["n"], sc["log_density"], sc["sq_err"], sc["chi2"]], gates)
    # a call that raises restores the model as well: one fold's P is not positive definite (tests/test_loo.py::test_loud_failures)
    from asvgp_amd.banded import NotPositiveDefiniteError
    if weighted:
        calls = []
        orig = model._apply_weights

        def sabotage(wt):
            orig(wt)
            calls.append(1)
            if len(calls) == 2:
                model._stats[20] = -1.0e9                                # diagonal entry 20 of the second fold's KufKfu band
        model._apply_weights = sabotage
        with pytest.raises(NotPositiveDefiniteError):
            model.kfold_scores(folds)
        del model._apply_weights
        assert len(calls) == 2
        assert_state_unchanged(model, st)
        again = model.kfold_scores(folds)
        for a, b in zip(again["folds"], res["folds"]):
            assert a["n"] == b["n"] and abs(a["log_density"] - b["log_density"]) <= 1e-9 * abs(b["log_density"])


def test_kfold_kron_against_explicit_models(A):
    order, m1, m2, N, K = 3, 11, 10, 4000, 4
    X, y, w, _, _, _ = kron_problem(order, m1, m2, N)
    folds = np.random.default_rng(62).integers(0, K, N)
    model = build_kron(A, order, m1, m2, X, y, w)
    st = model_state(model)
    res = model.kfold_scores(torch.as_tensor(folds))
    assert_state_unchanged(model, st)
    check_total(res)
    for f in range(K):
        tr, te = folds != f, folds == f
        tag = "k-fold GPR_kron 11x10 fold %d" % f
        mu, var = kron_yardstick(order, m1, m2, X[tr], y[tr], w[tr], X[te])
        vals, gates = score_sums(y[te], mu, var, KRON_S, w[te])
        check_sums(tag + " vs the dense posterior of the complement:", res["folds"][f], vals, gates)
        sc = build_kron(A, order, m1, m2, X[tr], y[tr], w[tr]).score((X[te], y[te]), weights=w[te])
        check_sums(tag + " vs a fresh model on the complement:", res["folds"][f], [sc["n"], sc["log_density"], sc["sq_err"], sc["chi2"]], gates)
    # unweighted: the internal twin; the model itself is not touched
    plain = build_kron(A, order, m1, m2, X, y, None)
    stp = model_state(plain)
    resp = plain.kfold_scores(folds)
    assert_state_unchanged(plain, stp)
    mu, var = kron_yardstick(order, m1, m2, X[folds != 0], y[folds != 0], None, X[folds == 0])
    check_sums("k-fold GPR_kron 11x10 unweighted fold 0 vs the dense posterior:", resp["folds"][0], *score_sums(y[folds == 0], mu, var, KRON_S, np.ones((folds == 0).sum())))
    from asvgp_amd.banded import NotPositiveDefiniteError
    orig = model._apply_weights

    def sabotage(wt):
        orig(wt)
        model._stats[:model.noff * model.Mtot].mul_(-1.0)
    model._apply_weights = sabotage
    with pytest.raises(NotPositiveDefiniteError):
        model.kfold_scores(folds)
    del model._apply_weights
    assert_state_unchanged(model, st)


# ------------------------------------------------------------------------------------------------ 7. K = N is leave-one-out
def test_kfold_with_one_row_per_fold_is_leave_one_out(A):
    N, M, order, s = 200, 25, 3, 0.05
    p = problem_1d(70, order, 1, M, N, 1, s)
    p["w"] = lognormal_weights(np.random.default_rng(71), N, zeros=False)
    model = build_1d(A, p)
    loo = model.loo_scores()
    tot = model.kfold_scores(np.arange(N))["total"]
    assert tot["n"] == loo["n"] == N
    # the summed per-row gates of tests/test_loo.py: delta_i = 1e-8 / (1 - h_i)^2 on the leave-one-out mean and variance
    ob = obasis(p)
    Phi = ob.evaluate_basis(p["x"].reshape(-1, 1), sparse=True)
    ref = dense_1d(ob, 1, p["v"], p["l"], s, p["x"], p["y"], p["w"])
    mu, g, var = ref.at(Phi)
    h = p["w"] * g / s
    mean = (mu - h[:, None] * p["y"]) / (1 - h)[:, None]
    vloo = var + g * h / (1 - h)
    gl, gs, _ = row_gates(p["y"], mean, vloo, s, p["w"], GATE / (1 - h) ** 2)
    report("K = N: yardstick max leverage", np.max(h), 1.0)
    assert report("K = N: log_density vs loo_scores (over the summed per-row gates)", abs(tot["log_density"] - loo["log_density"]), np.sum(gl)) <= 1.0
    assert report("K = N: sq_err vs loo_scores (over the summed per-row gates)", abs(tot["sq_err"] - loo["sq_err"]), np.sum(gs)) <= 1.0


# ------------------------------------------------------------------------------------------------ 8. refit on the Snelson fixture
def test_kfold_refit_snelson(A, S):
    X, Y = np.asarray(S["X"]), np.asarray(S["Y"])
    folds = np.arange(X.shape[0]) % 2
    model = A.GPR_1d((X, Y), A.Matern32(), A.B3Spline(-3.5, 10.5, 100))
    theta0 = model.theta()
    st = model_state(model)
    res = model.kfold_scores(folds, refit=True)
    assert model.theta() == theta0
    assert_state_unchanged(model, st)
    check_total(res)
    for f in range(2):
        other = A.GPR_1d((X[folds != f], Y[folds != f]), A.Matern32(), A.B3Spline(-3.5, 10.5, 100))
        other.fit()
        np.testing.assert_allclose(res["folds"][f]["theta"], other.theta(), rtol=5e-5)
        sc = other.score((X[folds == f], Y[folds == f]))
        assert sc["n"] == res["folds"][f]["n"] == (folds == f).sum()
        assert report("Snelson refit fold %d: log_density vs the fitted model of the other rows (absolute)" % f,
                      abs(res["folds"][f]["log_density"] - sc["log_density"]), 1e-6) <= 1.0


# ------------------------------------------------------------------------------------------------ 9. two ranks on one GPU over gloo
def shard_problem():
    p = problem_1d(2026, 4, 1, 256, 120_001, 1, 0.01, l=0.05, v=1.0, n_new=30_001)
    p["folds"] = np.random.default_rng(2027).integers(0, 3, p["N"])
    return p


def _score_shard_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)                       # both ranks share the one GPU of the test box; gloo moves the band
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import asvgp_amd as A
    from asvgp_amd.dist import shard_bounds
    p = shard_problem()
    lo, hi = shard_bounds(p["N"], world, rank)
    lo2, hi2 = shard_bounds(p["xn"].shape[0], world, rank)
    local = dict(p, x=p["x"][lo:hi], y=p["y"][lo:hi], w=p["w"][lo:hi], N=hi - lo)
    m = build_1d(A, local, process_group=dist.group.WORLD)
    sc = m.score((p["xn"][lo2:hi2].reshape(-1, 1), p["yn"][lo2:hi2]), weights=p["wn"][lo2:hi2])
    kf = m.kfold_scores(p["folds"][lo:hi] if rank == 0 else np.where(p["folds"][lo:hi] == 2, 1, p["folds"][lo:hi]))
    q.put((rank, sc, kf))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharded_score_and_kfold_match_single_rank(A):
    """(rank 1 holds no row of fold 2: K = 3 must come from the global maximum)"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 34600 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_score_shard_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = [q.get(timeout=300) for _ in procs]
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    from asvgp_amd.dist import shard_bounds
    p = shard_problem()
    lo, hi = shard_bounds(p["N"], 2, 1)
    folds = p["folds"].copy()
    folds[lo:hi] = np.where(folds[lo:hi] == 2, 1, folds[lo:hi])
    single = build_1d(A, p)
    s1 = single.score((p["xn"].reshape(-1, 1), p["yn"]), weights=p["wn"])
    k1 = single.kfold_scores(folds)
    assert sorted(r[0] for r in res) == [0, 1] and len(k1["folds"]) == 3

    def same(tag, a, b):
        assert a["n"] == b["n"]
        for key in ("log_density", "sq_err", "chi2"):
            assert report(tag + " " + key, abs(a[key] - b[key]), abs(b[key])) <= 1e-9

    for rank, sc, kf in res:
        same("two ranks (rank %d) score" % rank, sc, s1)
        assert len(kf["folds"]) == 3
        for f in range(3):
            same("two ranks (rank %d) k-fold fold %d" % (rank, f), kf["folds"][f], k1["folds"][f])
        same("two ranks (rank %d) k-fold total" % rank, kf["total"], k1["total"])
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]          # every rank returns the same global scores


# ------------------------------------------------------------------------------------------------ 10. loud failures
def test_loud_failures(A):
    p = problem_1d(80, 4, 1, 40, 400, 1, 0.03)
    model = build_1d(A, p)
    xn, yn, wn = p["xn"].reshape(-1, 1), p["yn"], p["wn"].copy()
    n = xn.shape[0]
    for name, args in (("score", ((xn, yn),)), ("predict_log_density_device", ((xn, yn),)), ("predict_y_device", (xn,))):
        for bad, word in ((-1.0, "row 3"), (float("nan"), "row 3")):
            wb = wn.copy()
            wb[3] = bad
            with pytest.raises(ValueError, match=word):
                getattr(model, name)(*args, weights=wb)
        with pytest.raises(ValueError, match="shape"):
            getattr(model, name)(*args, weights=wn[:-1])
    with pytest.raises(ValueError, match="Xnew"):
        model.score((np.zeros((n, 2)) + 0.5, yn))
    with pytest.raises(ValueError, match="Xnew"):
        model.predict_y_device(np.zeros((n, 2)) + 0.5)
    with pytest.raises(ValueError, match="Ynew"):
        model.score((xn, yn[:-1]))
    X2, y2, w2, Xn2, yn2, _ = kron_problem(3, 8, 9, 300, n_new=20)
    mk = build_kron(A, 3, 8, 9, X2, y2, w2)
    with pytest.raises(ValueError, match="Xnew"):
        mk.score((Xn2[:, :1], yn2))
    # folds: raised before anything is launched - the statistics are not even touched
    stats = model._stats.clone()
    for m_, nrow in ((model, 400), (mk, 300)):
        with pytest.raises(ValueError, match="shape"):
            m_.kfold_scores(np.zeros(nrow - 1, dtype=np.int64))
        bad = np.arange(nrow) % 3
        bad[7] = -1
        with pytest.raises(ValueError, match="row 7"):
            m_.kfold_scores(bad)
        with pytest.raises(ValueError, match="fold 1 has no row"):
            m_.kfold_scores(np.where(np.arange(nrow) % 2 == 0, 0, 3))
    only_zero = np.zeros(400, dtype=np.int64)
    only_zero[p["w"] == 0] = 1                                           # fold 1 holds rows of weight 0 only
    with pytest.raises(ValueError, match="fold 1 has no row of positive weight"):
        model.kfold_scores(only_zero)
    assert torch.equal(model._stats, stats)
    # a huge y in a row of weight 0 stays out of the scores; a NaN y in a counted row reaches them, and the row is still counted
    base = model.score((xn, yn), weights=wn)
    zero = int(np.flatnonzero(wn == 0)[0])
    y_big = yn.copy()
    y_big[zero] = 1e300
    sc = model.score((xn, y_big), weights=wn)
    assert sc == base and all(math.isfinite(sc[k]) for k in ("log_density", "sq_err", "chi2"))
    ld = model.predict_log_density_device((xn, y_big), weights=wn).cpu().numpy()
    assert not np.isfinite(ld[zero]) and np.all(np.isfinite(np.delete(ld, zero)))
    counted = int(np.flatnonzero(wn > 0)[0])
    y_nan = yn.copy()
    y_nan[counted] = np.nan
    sc = model.score((xn, y_nan), weights=wn)
    assert sc["n"] == base["n"] and math.isnan(sc["log_density"]) and math.isnan(sc["nlpd"])
    sck = mk.score((Xn2, np.where(np.arange(20)[:, None] == 4, np.nan, yn2)))
    assert sck["n"] == 20 and math.isnan(sck["log_density"])
