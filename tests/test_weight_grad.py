"""GPU: the gradient of the weighted bound in the weights (asvgp_weight_grad_1d; weight_gradient_device, noise_group_gradient and
fit_noise_groups of GPR_1d and of GPR_kron with d = 2).

Yardstick, written here: a dense numpy posterior - Phi from oracle.Basis.evaluate_basis, Kuu from O.make_Kuu, P = Kuu + Phi W Phi^T / s,
alpha, g_i = phi_i^T P^-1 phi_i, q_i = phi_i^T Kuu^-1 phi_i - and the closed form of include/asvgp_hip.h on it,
  d ELBO_w / d w_i = 1/2 [ D / w_i - D g_i / s - sum_d r_id^2 / s - (var_i - g_i) / s ],  var_i = v - q_i + g_i,  0 for w_i = 0.
From M = 1000 on the same formula takes mu, g and q from the oracle's band routines (two dense M x M inverses take seconds there, and
lose digits of Kuu^-1), as tests/test_loo.py does.  Two identities check the result against the project's own code: sum_i w_i grad_i =
-s d ELBO_w / d s (elbo_and_grad) and central differences of elbo() under set_weights.

Tolerances.  Per row: the first-order image of the project's 1e-8 gate on predicted means and variances,
|error| <= 1e-8 (D + 1 + 2 sum_d |r_id|) / s: the formula moves by (D + 1) / (2 s) per unit of g and var and by sum |r| / s per unit of mu,
doubled.  Group sums against float sums of the per-row output: 1e-12 of sum |terms|.  The analytic identity: 1e-7 sum |w_i grad_i| (the
project states 2e-8 for its gradient at the headline size; the sum adds the rounding of N terms).  Finite differences: elbo_tol / h_i
for the two bounds + 1e-5 of the terms of the formula for the truncation at h_i = 1e-3 w_i (the third derivative in log w is of the
order of the first's terms; (1e-3)^2 / 6 of it is far inside 1e-5).
Every comparison prints one "GERR" line (error over its gate or scale) for the record."""
import numpy as np
import pytest
import torch

from oracle import asvgp_oracle as O

pytestmark = pytest.mark.gpu

KNAMES = {0: "Matern12", 1: "Matern32", 2: "Matern52"}
UNSUPPORTED = -2                              # ASVGP_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def A():
    import asvgp_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from asvgp_amd import _lib
    _lib.get_lib()
    return asvgp_amd


def report(what, err, scale):
    r = float(err) / float(scale) if scale else float(err)
    print("GERR %-84s %.3e" % (what, r))
    return r


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def make_weights(rng, n, kind):
    """the weight kinds of tests/test_weighted_obs.py"""
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


def elbo_tol(e, N, v, s, yy, bcr=False):
    """tests/test_weighted_obs.py elbo_tol"""
    return 1e-9 * abs(e) + (5e-10 if bcr else 2e-11) * (0.5 * N * v / s + 0.5 * yy / s)


# ------------------------------------------------------------------------------------------------ yardsticks written here
def formula(mu, g, q, prior, y, w, s):
    """(grad (N,), r (N, D), var (N,)) from the posterior's mu, g = phi^T P^-1 phi and q = phi^T Kuu^-1 phi"""
    D = y.shape[1]
    r = y - mu
    var = prior - q + g
    pos = w > 0
    grad = np.where(pos, 0.5 * (D / np.where(pos, w, 1.0) - D * g / s - np.sum(r * r, axis=1) / s - (var - g) / s), 0.0)
    return grad, r, var


def dense_moments(PhiT, Kd, s, y, w):
    """(mu, g, q) of the dense posterior of a Gaussian linear model in the features; PhiT: scipy sparse (N, M), Kd: dense Kuu"""
    PhiW = PhiT.T.multiply(w[None, :]).tocsr()
    Pinv = np.linalg.inv(Kd + (PhiW @ PhiT).toarray() / s)
    Kinv = np.linalg.inv(Kd)
    alpha = Pinv @ (PhiW @ y) / s
    quad = lambda S: np.asarray(PhiT.multiply(PhiT @ S).sum(axis=1)).reshape(-1)
    return PhiT @ alpha, quad(Pinv), quad(Kinv)


def banded_moments(ob, kind, v, l, s, x, y, w):
    """(mu, g, q) through band quantities only (tests/test_loo.py banded_yardstick): band(P^-1), band(Kuu^-1) and alpha from the oracle's
    band Cholesky / selected inverse / triangular solves on the directly accumulated weighted statistics."""
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
    q = np.zeros(x.shape[0])
    for i in range(k + 1):
        ri = idx + k - i
        mu += vals[i][:, None] * alpha[ri]
        for j in range(k + 1):
            rj = idx + k - j
            hi, lo = np.maximum(ri, rj), np.minimum(ri, rj)
            g += vals[i] * vals[j] * SP[hi - lo, lo]
            q += vals[i] * vals[j] * SK[hi - lo, lo]
    return mu, g, q


def problem_1d(seed, order, kind, M, N, D, s=0.05, wkind="lognormal", l=None, v=1.2):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.02, 0.98, N)            # unsorted; inside the boundary layer of the spline features
    y = np.stack([np.sin(9 * (d + 1) * x) for d in range(D)], 1) + 0.3 * rng.normal(size=(N, D))
    w = None if wkind is None else make_weights(rng, N, wkind)
    return dict(order=order, kind=kind, M=M, N=N, D=D, s=s, l=(0.2 if M < 1000 else 20.0 / M) if l is None else l, v=v, x=x, y=y, w=w)


def build_1d(A, p):
    m = A.GPR_1d((p["x"].reshape(-1, 1), p["y"]), getattr(A, KNAMES[p["kind"]])(variance=p["v"], lengthscales=p["l"]),
                 getattr(A, "B%dSpline" % p["order"])(0, 1, p["M"]), weights=p["w"])
    m.likelihood.variance.assign(p["s"])
    return m


def yardstick_1d(p):
    """(grad, r, var, w) of the problem; w = 1 for a model without weights"""
    ob = O.Basis(p["order"], 0, 1, p["M"])
    w = np.ones(p["N"]) if p["w"] is None else p["w"]
    if p["M"] >= 1000:
        mu, g, q = banded_moments(ob, p["kind"], p["v"], p["l"], p["s"], p["x"], p["y"], w)
    else:
        PhiT = ob.evaluate_basis(p["x"].reshape(-1, 1), sparse=True).T.tocsr()
        mu, g, q = dense_moments(PhiT, O.band_to_dense_sym(O.make_Kuu(ob, p["kind"], p["v"], p["l"])), p["s"], p["y"], w)
    p["g"] = g                                # (kept for the leverages w g / s)
    return formula(mu, g, q, p["v"], p["y"], w, p["s"]) + (w,)


def row_gate(r, D, s):
    return 1e-8 * (D + 1 + 2 * np.sum(np.abs(r), axis=1)) / s


def check_rows(tag, got, p, ref=None):
    grad, r, _, w = yardstick_1d(p) if ref is None else ref
    assert got.shape == grad.shape
    assert report(tag + " per row (over its gate)", np.max(np.abs(got - grad) / row_gate(r, p["D"], p["s"])), 1.0) <= 1.0
    assert np.all(got[w == 0] == 0.0)         # a row with weight 0 is absent from the model: exactly 0
    return grad, w


def wgrad_call(model, N=None, groups=None, G=1, want="gs", x=None, expect=0):
    """asvgp_weight_grad_1d through the C-ABI with the model's rows and tables -> (grad (N,) or None, gsum (G, 2) or None), numpy"""
    from asvgp_amd import _lib
    lib = _lib.get_lib()
    alpha, W, Pinv = model._posterior_loo()
    b, D = model.basis, model.D
    N = model.X.shape[0] if N is None else N
    ws = torch.empty(max(lib.asvgp_weight_grad_workspace_bytes(b.m, b.order, D, min(G, 1024)), 8) // 8, dtype=torch.float64, device="cuda")
    grad = torch.full((N,), 7.0, dtype=torch.float64, device="cuda") if "g" in want else None
    gsum = torch.full((G, 2), 7.0, dtype=torch.float64, device="cuda") if "s" in want else None
    gt = None if groups is None else torch.as_tensor(groups, dtype=torch.int32).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.asvgp_weight_grad_1d(model._h.ptr, model.X.data_ptr(), model.y.data_ptr(), ptr(model.weights), N, D, b.mesh.data_ptr(),
                                  b.mesh.shape[0], b.delta_np, b.order, b.m, alpha.data_ptr(), W.data_ptr(), Pinv.data_ptr(),
                                  float(model.kernel.variance), float(model.likelihood.variance), ptr(gt), G, ptr(grad), ptr(gsum),
                                  ws.data_ptr(), ws.numel() * 8, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, lib.asvgp_last_error_string().decode()
    return (None if grad is None else grad.cpu().numpy()), (None if gsum is None else gsum.cpu().numpy())


def check_group_sums(tag, gsum, groups, G, grad, w):
    """n_g exact; T_g against the float sum of w_i grad_i over the group, 1e-12 of sum |terms|"""
    pos = w > 0
    assert np.array_equal(gsum[:, 0], np.bincount(groups[pos], minlength=G).astype(np.float64))
    t = w * grad
    ref = np.bincount(groups, weights=t, minlength=G)
    scale = np.bincount(groups, weights=np.abs(t), minlength=G)
    ok = scale > 0
    assert np.all(gsum[~ok, 1] == 0.0)
    assert report(tag + " T_g vs the float sum of the rows", np.max(np.abs(gsum[ok, 1] - ref[ok]) / scale[ok]), 1.0) <= 1e-12


# ------------------------------------------------------------------------------------------------ 1. per row, against the yardstick
# (order, kind, M, D, weights): order 1 carries the static bands of Matern-1/2 only, order 6 those of Matern-1/2 and 3/2
ROWS = [(1, 0, 20, 1, "decades"), (1, 0, 40, 3, "lognormal"), (3, 1, 30, 3, "integer"), (3, 2, 37, 1, None), (4, 2, 40, 1, "lognormal"),
        (4, 0, 25, 3, "decades"), (6, 1, 33, 3, None), (6, 0, 28, 1, "integer")]


@pytest.mark.parametrize("order,kind,M,D,wkind", ROWS)
def test_rows_against_dense_yardstick(A, order, kind, M, D, wkind):
    p = problem_1d(10 * order + kind + M, order, kind, M, 3000, D, wkind=wkind)
    model = build_1d(A, p)
    tag = "rows k=%d %s M=%d D=%d %s" % (order, KNAMES[kind], M, D, wkind)
    got = model.weight_gradient_device()
    assert got.is_cuda and got.dtype == torch.float64
    grad, w = check_rows(tag, got.cpu().numpy(), p)
    if wkind in ("decades", "integer"):
        assert np.any(w == 0)
    direct, _ = wgrad_call(model, want="g")                      # per-row output alone, no sums
    assert np.array_equal(direct, got.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 2. every branch of the launch plan
# (order, kind, M, N, D): unsorted x, lognormal weights with exact zeros added
PLAN = [
    (4, 1, 40, 2000, 1),                      # below 65 536 rows: tables through the caches
    (4, 1, 40, 70_000, 3),                    # staged whole, 1024 threads
    (4, 1, 3000, 70_000, 1),                  # k = 4, M = 3000: split into two ranges of mesh cells
    (6, 1, 1500, 70_000, 1),                  # order 6, 512 threads: two ranges
    (6, 1, 3000, 70_000, 1),                  # order 6, M = 3000: the tables fit no two ranges - through the caches at a staged N
    (3, 1, 40, 300_000, 1),                   # more rows than the grid has threads: the grid-stride loop wraps
]


@pytest.mark.parametrize("order,kind,M,N,D", PLAN)
def test_launch_plan_branches(A, order, kind, M, N, D):
    p = problem_1d(order + M + N, order, kind, M, N, D)
    p["w"][::7] = 0.0
    model = build_1d(A, p)
    tag = "plan k=%d M=%d N=%d D=%d" % (order, M, N, D)
    ref = yardstick_1d(p)
    grad, w = check_rows(tag, model.weight_gradient_device().cpu().numpy(), p, ref)
    # the sums by the same plan: one group in a fixed order, and 3 and 1000 groups in the bins (which shrink the staged tables' budget)
    rng = np.random.default_rng(N)
    both, one = wgrad_call(model, want="gs")
    assert np.array_equal(both, model.weight_gradient_device().cpu().numpy())
    check_group_sums(tag + " G=1", one, np.zeros(N, dtype=np.int64), 1, both, w)
    for G in (3, 1000):
        groups = rng.integers(0, G, N)
        _, gs = wgrad_call(model, groups=groups, G=G, want="s")
        check_group_sums(tag + " G=%d" % G, gs, groups, G, both, w)


# ------------------------------------------------------------------------------------------------ 3. group sums
@pytest.fixture(scope="module")
def grouped(A):
    p = problem_1d(77, 4, 1, 40, 3000, 3)
    p["w"][::5] = 0.0
    model = build_1d(A, p)
    grad = model.weight_gradient_device().cpu().numpy()
    return p, model, grad


@pytest.mark.parametrize("G", [1, 3, 1000])
def test_group_sums(A, grouped, G):
    p, model, grad = grouped
    N, w = p["N"], p["w"]
    rng = np.random.default_rng(G)
    if G == 1000:                             # most groups empty: 40 labels in use, shuffled over the rows
        groups = rng.choice(rng.choice(G, 40, replace=False), N)
        groups[0] = G - 1
    else:
        groups = rng.permutation(np.arange(N) % G)
    _, gs = wgrad_call(model, groups=None if G == 1 else groups, G=G, want="s")
    check_group_sums("group sums C-ABI G=%d" % G, gs, groups, G, grad, w)
    out = model.noise_group_gradient(groups)                     # G = max + 1
    assert out["n"].shape == out["grad_log_weight"].shape == (G,)
    assert np.issubdtype(out["n"].dtype, np.integer)
    check_group_sums("noise_group_gradient G=%d" % G, np.stack([out["n"].astype(np.float64), out["grad_log_weight"]], 1), groups, G, grad, w)
    if G == 3:                                # labels given as a device tensor of another integer type
        again = model.noise_group_gradient(torch.as_tensor(groups, dtype=torch.int16).cuda())
        assert np.array_equal(again["n"], out["n"])


def test_no_groups_twice_same_bits(A, grouped):
    _, model, _ = grouped
    a = wgrad_call(model, want="s")[1]
    b = wgrad_call(model, want="s")[1]
    c = wgrad_call(model, want="gs")[1]
    assert a.tobytes() == b.tobytes() == c.tobytes()


def test_more_groups_than_the_bins_hold(A, grouped):
    p, model, grad = grouped
    wgrad_call(model, groups=np.zeros(p["N"], dtype=np.int64), G=1025, want="s", expect=UNSUPPORTED)
    groups = np.random.default_rng(3).integers(0, 1500, p["N"])     # the Python surface sums the per-row output instead
    groups[0] = 1499
    out = model.noise_group_gradient(groups)
    check_group_sums("noise_group_gradient G=1500 (index_add_)", np.stack([out["n"].astype(np.float64), out["grad_log_weight"]], 1),
                     groups, 1500, grad, p["w"])


def test_label_out_of_range(A, grouped):
    p, model, grad = grouped
    groups = np.arange(p["N"]) % 3
    bad = groups.copy()
    bad[5] = -1
    with pytest.raises(ValueError):
        model.noise_group_gradient(bad)
    # the kernel itself leaves such a row out and never indexes with its label
    bad[6], bad[7] = 3, 2 ** 31 - 1
    _, gs = wgrad_call(model, groups=bad, G=3, want="s")
    keep = np.ones(p["N"], dtype=bool)
    keep[5:8] = False
    check_group_sums("labels outside [0, G) are left out", gs, groups[keep], 3, grad[keep], p["w"][keep])


def test_empty_batch_zeroes_gsum(A, grouped):
    _, model, _ = grouped
    _, gs = wgrad_call(model, N=0, groups=None, G=1, want="s")
    assert np.array_equal(gs, np.zeros((1, 2)))


# ------------------------------------------------------------------------------------------------ 4. the existing analytic gradient
@pytest.mark.parametrize("D", [1, 3])
def test_scaling_identity_1d(A, D):
    """sum_g T_g = sum_i w_i grad_i = -s d ELBO_w / d s"""
    p = problem_1d(200 + D, 4, 1, 40, 3000, D)
    model = build_1d(A, p)
    groups = np.arange(p["N"]) % 3
    T = model.noise_group_gradient(groups)["grad_log_weight"]
    ds = float(model.elbo_and_grad()[3])
    scale = float(np.sum(np.abs(p["w"] * model.weight_gradient_device().cpu().numpy())))
    assert report("identity GPR_1d D=%d: sum T_g + s dELBO/ds" % D, abs(np.sum(T) + p["s"] * ds), scale) <= 1e-7


def kron_problem(N=3000, seed=5):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(0.03, 0.97, N), rng.uniform(-0.91, 1.91, N)], axis=1)
    y = np.sin(12 * X[:, :1]) * np.cos(3 * X[:, 1:]) + 0.1 * rng.normal(size=(N, 1))
    return X, y, np.exp(rng.normal(size=N))


def build_kron(A, X, y, w, m1=12, m2=14, order=3, s=0.05):
    Bs = getattr(A, "B%dSpline" % order)
    m = A.GPR_kron((X, y), [A.Matern32(variance=1.1, lengthscales=0.3), A.Matern32(variance=0.9, lengthscales=0.8)],
                   [Bs(0, 1, m1), Bs(-1, 2, m2)], weights=w)
    m.likelihood.variance.assign(s)
    return m


def test_scaling_identity_kron(A):
    X, y, w = kron_problem()
    model = build_kron(A, X, y, w)
    groups = np.arange(X.shape[0]) % 3
    out = model.noise_group_gradient(groups)
    assert np.array_equal(out["n"], np.bincount(groups))
    grad = model.weight_gradient_device().cpu().numpy()
    check_group_sums("kron group sums", np.stack([out["n"].astype(np.float64), out["grad_log_weight"]], 1), groups, 3, grad, w)
    _, g = model.elbo_and_grad()
    scale = float(np.sum(np.abs(w * grad)))
    assert report("identity GPR_kron 12x14: sum T_g + s dELBO/ds", abs(np.sum(out["grad_log_weight"]) + 0.05 * g[-1]), scale) <= 1e-7


# ------------------------------------------------------------------------------------------------ 5. finite differences of elbo()
def check_finite_differences(tag, model, w, rows, grad, D, terms, tol):
    w0 = model.weights.clone()
    try:
        for i in rows:
            h = 1e-3 * w[i]
            e = []
            for sign in (1.0, -1.0):
                wi = w.copy()
                wi[i] += sign * h
                model.set_weights(wi)
                e.append(float(model.elbo()))
            fd = (e[0] - e[1]) / (2 * h)
            allowed = tol / h + 1e-5 * terms[i]
            assert report("%s row %d (w = %.3g): central difference vs the gradient (over its allowance)" % (tag, i, w[i]),
                          abs(fd - grad[i]), allowed) <= 1.0
    finally:
        model.set_weights(w0)                                    # the weights are restored
    assert torch.equal(model.weights, w0)


@pytest.mark.parametrize("D", [1, 3])
def test_finite_differences_1d(A, D):
    p = problem_1d(300 + D, 4, 1, 40, 400, D)
    model = build_1d(A, p)
    ref, r, var, w = yardstick_1d(p)
    s, v = p["s"], p["v"]
    grad = model.weight_gradient_device().cpu().numpy()
    lev = w * p["g"] / s                                         # leverage h_i = w_i g_i / s
    top = int(np.argmax(lev))
    rows = [top] + [int(i) for i in np.random.default_rng(D).choice(np.delete(np.arange(p["N"]), top), 7, replace=False)]
    report("finite differences GPR_1d D=%d: largest leverage" % D, lev[top], 1.0)
    terms = D / w + (np.sum(r * r, axis=1) + D * var) / s
    yy = float(np.sum(w[:, None] * p["y"] ** 2))
    tol = elbo_tol(float(model.elbo()), max(w.sum(), p["N"]), v, s, yy, bcr=True)
    check_finite_differences("finite differences GPR_1d D=%d" % D, model, w, rows, grad, D, terms, tol)


def test_finite_differences_kron(A):
    X, y, w = kron_problem(N=400, seed=6)
    model = build_kron(A, X, y, w, m1=8, m2=9)
    grad = model.weight_gradient_device().cpu().numpy()
    mean, var = (t.cpu().numpy() for t in model.predict_f_device(X))
    r2 = ((y - mean) ** 2).reshape(-1)
    terms = 1 / w + (r2 + var.reshape(-1)) / 0.05
    tol = elbo_tol(float(model.elbo()), max(w.sum(), 400), 1.1 * 0.9, 0.05, float(np.sum(w[:, None] * y * y)), bcr=True)
    rows = list(np.random.default_rng(8).choice(400, 4, replace=False))
    check_finite_differences("finite differences GPR_kron 8x9", model, w, rows, grad, 1, terms, tol)


# ------------------------------------------------------------------------------------------------ 6. fit_noise_groups
@pytest.fixture(scope="module")
def instruments():
    rng = np.random.default_rng(11)
    N = 6000
    x = rng.uniform(0.0, 1.0, N)
    x = np.clip(x, 1e-9, 1 - 1e-9)
    groups = rng.permutation(np.arange(N) % 3)
    sd = np.array([0.1, 0.3, 0.05])[groups]
    y = (np.sin(12 * x) + sd * rng.normal(size=N)).reshape(-1, 1)
    return x, y, groups


def instrument_model(A, x, y):
    m = A.GPR_1d((x.reshape(-1, 1), y), A.Matern32(variance=1.0, lengthscales=0.2), A.B3Spline(0, 1, 40), weights=np.ones(x.shape[0]))
    return m


def test_fit_noise_groups(A, instruments):
    x, y, groups = instruments
    model = instrument_model(A, x, y)
    w0 = model.weights.cpu().numpy().copy()
    before = float(model.elbo())
    res = model.fit_noise_groups(groups, maxiter=200, pinned=0)
    after = float(model.elbo())
    rho = model.noise_scales
    print("fit_noise_groups: bound %.6f -> %.6f, rho = %s, theta = %s, %d evaluations" % (before, after, rho, model.theta(), res.nfev))
    assert after >= before
    assert rho.shape == (3,) and rho[0] == 1.0
    assert abs(rho[1] / 9.0 - 1.0) <= 0.25 and abs(rho[2] / 0.25 - 1.0) <= 0.25
    assert np.array_equal(model.weights.cpu().numpy(), w0 / rho[groups])
    assert abs(after + res.fun) <= 1e-6 * abs(after)             # the model is left at the returned point


def test_fit_noise_groups_restores_on_exception(A, instruments, monkeypatch):
    x, y, groups = instruments
    model = instrument_model(A, x, y)
    w0, stats0 = model.weights.clone(), model._stats.clone()
    theta0 = [(p._u, p._value) for p in model.trainable_parameters]
    sums0 = (model.num_data, model.weight_sum, model.log_weight_sum)
    calls = []
    inner = model._group_sums

    def failing(labels, G):
        calls.append(1)
        if len(calls) == 3:
            raise RuntimeError("forced")
        return inner(labels, G)

    monkeypatch.setattr(model, "_group_sums", failing)
    with pytest.raises(RuntimeError, match="forced"):
        model.fit_noise_groups(groups, maxiter=50)
    assert len(calls) == 3
    assert torch.equal(model.weights, w0) and torch.equal(model._stats, stats0)
    assert [(p._u, p._value) for p in model.trainable_parameters] == theta0
    assert (model.num_data, model.weight_sum, model.log_weight_sum) == sums0


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(A):
    rng = np.random.default_rng(0)
    N = 200
    X = rng.uniform(0.05, 0.95, (N, 3))
    y = rng.normal(size=(N, 1))
    groups = np.arange(N) % 2
    kerns = lambda d: [A.Matern32(variance=1.0, lengthscales=0.3) for _ in range(d)]
    additive = A.GPR_additive((X[:, :2], y), kerns(2), [A.B3Spline(0, 1, 8) for _ in range(2)])
    kron3 = A.GPR_kron((X, y), kerns(3), [A.B3Spline(0, 1, 8) for _ in range(3)])
    for model in (additive, kron3):
        for name, args in (("weight_gradient_device", ()), ("noise_group_gradient", (groups,)), ("fit_noise_groups", (groups,))):
            with pytest.raises(NotImplementedError, match=name):
                getattr(model, name)(*args)
    p = problem_1d(1, 3, 1, 20, 300, 1, wkind=None)
    unweighted = build_1d(A, p)
    with pytest.raises(ValueError, match="built without weights"):
        unweighted.fit_noise_groups(np.arange(300) % 2)
    assert unweighted.noise_group_gradient(np.arange(300) % 2)["n"].tolist() == [150, 150]    # (the gradient itself takes w = 1)
