"""Full posterior covariance of GPR_additive: d = 8, m_i = 256 (M_tot = 2048, GPR_1d's headline M), order 3, Matern-3/2, N = 1M.
Times the once-per-theta prepare's parts (the dense factorisation _factor, cholesky_inverse of its factor, the K_i^-1 subtraction) and
the whole prepare; predict_f_cov_device at n = 1k / 10k with W cached; and the same covariance through dense torch on the same GPU
(dense Kus, triangular solves, GEMMs).  Times are medians of device-event timings (warm-up first).  The kernel alone: run this under
rocprofv3 --kernel-trace --stats."""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import asvgp_amd as A  # noqa: E402
from asvgp_amd import utils  # noqa: E402

N, d, m, k = 1_000_000, 8, 256, 3
th, s = [(1.0 - 0.05 * i, 0.1 + 0.02 * i) for i in range(d)], 0.01
rng = np.random.default_rng(0)
X = rng.uniform(1e-6, 1 - 1e-6, (N, d))
y = np.sin(6 * X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N, 1))
model = A.GPR_additive((torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()),
                       [A.Matern32(variance=v, lengthscales=l) for v, l in th], [A.B3Spline(0, 1, m) for _ in range(d)])
model.likelihood.variance.assign(s)
M = model.Mtot
vs = sum(v for v, _ in th)


def timed(fn, reps=5, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


f = model._factor()
t_fac = timed(lambda: model._factor())
t_inv = timed(lambda: torch.cholesky_inverse(f["L"]))
W = torch.cholesky_inverse(f["L"])


def subtract():                                  # the d dense K_i^-1 (batched over equal m_i) subtracted, W symmetrised
    return model._minus_kuu_inverse(W.clone(), f["Ks"])


t_sub = timed(subtract)


def prepare():                                   # what the first predict_f_cov_device of a theta pays
    model._post_cov = None
    return model._posterior_cov()


t_prep = timed(prepare, reps=3)
print("d=%d m_i=%d M_tot=%d k=%d N=%d | factor %.0f us | cholesky_inverse %.0f us | K_i^-1 subtraction %.0f us | whole prepare %.0f us"
      % (d, m, M, k, N, t_fac, t_inv, t_sub, t_prep), flush=True)
del W

sq3 = 3.0 ** 0.5
for n in (1_000, 10_000):
    xs = torch.from_numpy(rng.uniform(0.001, 0.999, (n, d))).cuda()
    model.predict_f_cov_device(xs)
    t_cov = timed(lambda: model.predict_f_cov_device(xs), reps=7, warm=2)

    def torch_route():
        f = model._factor()
        Kus = torch.cat([b.evaluate_basis(xs[:, i:i + 1].contiguous(), sparse=False) for i, b in enumerate(model.bases)], 0)
        TP = torch.linalg.solve_triangular(f["L"], Kus, upper=False)
        out = TP.T @ TP
        for i, (kern, K) in enumerate(zip(model.kernels, f["Ks"])):
            LK = torch.linalg.cholesky(utils.band_to_dense_sym(K))
            TK = torch.linalg.solve_triangular(LK, Kus[model.offsets[i]:model.offsets[i + 1]], upper=False)
            out -= TK.T @ TK
            r = (xs[:, i:i + 1] - xs[:, i].reshape(1, -1)).abs() * (sq3 / float(kern.lengthscales))
            out += float(kern.variance) * (1 + r) * torch.exp(-r)
        return out
    ref = torch_route()
    t_torch = timed(torch_route, reps=3, warm=1)
    got = model.predict_f_cov_device(xs)
    diff = (got - ref).abs().max().item()
    _, var = model.predict_f_device(xs)
    ddiag = (torch.diagonal(got) - var[:, 0]).abs().max().item()
    print("n=%6d: predict_f_cov_device %9.1f us (%.0f MB out, store floor %.1f us at 8 TB/s; %.2e Matern evaluations) | dense torch "
          "%10.1f us | ratio %.1fx | prepare + call %.1fx | max |diff| %.2e (%.1e sum v) | diag vs predict_f %.2e"
          % (n, t_cov, n * n * 8 / 1e6, n * n * 8 / 8e6, float(n) * n * d, t_torch, t_torch / t_cov, t_torch / (t_prep + t_cov), diff,
             diff / vs, ddiag), flush=True)
    del ref, got
    torch.cuda.empty_cache()
model.close()
