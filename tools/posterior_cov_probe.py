"""Full posterior covariance of GPR_1d: asvgp_posterior_cov_prepare_1d (dense W = P^-1 - Kuu^-1, once per theta) at M = 2048 and
predict_f_cov_device at n = 1k / 10k (D = 1), against the same covariance through torch on the same GPU: dense Cholesky of Kuu and P,
triangular solves on Kus, GEMMs.  Times are medians of device-event timings (warm-up first)."""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
import asvgp_amd as A
from oracle import asvgp_oracle as O

N, M, k = 1_000_000, 2048, 4
v, l, s = 1.0, 0.05, 0.01
rng = np.random.default_rng(0)
x = rng.uniform(1e-9, 1 - 1e-9, N); y = np.sin(20 * x) + 0.1 * rng.standard_normal(N)
model = A.GPR_1d((torch.from_numpy(x).cuda().reshape(-1, 1), torch.from_numpy(y).cuda().reshape(-1, 1)),
                 A.Matern32(variance=v, lengthscales=l), A.B4Spline(0, 1, M))
model.likelihood.variance.assign(s)


def timed(fn, reps=7, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


def prepare():
    model._post_cov = None
    return model._posterior_cov()


t_prep = timed(prepare)
t_band = timed(lambda: (setattr(model, "_post", None), model._posterior()))
print("prepare M=%d k=%d: dense W %.1f us (band-only posterior_prepare %.1f us; W_dense %.1f MB)" % (M, k, t_prep, t_band, M * M * 8 / 1e6), flush=True)

# the torch route's inputs: dense Kuu and P from the same bands, dense Kus from the same basis
ob = O.Basis(k, 0, 1, M)
Kuu_b = O.make_Kuu(ob, 1, v, l)
Ab = model.KufKfu.cpu().numpy()
Kd = torch.from_numpy(O.unpack_banded_matrix_to_dense(O.symmetrise_band(Kuu_b, k), k, k)).cuda()
Pd = torch.from_numpy(O.unpack_banded_matrix_to_dense(O.symmetrise_band(Ab, k), k, k)).cuda() / s + Kd
sq3 = 3.0 ** 0.5
for n in (1_000, 10_000):
    xs = np.sort(rng.uniform(0.001, 0.999, n))
    xs_d = torch.from_numpy(xs).cuda()
    Kus = torch.from_numpy(ob.evaluate_basis(xs, sparse=False)).cuda()
    model.predict_f_cov_device(xs_d)
    t_cov = timed(lambda: model.predict_f_cov_device(xs_d))

    def torch_route():
        LK = torch.linalg.cholesky(Kd)
        LP = torch.linalg.cholesky(Pd)
        TK = torch.linalg.solve_triangular(LK, Kus, upper=False)
        TP = torch.linalg.solve_triangular(LP, Kus, upper=False)
        r = (xs_d[:, None] - xs_d[None, :]).abs() * (sq3 / l)
        return v * (1 + r) * torch.exp(-r) + TP.T @ TP - TK.T @ TK
    ref = torch_route()
    t_torch = timed(torch_route, reps=5, warm=1)
    got = model.predict_f_cov_device(xs_d)
    diff = (got - ref).abs().max().item()
    out_mb = n * n * 8 / 1e6
    floor_us = n * n * 8 / 8.0e12 * 1e6    # output write at 8 TB/s
    print("n=%6d: predict_f_cov_device %9.1f us (%.0f MB out, %.2f TB/s; write floor at 8 TB/s %.1f us) | torch route %10.1f us | "
          "ratio %.1fx | max |diff| %.2e" % (n, t_cov, out_mb, n * n * 8 / t_cov / 1e6, floor_us, t_torch, t_torch / t_cov, diff), flush=True)
    del Kus, ref, got
    torch.cuda.empty_cache()
model.close()
