"""Posterior gradient predictions against the posterior of f itself, on the same points.
1-D: M = 2048, k = 4, Matern-3/2, 10M unsorted points: predict_f_gradient_device (asvgp_predict_deriv_1d) beside the table kernel
(asvgp_predict_1d, the plan it shares) and predict_f_device (which takes the cell-polynomial kernel at this size).
2-D: 100 x 100 B4 (the eNATL60 shape, twisted layout) and 128 x 128 with k = 3, n = 100k and 1M with the factor cached:
predict_f_gradient_device (asvgp_predict_grad_kron2d) beside predict_f_device.  Times are medians of device-event timings (warm-up
first)."""
import sys
import numpy as np
import torch
sys.path.insert(0, ".")
import asvgp_amd as A
from asvgp_amd._lib import check, get_lib, stream_ptr


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


rng = np.random.default_rng(0)
# ---------------------------------------------------------------------------------------------------------------- 1-D
N, M, k = 1_000_000, 2048, 4
x = rng.uniform(1e-9, 1 - 1e-9, N); y = np.sin(20 * x) + 0.1 * rng.standard_normal(N)
model = A.GPR_1d((torch.from_numpy(x).cuda().reshape(-1, 1), torch.from_numpy(y).cuda().reshape(-1, 1)),
                 A.Matern32(variance=1.0, lengthscales=0.05), A.B4Spline(0, 1, M))
model.likelihood.variance.assign(0.01)
ns = 10_000_000
xs = (torch.rand(ns, dtype=torch.float64, device="cuda") * 0.998 + 0.001).reshape(-1, 1)
alpha, W = model._posterior()
b = model.basis
mean_t = torch.empty(ns, dtype=torch.float64, device="cuda")
var_t = torch.empty(ns, dtype=torch.float64, device="cuda")


def table():
    check(get_lib().asvgp_predict_1d(xs.data_ptr(), ns, b.mesh.data_ptr(), b.mesh.shape[0], b.delta_np, b.order, b.m, alpha.data_ptr(),
                                     W.data_ptr(), 1.0, 1, mean_t.data_ptr(), var_t.data_ptr(), stream_ptr()), "predict_1d")


t_grad = timed(lambda: model.predict_f_gradient_device(xs))
t_table = timed(table)
t_f = timed(lambda: model.predict_f_device(xs))
print("1-D M=%d k=%d n=%d unsorted: predict_f_gradient_device %.1f us (%.2f TB/s at 24 B/point) | table kernel asvgp_predict_1d %.1f us | "
      "predict_f_device %.1f us | gradient / table %.2fx" % (M, k, ns, t_grad, 24 * ns / t_grad / 1e6, t_table, t_f, t_grad / t_table), flush=True)
del xs, mean_t, var_t
model.close()
torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------------------------------- 2-D
for order, m, Nk in ((4, 100, 200_000), (3, 128, 1_000_000)):
    X = rng.uniform(0.0005, 0.9995, (Nk, 2))
    yk = np.sin(8 * X[:, :1]) * np.cos(5 * X[:, 1:]) + 0.1 * rng.normal(size=(Nk, 1))
    B = getattr(A, "B%dSpline" % order)
    km = A.GPR_kron((X, yk), [A.Matern32(variance=1.1, lengthscales=0.1), A.Matern32(variance=0.9, lengthscales=0.15)],
                    [B(0, 1, m), B(0, 1, m)])
    km.likelihood.variance.assign(0.01)
    lay = km._twist_layout()
    km.predict_f_device(X[:10])                          # factor + selected inverse, cached
    for n in (100_000, 1_000_000):
        Xq = torch.from_numpy(rng.uniform(0.001, 0.999, (n, 2))).cuda()
        t_g = timed(lambda: km.predict_f_gradient_device(Xq))
        t_p = timed(lambda: km.predict_f_device(Xq))
        print("2-D %d x %d k=%d (%s layout) n=%7d, factor cached: predict_f_gradient_device %.1f us | predict_f_device %.1f us | ratio %.2fx"
              % (m, m, order, "twisted" if lay is not None else "one-sided", n, t_g, t_p, t_g / t_p), flush=True)
        del Xq
    km.close()
    torch.cuda.empty_cache()
