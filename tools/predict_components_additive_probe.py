"""Posterior of the additive components and of the gradient of GPR_additive: d = 8, m_i = 256 (M_tot = 2048), order 3, Matern-3/2,
N = 1M (the configuration of posterior_cov_additive_probe.py).  Times the first call of a theta (W and alpha from one dense factor);
predict_f_components_device (p = 0) and predict_f_gradient_device (p = 1) at n = 100k and 1M with W cached; predict_f_device at the same n
for context; and the same formulas through dense torch at n = 100k (per dimension j the GEMM W[:, block j] Phi_j, then the products with
Phi_i summed per pair): time and largest difference.  Times are medians of device-event timings (warm-up first).  The kernel alone: run
with --trace under rocprofv3 --kernel-trace --stats (only the kernel calls, three of each)."""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import asvgp_amd as A  # noqa: E402

TRACE = "--trace" in sys.argv
N, d, m, k = 1_000_000, 8, 256, 3
th, s = [(1.0 - 0.05 * i, 0.1 + 0.02 * i) for i in range(d)], 0.01
rng = np.random.default_rng(0)
X = rng.uniform(1e-6, 1 - 1e-6, (N, d))
y = np.sin(6 * X).sum(1, keepdims=True) + 0.1 * rng.standard_normal((N, 1))
model = A.GPR_additive((torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()),
                       [A.Matern32(variance=v, lengthscales=l) for v, l in th], [A.B3Spline(0, 1, m) for _ in range(d)])
model.likelihood.variance.assign(s)
M = model.Mtot
pairs = d * (d + 1) // 2
w_bytes = pairs * (k + 1) ** 2 * 8                 # W gathered per point: (k + 1) rows of k + 1 doubles per pair j <= i
a_bytes = d * (k + 1) * 8
st_bytes = (d + d * d) * 8
print("d=%d m_i=%d M_tot=%d k=%d N=%d | per point: W gathered %d B (%d pairs x %d x %d B), alpha %d B, stores %d B | W %.1f MB"
      % (d, m, M, k, N, w_bytes, pairs, k + 1, (k + 1) * 8, a_bytes, st_bytes, M * M * 8 / 1e6), flush=True)


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


xs = {n: torch.from_numpy(rng.uniform(0.001, 0.999, (n, d))).cuda() for n in (100_000, 1_000_000)}
if TRACE:
    for n, x in xs.items():
        for _ in range(3):
            model.predict_f_components_device(x)
            model.predict_f_gradient_device(x)
    torch.cuda.synchronize()
    model.close()
    sys.exit(0)


def prepare():                                   # what the first call of a theta pays: W and alpha from one factor
    model._post_cov = model._post_alpha = None
    return model._posterior_cov()


t_prep = timed(prepare, reps=3)
print("first call of a theta (W + alpha): %.0f us" % t_prep, flush=True)
for n, x in xs.items():
    t0 = timed(lambda: model.predict_f_components_device(x), reps=7, warm=2)
    t1 = timed(lambda: model.predict_f_gradient_device(x), reps=7, warm=2)
    tf = timed(lambda: model.predict_f_device(x), reps=3, warm=1)
    print("n=%8d: components %8.1f us (%.1f GB/s of W gathers) | gradient %8.1f us (%.1f GB/s) | predict_f_device %9.1f us"
          % (n, t0, n * w_bytes / t0 / 1e3, t1, n * w_bytes / t1 / 1e3, tf), flush=True)

n, x = 100_000, xs[100_000]
W, _ = model._posterior_cov()
alpha = model._post_alpha[1]


def torch_route(p):
    Ph = [b.evaluate_basis(x[:, i:i + 1].contiguous(), dx=p, sparse=False) for i, b in enumerate(model.bases)]
    mean = torch.stack([Ph[i].t() @ alpha[i * m:(i + 1) * m] for i in range(d)], 1)
    cov = torch.empty((n, d, d), dtype=torch.float64, device=x.device)
    for j in range(d):
        G = W[:, j * m:(j + 1) * m] @ Ph[j]                    # (M_tot, n)
        for i in range(d):
            cov[:, i, j] = (Ph[i] * G[i * m:(i + 1) * m]).sum(0)
        del G
    for i, kern in enumerate(model.kernels):
        v, l = float(kern.variance), float(kern.lengthscales)
        cov[:, i, i] += v if p == 0 else 3.0 * v / l ** 2
    return mean, cov


for p, fn in ((0, model.predict_f_components_device), (1, model.predict_f_gradient_device)):
    rm, rc = torch_route(p)
    t_torch = timed(lambda: torch_route(p), reps=3, warm=1)
    t_k = timed(lambda: fn(x), reps=7, warm=2)
    gm, gc = fn(x)
    pr = torch.tensor([float(kn.variance) if p == 0 else 3.0 * float(kn.variance) / float(kn.lengthscales) ** 2 for kn in model.kernels],
                      dtype=torch.float64, device=x.device)
    sc = torch.sqrt(torch.outer(pr, pr))
    print("n=%d p=%d: dense torch %10.1f us (%.2f TFLOP of GEMM) | kernel route %8.1f us | ratio %.1fx | max |diff| mean %.2e (%.1e of "
          "max), cov %.2e of sqrt(prior_i prior_j)"
          % (n, p, t_torch, 2.0 * M * m * d * n / 1e12, t_k, t_torch / t_k, (gm - rm).abs().max().item(),
             (gm - rm).abs().max().item() / rm.abs().max().item(), ((gc - rc).abs() / sc).max().item()), flush=True)
    del rm, rc
    torch.cuda.empty_cache()
model.close()
