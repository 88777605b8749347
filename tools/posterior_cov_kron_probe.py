"""Full posterior covariance of GPR_kron at BASELINE config 4's size (128 x 128 basis, k = 4, Matern-3/2, N = 1M; twisted layout).
Times the prepare's parts (band factorisation of P, selected inverse on the band, the dense Sigma kernel asvgp_kron_dense_inverse alone)
and the whole prepare; predict_f_cov_device at n = 1k / 10k, with the test rows in random and in cell order; and the same covariance
through dense torch on the same GPU (P densified from the block band, dense Cholesky, triangular solves, GEMMs).  Times are medians of
device-event timings (warm-up first)."""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import asvgp_amd as A  # noqa: E402
from asvgp_amd import _lib, utils  # noqa: E402

N, m, k = 1_000_000, 128, 4
th, s = [(1.0, 0.1), (1.0, 0.1)], 0.01
rng = np.random.default_rng(0)
X = rng.uniform(1e-6, 1 - 1e-6, (N, 2))
y = np.sin(8 * X[:, :1]) * np.cos(5 * X[:, 1:]) + 0.1 * rng.standard_normal((N, 1))
model = A.GPR_kron((torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()),
                   [A.Matern32(variance=v, lengthscales=l) for v, l in th], [A.B4Spline(0, 1, m), A.B4Spline(0, 1, m)])
model.likelihood.variance.assign(s)
M = model.Mtot
lay = model._twist_layout()


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


f = model._factor(want_alpha=False)
t_fac = timed(lambda: model._factor(want_alpha=False))
f["keep_G"] = True
t_sel = timed(lambda: model._selinv(f))
SigD, SigS, Bb = model._selinv(f)
nb = lay["nb"]
G = f.pop("G").transpose(0, 1).contiguous()
Sig = torch.empty((M, M), dtype=torch.float64, device="cuda")
lib = _lib.get_lib()


def sweep():                                     # asvgp_kron_dense_inverse alone: seeds + 29 step launches
    _lib.check(lib.asvgp_kron_dense_inverse(G.data_ptr(), SigD.data_ptr(), SigS.data_ptr(), M, Bb, 1, nb, lay["top_end"], lay["padt"],
                                              lay["padb"], Sig.data_ptr(), _lib.stream_ptr()), "kron_dense_inverse")


t_sweep = timed(sweep)
del G, Sig
torch.cuda.empty_cache()


def prepare():                                   # what the first predict_f_cov_device of a theta pays: factor, selected inverse, dense Sigma, K_d^-1
    model._post, model._post_cov = None, None
    return model._posterior_cov()


t_prep = timed(prepare, reps=3)
# block products of the sweep: (1) + (2), 2 Bb^3 flops each
prods = sum(nb - j - 2 for j in range(nb - 2)) + sum((nb - j - 2) + (nb - 1) for j in range(nb - 1))
flops = prods * 2.0 * Bb ** 3
print("M_tot=%d k=%d twisted Bb=%d nb=%d | factor %.0f us | selected inverse %.0f us | dense Sigma kernel alone %.0f us (%.2e flops, "
      "%.1f TFLOP/s; Sigma %.2f GB) | whole prepare %.0f us" % (M, k, Bb, nb, t_fac, t_sel, t_sweep, flops, flops / t_sweep / 1e6,
                                                              M * M * 8 / 1e9, t_prep), flush=True)

Sig, _ = model._posterior_cov()
K1, K2 = model.kernels
Ks = []
for feat, kern in zip(model.inducing_features, model.kernels):
    Ks.append(utils.band_to_dense_sym(feat.inverse_band(kern)[0]))
Pd = model.KufKfu_dense / s + torch.kron(Ks[0], Ks[1])
sq3 = 3.0 ** 0.5
for n in (1_000, 10_000):
    xs = torch.from_numpy(rng.uniform(0.001, 0.999, (n, 2))).cuda()
    model.predict_f_cov_device(xs)
    t_cov = timed(lambda: model.predict_f_cov_device(xs), reps=7, warm=2)
    # the rows x1 in cell order (neighbouring workgroups then read the same Sigma rows), the columns as they are
    b1, b2 = model.bases
    cell = torch.floor((xs[:, 0] - b1.a) / b1.delta_np) * (b2.m - k) + torch.floor((xs[:, 1] - b2.a) / b2.delta_np)
    xs_c = xs[torch.argsort(cell)].contiguous()
    t_cov_rand = timed(lambda: model.predict_f_cov_device(xs, xs), reps=7, warm=2)
    t_cov_cell = timed(lambda: model.predict_f_cov_device(xs_c, xs), reps=7, warm=2)
    print("n=%6d: rows in random order %.1f us, rows in cell order %.1f us" % (n, t_cov_rand, t_cov_cell), flush=True)
    Phi = model._dense_rows(xs)
    Phid = [b.evaluate_basis(xs[:, d:d + 1].contiguous(), sparse=False) for d, b in enumerate(model.bases)]

    def torch_route():
        LP = torch.linalg.cholesky(Pd)
        TP = torch.linalg.solve_triangular(LP, Phi, upper=False)
        out = TP.T @ TP
        for d, (kern, Kd) in enumerate(zip(model.kernels, Ks)):
            LK = torch.linalg.cholesky(Kd)
            TK = torch.linalg.solve_triangular(LK, Phid[d], upper=False)
            r = (xs[:, d:d + 1] - xs[:, d].reshape(1, -1)).abs() * (sq3 / float(kern.lengthscales))
            if d == 0:
                kk = float(kern.variance) * (1 + r) * torch.exp(-r)
                qk = TK.T @ TK
            else:
                kk = kk * (float(kern.variance) * (1 + r) * torch.exp(-r))
                qk = qk * (TK.T @ TK)
        return kk + out - qk
    ref = torch_route()
    t_torch = timed(torch_route, reps=3, warm=1)
    got = model.predict_f_cov_device(xs)
    diff = (got - ref).abs().max().item()
    print("n=%6d: predict_f_cov_device %9.1f us (%.0f MB out; Sigma rows read %.1f GB) | dense torch %10.1f us | ratio %.1fx | "
          "max |diff| %.2e" % (n, t_cov, n * n * 8 / 1e6, n * (k + 1) ** 2 * M * 8 / 1e9, t_torch, t_torch / t_cov, diff), flush=True)
    del Phi, Phid, ref, got
    torch.cuda.empty_cache()
print("dense torch: the cholesky of the dense P alone %.0f us" % timed(lambda: torch.linalg.cholesky(Pd), reps=3), flush=True)
model.close()
