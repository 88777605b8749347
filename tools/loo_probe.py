"""Leave-one-out predictions: the fused kernel against what a user could write without it, in ONE process, alternating, after warm-up,
timed with device events.

1-D: N = 10M, M = 2048, B4, Matern-3/2, unsorted x, weighted and unweighted:
  asvgp_loo_1d with the scores alone (nothing of size N written),
  asvgp_loo_1d with every per-row output and the scores,
  the composition: asvgp_predict_1d_h twice (with W, and with Pinv_band and variance 0 for g), then the formulas and the four
  reductions as torch elementwise operations and sums.
Kronecker: 128 x 128, k = 3, N = 1M: loo_predict_f_device, loo_log_density_device and loo_scores next to predict_f_device on the same rows
(the two per-point kernels they share).
Prints microseconds (median of the rounds), bytes per point, the share of the 8 TB/s HBM peak, and the ratios."""
import math
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import asvgp_amd as A  # noqa: E402
from asvgp_amd._lib import check, get_lib, stream_ptr  # noqa: E402

PEAK = 8.0e12
ROUNDS = 15


def timed(fns, rounds=ROUNDS, warm=3):
    """median device time (us) of every callable, the callables ALTERNATING inside each round"""
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[i].append(e0.elapsed_time(e1) * 1e3)
    return [float(np.median(t)) for t in ts]


def line(name, us, n, bytes_per_point):
    share = n * bytes_per_point / (us * 1e-6) / PEAK
    print("%-72s %9.1f us  %3d B/point  %5.1f %% of 8 TB/s" % (name, us, bytes_per_point, 100 * share), flush=True)


def composition(model, alpha, W, Pinv):
    """the same outputs without asvgp_loo_1d"""
    lib = get_lib()
    b = model.basis
    x, y, w = model.X.reshape(-1), model.y.reshape(-1), model.weights
    n = x.shape[0]
    s, v = float(model.likelihood.variance), float(model.kernel.variance)
    mu, var, g, unused = (torch.empty(n, dtype=torch.float64, device=x.device) for _ in range(4))

    def predict(band, prior, mean_out, var_out):
        check(lib.asvgp_predict_1d_h(model._h.ptr, x.data_ptr(), n, b.mesh.data_ptr(), b.mesh.shape[0], b.delta_np, b.order, b.m, alpha.data_ptr(),
                                     band.data_ptr(), prior, 1, mean_out.data_ptr(), var_out.data_ptr(), stream_ptr()), "predict_1d")

    def run():
        predict(W, v, mu, var)
        predict(Pinv, 0.0, unused, g)
        h = g / s if w is None else w * g / s
        om = 1.0 - h
        mean = (mu - h * y) / om
        vloo = var + g * (h / om)
        s2 = vloo + (s if w is None else s / w)
        sq = (y - mean) ** 2
        ld = -0.5 * (torch.log(2 * math.pi * s2) + sq / s2)
        scores = torch.stack([torch.tensor(float(n), dtype=torch.float64, device=x.device) if w is None else (w > 0).sum().double(),
                              ld.sum(), sq.sum(), h.max()])
        return mean, vloo, ld, scores
    return run


def probe_1d():
    N, M = 10_000_000, 2048
    rng = np.random.default_rng(1234)
    x = rng.uniform(0.02, 0.98, N)
    y = np.sin(20 * x) + 0.1 * rng.standard_normal(N)
    w = np.exp(rng.standard_normal(N))
    xd, yd, wd = (torch.from_numpy(a).cuda() for a in (x, y, w))
    ok = True
    for name, kw, b_in in (("weighted", dict(weights=wd), 24), ("unweighted", {}, 16)):
        m = A.GPR_1d((xd.reshape(-1, 1), yd.reshape(-1, 1)), A.Matern32(variance=1.0, lengthscales=0.05), A.B4Spline(0, 1, M), **kw)
        m.likelihood.variance.assign(0.01)
        alpha, W, Pinv = m._posterior_loo()
        comp = composition(m, alpha, W, Pinv)
        fused_rows = lambda: m._loo(want_mean=True, want_var=True, want_logdens=True, want_scores=True)
        fused_scores = lambda: m._loo(want_scores=True)
        t_s, t_r, t_c = timed([fused_scores, fused_rows, comp])
        fm, fv, fl, fs = fused_rows()
        cm, cv, cl, cs = comp()
        err = max(float((fm.reshape(-1) - cm).abs().max()), float((fv.reshape(-1) - cv).abs().max()),
                  float(((fs - cs).abs() / cs.abs().clamp_min(1.0)).max()))
        print("1-D  N = %d  M = %d  B4  Matern-3/2  %s   (fused and composed outputs agree to %.1e)" % (N, M, name, err))
        line("  asvgp_loo_1d, scores only", t_s, N, b_in)
        line("  asvgp_loo_1d, mean + var + logdens + scores", t_r, N, b_in + 24)
        # composition: 2 x (8 in, 16 out) for the predictions, then ~17 elementwise / reduction passes of 16 to 24 B each
        line("  composition: predict_1d_h twice + torch elementwise and sums", t_c, N, 200)
        print("  composition / fused per-row = %.2f (must be >= 2);   scores only / per-row = %.2f (must be <= 1)" % (t_c / t_r, t_s / t_r), flush=True)
        ok = ok and t_c >= 2.0 * t_r and t_s <= t_r
    print("1-D acceptance (composition >= 2 x fused per-row, scores only <= per-row): %s" % ("met" if ok else "NOT met"), flush=True)


def probe_kron():
    N, m, k = 1_000_000, 128, 3
    g = torch.Generator(device="cuda").manual_seed(5)
    X = torch.rand((N, 2), generator=g, device="cuda", dtype=torch.float64) * 0.94 + 0.03
    y = torch.sin(6 * X[:, :1]) * torch.cos(4 * X[:, 1:]) + 0.1 * torch.randn((N, 1), generator=g, device="cuda", dtype=torch.float64)
    w = torch.exp(torch.randn(N, generator=g, device="cuda", dtype=torch.float64))
    for name, kw in (("weighted", dict(weights=w)), ("unweighted", {})):
        mk = A.GPR_kron((X, y), [A.Matern32(), A.Matern32()], [A.B3Spline(0, 1, m), A.B3Spline(0, 1, m)], **kw)
        mk.likelihood.variance.assign(0.05)
        mk.predict_f_device(X[:16])                # (the factorisation and the selected inverse: once per theta, outside the timing)
        t_p, t_f, t_l, t_s = timed([lambda: mk.predict_f_device(X), mk.loo_predict_f_device, mk.loo_log_density_device, mk.loo_scores], rounds=7)
        print("Kronecker  N = %d  %d x %d  k = %d  %s" % (N, m, m, k, name))
        line("  predict_f_device on the training rows (the two per-point kernels)", t_p, N, 48)
        line("  loo_predict_f_device", t_f, N, 48)
        line("  loo_log_density_device", t_l, N, 48)
        line("  loo_scores (host floats)", t_s, N, 48)
        print("  loo_scores / predict_f_device = %.2f" % (t_s / t_p), flush=True)


if __name__ == "__main__":
    probe_1d()
    probe_kron()
