"""Gradient of the bound in the weights: the fused kernel (asvgp_weight_grad_1d) against what a user could write without it, in ONE process,
alternating, after warm-up, timed with device events.

N = 10M, M = 2048, B4, Matern-3/2, unsorted x, weighted:
  asvgp_weight_grad_1d with the per-row output,
  asvgp_weight_grad_1d with gsum only (nothing of size N written) for G = 1 (no labels: the fixed-order records), 16 and 1024 (bins in LDS),
  asvgp_loo_1d with the scores alone: the pass of the same read traffic,
  the composition: predict_f_device and loo_predict_f_device (g, which D > 1 needs, from the two variances), then the formula in torch;
  its group sums with index_add_ (what the Python surface does above 1024 groups and for GPR_kron) and with torch.bincount.
Prints microseconds (median of the rounds), bytes per point, the share of the 8 TB/s HBM peak, and the ratios."""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
import asvgp_amd as A  # noqa: E402

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
    print("%-76s %9.1f us  %3d B/point  %5.1f %% of 8 TB/s" % (name, us, bytes_per_point, 100 * share), flush=True)


def composition(model, labels, G, sums):
    """the per-row gradient (and, sums = "index_add" / "bincount" / None, the group sums) without asvgp_weight_grad_1d (D = 1)"""
    X, y, w = model.X, model.y.reshape(-1), model.weights
    s = float(model.likelihood.variance)

    def run():
        mu, var = model.predict_f_device(X)
        _, vloo = model.loo_predict_f_device()
        var, vloo = var.reshape(-1), vloo.reshape(-1)
        # vloo - var = g h / (1 - h) with h = w g / s: a quadratic in g
        d = (vloo - var) * s / w
        g = 0.5 * (torch.sqrt(d * d + 4 * d) - d)
        r = y - mu.reshape(-1)
        grad = 0.5 * (1.0 / w - (r * r + var) / s)
        out = None
        if sums == "index_add":
            out = torch.zeros((G, 2), dtype=torch.float64, device=w.device)
            out[:, 0].index_add_(0, labels, (w > 0).double())
            out[:, 1].index_add_(0, labels, w * grad)
        elif sums == "bincount":
            out = torch.stack([torch.bincount(labels, weights=(w > 0).double(), minlength=G),
                               torch.bincount(labels, weights=w * grad, minlength=G)], 1)
        return grad, out, g
    return run


def main():
    N, M = 10_000_000, 2048
    rng = np.random.default_rng(1234)
    x = rng.uniform(0.02, 0.98, N)
    y = np.sin(20 * x) + 0.1 * rng.standard_normal(N)
    w = np.exp(rng.standard_normal(N))
    xd, yd, wd = (torch.from_numpy(a).cuda() for a in (x, y, w))
    m = A.GPR_1d((xd.reshape(-1, 1), yd.reshape(-1, 1)), A.Matern32(variance=1.0, lengthscales=0.05), A.B4Spline(0, 1, M), weights=wd)
    m.likelihood.variance.assign(0.01)
    m._posterior_loo()
    m._posterior()
    labels = {G: torch.from_numpy(rng.integers(0, G, N)).cuda() for G in (16, 1024)}
    l32 = {G: t.to(torch.int32) for G, t in labels.items()}
    comp_rows, comp_bin, comp = (composition(m, labels[16], 16, how) for how in (None, "bincount", "index_add"))
    fns = [lambda: m._weight_grad(True), lambda: m._weight_grad(False, None, 1), lambda: m._weight_grad(False, l32[16], 16),
           lambda: m._weight_grad(False, l32[1024], 1024), lambda: m._loo(want_scores=True), comp_rows, comp_bin]
    t_row, t_1, t_16, t_1024, t_loo, t_cr, t_cb = timed(fns)
    t_c, = timed([comp], rounds=3, warm=1)          # (seconds: 10M fp64 atomics on 32 addresses)
    grad = m._weight_grad(True)[0]
    cgrad, csum, _ = comp()
    fsum = m._weight_grad(False, l32[16], 16)[1]
    err = float(((grad - cgrad).abs() / (1.0 + cgrad.abs())).max())
    serr = float(((fsum - csum).abs() / csum.abs().clamp_min(1.0)).max())
    print("N = %d  M = %d  B4  Matern-3/2  weighted   (fused and composed: rows agree to %.1e relative, group sums to %.1e)" % (N, M, err, serr))
    line("  asvgp_weight_grad_1d, per-row output", t_row, N, 24 + 8)
    line("  asvgp_weight_grad_1d, gsum only, G = 1 (no labels)", t_1, N, 24)
    line("  asvgp_weight_grad_1d, gsum only, G = 16", t_16, N, 28)
    line("  asvgp_weight_grad_1d, gsum only, G = 1024", t_1024, N, 28)
    line("  asvgp_loo_1d, scores only (the same read traffic)", t_loo, N, 24)
    line("  composition, per-row gradient: predict_f_device + loo_predict_f_device + torch", t_cr, N, 300)
    line("  composition, + group sums with torch.bincount, G = 16", t_cb, N, 350)
    line("  composition, + group sums with index_add_, G = 16", t_c, N, 350)
    print("  gsum only G = 1 / loo scores only = %.2f;   composed rows / per-row = %.2f;   composed bincount / gsum G = 16 = %.2f;   "
          "composed index_add_ / gsum G = 16 = %.0f" % (t_1 / t_loo, t_cr / t_row, t_cb / t_16, t_c / t_16), flush=True)


if __name__ == "__main__":
    main()
