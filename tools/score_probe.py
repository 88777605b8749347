"""Held-out scores: the fused kernel (asvgp_score_1d) next to predict_f_device and to what a user could write without it, in ONE process,
alternating, after warm-up, timed with device events.

1-D: N = 10M unsorted held-out rows, M = 2048, B4, Matern-3/2, D = 1, held-out weights and none:
  (a) score, scores only (nothing of size N written),
  (b) predict_log_density_device,
  (c) predict_f_device on the same rows (the existing kernel: the yardstick for (a)),
  (d) the composition every model class has by default: predict_f_device + torch elementwise + sums,
  (e) the existing host route predict_log_density at N = 1M (wall clock: it copies to the host and finishes in numpy).
Kronecker: 128 x 128, k = 3, N = 1M: score next to predict_f_device on the same rows.
Prints microseconds (median of the rounds), the spread of (c) (its 10th to 90th percentile), the ratios, and the largest difference between
the fused and the composed outputs."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import asvgp_amd as A  # noqa: E402
from asvgp_amd.gpr import _GPModelSurface  # noqa: E402

ROUNDS = 15


def timed(fns, rounds=ROUNDS, warm=3):
    """device times (us) of every callable, the callables ALTERNATING inside each round: list of arrays"""
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
    return [np.asarray(t) for t in ts]


def line(name, t, n):
    print("%-78s %10.1f us   %7.3f ns/row" % (name, float(np.median(t)), 1e3 * float(np.median(t)) / n), flush=True)


def probe_1d():
    N, M, N_TRAIN, N_HOST = 10_000_000, 2048, 1_000_000, 1_000_000
    rng = np.random.default_rng(1234)
    f = lambda x: np.sin(20 * x)
    xt = rng.uniform(0.02, 0.98, N_TRAIN)
    yt = f(xt) + 0.1 * rng.standard_normal(N_TRAIN)
    x = rng.uniform(0.02, 0.98, N)
    y = f(x) + 0.1 * rng.standard_normal(N)
    w = np.exp(rng.standard_normal(N))
    xd, yd, wd = (torch.from_numpy(a).cuda() for a in (x.reshape(-1, 1), y.reshape(-1, 1), w))
    m = A.GPR_1d((xt.reshape(-1, 1), yt.reshape(-1, 1)), A.Matern32(variance=1.0, lengthscales=0.05), A.B4Spline(0, 1, M))
    m.likelihood.variance.assign(0.01)
    m._posterior()
    for name, wt in (("held-out weights", wd), ("no held-out weights", None)):
        fused_scores = lambda: m._score_device(xd, yd, wt)
        fused_rows = lambda: m._score_call(xd, yd, wt, want_logdens=True)[0]
        predict = lambda: m.predict_f_device(xd)
        composed = lambda: _GPModelSurface._score_device(m, xd, yd, wt)
        t_a, t_b, t_c, t_d = timed([fused_scores, fused_rows, predict, composed])
        spread = float(np.percentile(t_c, 90) - np.percentile(t_c, 10))
        sa, sd = fused_scores(), composed()
        ld_f, ld_c = fused_rows(), _GPModelSurface._heldout_moments(m, xd, yd, wt)[3]
        print("1-D  N = %d  M = %d  B4  Matern-3/2  D = 1  %s" % (N, M, name))
        line("  (a) score, scores only (asvgp_score_1d)", t_a, N)
        line("  (b) predict_log_density_device (asvgp_score_1d, logdens out)", t_b, N)
        line("  (c) predict_f_device on the same rows", t_c, N)
        line("  (d) composition: predict_f_device + torch elementwise + sums", t_d, N)
        print("  spread of (c), 10th to 90th percentile: %.1f us;  (a) - (c) = %+.1f us;  (a) within (c) + spread: %s"
              % (spread, float(np.median(t_a) - np.median(t_c)), "yes" if np.median(t_a) <= np.median(t_c) + spread else "NO"))
        print("  (d) / (a) = %.2f;  fused vs composed: logdens max |diff| = %.2e, scores max relative diff = %.2e"
              % (float(np.median(t_d) / np.median(t_a)), float((ld_f - ld_c).abs().max()), float(((sa - sd).abs() / sd.abs().clamp_min(1.0)).max())),
              flush=True)
    # (e) the host route, wall clock (it ends on the host), at 1M rows
    xh, yh = x[:N_HOST].reshape(-1, 1), y[:N_HOST].reshape(-1, 1)
    xhd, yhd = xd[:N_HOST].contiguous(), yd[:N_HOST].contiguous()
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.predict_log_density((xhd, yh))
        ts.append((time.perf_counter() - t0) * 1e6)
    line("  (e) host route predict_log_density, N = 1M (wall clock, device-resident X)", np.asarray(ts), N_HOST)
    t_a1 = timed([lambda: m._score_device(xhd, yhd, None)])[0]
    line("      score, scores only, on the same 1M rows", t_a1, N_HOST)
    print("  (e) per row / (a) per row = %.0f" % (float(np.median(ts)) / float(np.median(t_a1))), flush=True)


def probe_kron():
    N, mm, k = 1_000_000, 128, 3
    g = torch.Generator(device="cuda").manual_seed(5)
    draw = lambda n: torch.rand((n, 2), generator=g, device="cuda", dtype=torch.float64) * 0.94 + 0.03
    fy = lambda X: torch.sin(6 * X[:, :1]) * torch.cos(4 * X[:, 1:]) + 0.1 * torch.randn((X.shape[0], 1), generator=g, device="cuda", dtype=torch.float64)
    X, Xn = draw(N), draw(N)
    y, yn = fy(X), fy(Xn)
    w = torch.exp(torch.randn(N, generator=g, device="cuda", dtype=torch.float64))
    mk = A.GPR_kron((X, y), [A.Matern32(), A.Matern32()], [A.B3Spline(0, 1, mm), A.B3Spline(0, 1, mm)])
    mk.likelihood.variance.assign(0.05)
    mk.predict_f_device(Xn[:16])                   # (the factorisation and the selected inverse: once per theta, outside the timing)
    t_p, t_s, t_w = timed([lambda: mk.predict_f_device(Xn), lambda: mk._score_device(Xn, yn, None), lambda: mk._score_device(Xn, yn, w)], rounds=7)
    print("Kronecker  N = %d  %d x %d  k = %d" % (N, mm, mm, k))
    line("  predict_f_device (the two per-point kernels)", t_p, N)
    line("  score (composed on the device), no held-out weights", t_s, N)
    line("  score (composed on the device), held-out weights", t_w, N)
    print("  score / predict_f_device = %.2f (%.2f weighted)" % (float(np.median(t_s) / np.median(t_p)), float(np.median(t_w) / np.median(t_p))), flush=True)


if __name__ == "__main__":
    probe_1d()
    probe_kron()
