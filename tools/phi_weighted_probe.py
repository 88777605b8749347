"""Weighted against unweighted Phi pass, in ONE call, alternating, after warm-up, timed with device events.

1-D: N = 10M, M = 2048, B4, Matern-3/2, unsorted and sorted x: the unweighted pass (algorithm auto), the weighted register-moment
kernel (16), the weighted general kernel (11) and what a user can do without the feature - the weighted statistics through torch on
the same GPU (asvgp_phi_evaluate_1d rows + index_add_ of the weighted products).
Kronecker: 128 x 128, k = 3, N = 1M: the cell-sorted matrix-core pass, unweighted and weighted.
Prints microseconds (median of the rounds), bytes per point, the share of the 8 TB/s HBM peak, and the ratios."""
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


def line(name, us, n, bytes_per_point, base=None):
    share = n * bytes_per_point / (us * 1e-6) / PEAK
    tail = "" if base is None else "   x%.2f of the unweighted pass" % (us / base)
    print("%-58s %9.1f us  %3d B/point  %5.1f %% of 8 TB/s%s" % (name, us, bytes_per_point, 100 * share, tail), flush=True)


def torch_weighted_stats(model, w):
    """the weighted statistics without the feature: Phi rows from asvgp_phi_evaluate_1d, weighted products through index_add_"""
    lib = get_lib()
    b, k, M = model.basis, model.bandwidth, model.basis.m
    x, y = model.X.reshape(-1), model.y.reshape(-1)
    n = x.shape[0]
    rows = torch.empty((k + 1, n), dtype=torch.int64, device=x.device)
    vals = torch.empty((k + 1, n), dtype=torch.float64, device=x.device)
    band = torch.zeros((k + 1) * M, dtype=torch.float64, device=x.device)
    rhs = torch.zeros(M, dtype=torch.float64, device=x.device)

    def run():
        check(lib.asvgp_phi_evaluate_1d(x.data_ptr(), n, b.mesh.data_ptr(), b.mesh.shape[0], b.delta_np, k, 0, rows.data_ptr(), vals.data_ptr(),
                                        stream_ptr()), "phi_evaluate_1d")
        band.zero_(); rhs.zero_()
        wy = w * y
        for i in range(k + 1):
            rhs.index_add_(0, rows[i], vals[i] * wy)
            wv = w * vals[i]
            for j in range(i, k + 1):          # rows[i] >= rows[j]: sub-diagonal j - i, column rows[j]
                band.index_add_(0, (j - i) * M + rows[j], wv * vals[j])
        return (w * y * y).sum(), w.sum(), torch.log(w).sum()
    return run, band, rhs


def probe_1d():
    N, M = 10_000_000, 2048
    rng = np.random.default_rng(1234)
    x = rng.uniform(1e-9, 1 - 1e-9, N)
    y = np.sin(20 * x) + 0.1 * rng.standard_normal(N)
    w = np.exp(rng.standard_normal(N))
    for name, xs in (("unsorted", x), ("sorted", np.sort(x))):
        xd, yd, wd = (torch.from_numpy(a).cuda() for a in (xs, y, w))
        mk = lambda **kw: A.GPR_1d((xd.reshape(-1, 1), yd.reshape(-1, 1)), A.Matern32(variance=1.0, lengthscales=0.05), A.B4Spline(0, 1, M), **kw)
        mu, mw, mg = mk(), mk(weights=wd), mk(weights=wd)
        mg._h.set_phi_algorithm(1)
        run_t, band, rhs = torch_weighted_stats(mu, wd)
        t_u, t_w, t_g, t_t = timed([mu._phi_pass_local, mw._phi_pass_local, mg._phi_pass_local, run_t])
        assert (mu._h.phi_last_algorithm(), mw._h.phi_last_algorithm(), mg._h.phi_last_algorithm()) == (6, 16, 11)
        k1 = 5 * M
        err = max(float((mw._stats[:k1] - band).abs().max() / band.abs().max()), float((mw._stats[k1:k1 + M] - rhs).abs().max() / rhs.abs().max()))
        print("1-D  N = %d  M = %d  B4  %s   (torch route agrees with kernel 16 to %.1e)" % (N, M, name, err))
        line("  unweighted pass (algorithm 6) + reduce", t_u, N, 16)
        line("  weighted register-moment kernel (16) + reduces", t_w, N, 24, t_u)
        line("  weighted general kernel (11) + reduces", t_g, N, 24, t_u)
        line("  torch: phi_evaluate_1d + 20 index_add_", t_t, N, 24, t_u)
        print("  weighted (16) / unweighted = %.2f (bytes read: 24 / 16 = 1.50);   torch route / weighted (16) = %.1f" % (t_w / t_u, t_t / t_w), flush=True)


def probe_kron():
    N, m, k = 1_000_000, 128, 3
    g = torch.Generator(device="cuda").manual_seed(5)
    X = torch.rand((N, 2), generator=g, device="cuda", dtype=torch.float64) * 0.998 + 0.001
    y = torch.sin(6 * X[:, :1]) * torch.cos(4 * X[:, 1:]) + 0.1 * torch.randn((N, 1), generator=g, device="cuda", dtype=torch.float64)
    w = torch.exp(torch.randn(N, generator=g, device="cuda", dtype=torch.float64))
    mk = lambda **kw: A.GPR_kron((X, y), [A.Matern32(), A.Matern32()], [A.B3Spline(0, 1, m), A.B3Spline(0, 1, m)], **kw)
    mu, mw = mk(), mk(weights=w)
    t_u, t_w, t_pu, t_pw = timed([mu._phi_pass_local, mw._phi_pass_local, lambda: mu._phi_pass_local(sorted_cells=False),
                                  lambda: mw._phi_pass_local(sorted_cells=False)], rounds=7)
    print("Kronecker  N = %d  %d x %d  k = %d" % (N, m, m, k))
    line("  cell-sorted matrix-core pass, unweighted", t_u, N, 24)
    line("  cell-sorted matrix-core pass, weighted", t_w, N, 32, t_u)
    line("  per-point atomic pass, unweighted", t_pu, N, 24)
    line("  per-point atomic pass, weighted", t_pw, N, 32, t_pu)
    print("  weighted / unweighted (cell-sorted) = %.2f (bytes read: 32 / 24 = 1.33)" % (t_w / t_u), flush=True)


if __name__ == "__main__":
    probe_1d()
    probe_kron()
