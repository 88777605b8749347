"""CPU: the closed form behind asvgp_weight_grad_1d (include/asvgp_hip.h) against central differences of a dense numpy ELBO_w, the scaling
identity sum_i w_i d ELBO_w / d w_i = -s d ELBO_w / d s, the export of the two entry points, the validation of group labels on CPU
tensors and the signatures of the three new methods.  No GPU is touched."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import asvgp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("asvgp_weight_grad_workspace_bytes", "asvgp_weight_grad_1d")


def problem(D, N=40, M=7, order=2, seed=0):         # (order 3 needs M >= 8 boundary bands)
    rng = np.random.default_rng(seed + D)
    ob = O.Basis(order, 0, 1, M)
    x = rng.uniform(0.02, 0.98, N)
    y = np.stack([np.sin(5 * (d + 1) * x) for d in range(D)], 1) + 0.2 * rng.normal(size=(N, D))
    w = np.exp(rng.normal(size=N))
    Phi = ob.evaluate_basis(x.reshape(-1, 1), sparse=False)          # (M, N)
    Kuu = O.band_to_dense_sym(O.make_Kuu(ob, O.MATERN32, 1.2, 0.3))
    return Phi, Kuu, 1.2, y, w


def elbo_w(Phi, Kuu, v, s, y, w):
    """The weighted bound (include/asvgp_hip.h, "Per-observation noise weights"), dense: the trace terms counted once for D outputs."""
    D = y.shape[1]
    pos = w > 0
    A = (Phi * w[None, :]) @ Phi.T
    b = Phi @ (w[:, None] * y)
    LP = np.linalg.cholesky(Kuu + A / s)
    LK = np.linalg.cholesky(Kuu)
    c = np.linalg.solve(LP, b) / s
    return (-0.5 * D * pos.sum() * np.log(2 * np.pi * s) + 0.5 * D * np.sum(np.log(w[pos])) - D * np.sum(np.log(np.diag(LP)))
            + D * np.sum(np.log(np.diag(LK))) - 0.5 * np.sum(w[:, None] * y * y) / s + 0.5 * np.sum(c * c)
            - 0.5 * w.sum() * v / s + 0.5 * np.trace(np.linalg.solve(Kuu, A)) / s)


def closed_form(Phi, Kuu, v, s, y, w):
    D = y.shape[1]
    Pinv = np.linalg.inv(Kuu + (Phi * w[None, :]) @ Phi.T / s)
    alpha = Pinv @ (Phi @ (w[:, None] * y)) / s
    g = np.sum(Phi * (Pinv @ Phi), axis=0)
    q = np.sum(Phi * np.linalg.solve(Kuu, Phi), axis=0)
    r = y - Phi.T @ alpha
    var = v - q + g
    return 0.5 * (D / w - D * g / s - np.sum(r * r, axis=1) / s - (var - g) / s)


@pytest.mark.parametrize("D", [1, 3])
def test_closed_form_against_central_differences(D):
    Phi, Kuu, v, y, w = problem(D)
    s = 0.05
    grad = closed_form(Phi, Kuu, v, s, y, w)
    for i in range(w.shape[0]):
        h = 1e-5 * w[i]
        wp, wm = w.copy(), w.copy()
        wp[i] += h
        wm[i] -= h
        fd = (elbo_w(Phi, Kuu, v, s, y, wp) - elbo_w(Phi, Kuu, v, s, y, wm)) / (2 * h)
        assert abs(fd - grad[i]) <= 1e-6 * max(abs(grad[i]), D / w[i])


@pytest.mark.parametrize("D", [1, 3])
def test_scaling_identity(D):
    """scaling every weight by c is scaling s by 1 / c (up to the constant D / 2 sum log w): sum_i w_i grad_i = -s d ELBO_w / d s"""
    Phi, Kuu, v, y, w = problem(D, seed=5)
    s = 0.05
    lhs = float(np.sum(w * closed_form(Phi, Kuu, v, s, y, w)))
    h = 1e-6 * s
    ds = (elbo_w(Phi, Kuu, v, s + h, y, w) - elbo_w(Phi, Kuu, v, s - h, y, w)) / (2 * h)
    assert abs(lhs + s * ds) <= 1e-6 * np.sum(np.abs(w * closed_form(Phi, Kuu, v, s, y, w)))


def test_exported_and_declared():
    from asvgp_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "asvgp_hip.h")).read()
    lib = _lib.get_lib()
    for n in NAMES:
        assert re.search(r"\b%s\(" % n, hdr), "%s is not declared in the header" % n
        assert n in _lib.SIGNATURES
        assert getattr(lib, n) is not None
    loo, wg = _lib.SIGNATURES["asvgp_loo_1d"], _lib.SIGNATURES["asvgp_weight_grad_1d"]
    assert wg[1][:16] == loo[1][:16]                             # asvgp_loo_1d's arguments up to the noise variance, then groups, G, grad, gsum
    assert lib.asvgp_weight_grad_workspace_bytes(2048, 4, 1, 1) == lib.asvgp_loo_workspace_bytes(2048, 4, 1)
    assert lib.asvgp_weight_grad_workspace_bytes(2048, 4, 1, 1024) == 8 * 1024 * 2048      # 1024 workgroup rows of 2 G doubles
    for G in (0, -1, 1025):
        assert lib.asvgp_weight_grad_workspace_bytes(2048, 4, 1, G) == 0
    assert lib.asvgp_weight_grad_workspace_bytes(16, 7, 1, 1) == 0 and lib.asvgp_weight_grad_workspace_bytes(16, 3, 0, 1) == 0


def test_group_validation_on_cpu_tensors():
    from asvgp_amd import gpr
    labels, G = gpr._prepare_groups(torch.tensor([2, 0, 2, 5], dtype=torch.int32), 4, "cpu", "t")
    assert labels.dtype == torch.int64 and labels.tolist() == [2, 0, 2, 5] and G == 6
    assert gpr._prepare_groups(np.array([[1], [0]]), 2, "cpu", "t")[1] == 2          # (N, 1) is accepted, as folds are
    with pytest.raises(ValueError, match="shape"):
        gpr._prepare_groups(torch.zeros(3, dtype=torch.int64), 4, "cpu", "t")
    with pytest.raises(ValueError, match="shape"):
        gpr._prepare_groups(torch.zeros((4, 2), dtype=torch.int64), 4, "cpu", "t")
    with pytest.raises(ValueError, match="integer"):
        gpr._prepare_groups(torch.zeros(4, dtype=torch.float64), 4, "cpu", "t")
    with pytest.raises(ValueError, match="row 2 has group -3"):
        gpr._prepare_groups(torch.tensor([0, 1, -3, 1]), 4, "cpu", "t")


def test_signatures():
    from asvgp_amd import gpr
    for cls in (gpr.GPR_1d, gpr.GPR_kron, gpr.GPR_additive):
        assert list(inspect.signature(cls.weight_gradient_device).parameters) == ["self"]
        assert list(inspect.signature(cls.noise_group_gradient).parameters) == ["self", "groups"]
        sig = inspect.signature(cls.fit_noise_groups)
        assert list(sig.parameters) == ["self", "groups", "maxiter", "pinned"]
        assert sig.parameters["maxiter"].default == 200 and sig.parameters["pinned"].default == 0
