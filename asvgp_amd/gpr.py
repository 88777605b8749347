"""GPR_1d: drop-in for asvgp/gpr.py:18-136 hosted on the MI355X HIP library.

Same surface: GPR_1d(data=(X[N,1], y[N,D]), kernel, basis) with .elbo(), .maximum_log_likelihood_objective(),
.training_loss(), .predict_f(Xnew, full_cov=False, full_output_cov=False, batch=False) and the attributes
X, y, bandwidth, Kuf_y, KufKfu, KufKfu_sparse, tr_yTy, kernel, likelihood.variance, inducing_features.
Additions (not in the reference): elbo_and_grad() (analytic gradient, replacing TF autodiff through the
banded_matrices op gradients), fit() (L-BFGS-B driver, replacing gpflow.optimizers.Scipy), process_group= for
N-sharded construction over RCCL.
"""
import ctypes
import math
import time

import numpy as np
import torch
import torch.distributed as dist

from . import kernels, utils
from . import kernels as kernels_mod
from ._lib import AsvgpError, Handle, check, f64c, get_lib, require_cuda, stream_ptr
from .banded import NotPositiveDefiniteError
from .dist import allreduce_stats
from .inducing_features import SplineFeatures1D


def _to_device(a, device):
    t = torch.as_tensor(a)
    return f64c(t.to(device))


def _require_inside(col, a, b, strict, what):
    """gpr.py:24-25 asserts a < X < b; raised explicitly so that `python -O` cannot strip it: the fixed-point Phi pass
    assumes t in [0, 1] and would return finite but wrong statistics for points outside the mesh (or NaN)."""
    if col.numel() == 0:
        return
    lo, hi = torch.aminmax(col)
    lo, hi = lo.item(), hi.item()
    ok = (lo > a and hi < b) if strict else (lo >= a and hi <= b)
    if not ok or lo != lo or hi != hi:
        raise AssertionError("%s: inputs must lie %s the basis domain (%g, %g); got [%g, %g]"
                             % (what, "strictly inside" if strict else "inside", a, b, lo, hi))


def _prepare_weights(weights, n, dev, what):
    """Per-observation weights (noise variance sigma2 / w_i): array-like (N,) or (N, 1) -> fp64 device tensor (N,), validated once
    like _require_inside: every weight finite and >= 0, else ValueError naming the first bad row."""
    w = _to_device(weights, dev)
    if w.dim() == 2 and w.shape[1] == 1:
        w = w.reshape(-1)
    if w.dim() != 1 or w.shape[0] != n:
        raise ValueError("%s: weights must have shape (N,) or (N, 1) with N = %d rows; got %s" % (what, n, tuple(torch.as_tensor(weights).shape)))
    bad = ~(torch.isfinite(w) & (w >= 0))
    if w.numel() and bool(bad.any()):
        i = int(torch.nonzero(bad)[0].item())
        raise ValueError("%s: weights must be finite and >= 0; row %d has weight %r" % (what, i, w[i].item()))
    return w.contiguous()


def _predictive_weights(weights, n):
    """weights of predict_y / predict_log_density for the NEW points: (n, 1) numpy column, every entry finite and > 0."""
    w = np.asarray(weights.cpu() if isinstance(weights, torch.Tensor) else weights, dtype=np.float64).reshape(-1, 1)
    if w.shape[0] != n:
        raise ValueError("weights must have one entry per new point (%d); got %d" % (n, w.shape[0]))
    if not np.all(np.isfinite(w) & (w > 0)):
        raise ValueError("weights of new points must be finite and > 0 (noise variance sigma2 / w)")
    return w


def _prepare_heldout(data, weights, ncol, D, dev, what):
    """Held-out rows (Xnew (n, ncol), Ynew (n, D)) and their weights -> fp64 device tensors (X (n, ncol), Y (n, D), w (n,) or None),
    validated before anything is launched: ValueError for a wrong number of columns or rows, or a weight that is not finite and >= 0."""
    Xnew, Ynew = data
    X = _to_device(Xnew, dev)
    if X.dim() == 1 and ncol == 1:
        X = X.reshape(-1, 1)
    if X.dim() != 2 or X.shape[1] != ncol:
        raise ValueError("%s: Xnew must have shape (n, %d); got %s" % (what, ncol, tuple(X.shape)))
    n = X.shape[0]
    Y = _to_device(Ynew, dev)
    if Y.dim() == 1 and D == 1:
        Y = Y.reshape(-1, 1)
    if Y.dim() != 2 or tuple(Y.shape) != (n, D):
        raise ValueError("%s: Ynew must have shape (%d, %d), one row per row of Xnew; got %s" % (what, n, D, tuple(Y.shape)))
    w = None if weights is None else _prepare_weights(weights, n, dev, what)
    return X.contiguous(), Y.contiguous(), w


def _prepare_labels(labels, n, dev, what, noun):
    """Integer labels (noun = "fold" / "group") of this rank's n rows -> int64 device tensor (n,).  ValueError, before anything is
    launched, for a wrong shape, a label that is not an integer, or a negative label."""
    f = torch.as_tensor(labels)
    if f.dim() == 2 and f.shape[1] == 1:
        f = f.reshape(-1)
    if f.dim() != 1 or f.shape[0] != n:
        raise ValueError("%s: %ss must have shape (N,) with N = %d rows; got %s" % (what, noun, n, tuple(f.shape)))
    if f.dtype.is_floating_point or f.dtype == torch.bool or f.dtype.is_complex:
        raise ValueError("%s: %ss must be an integer array; got %s" % (what, noun, f.dtype))
    f = f.to(device=dev, dtype=torch.int64).contiguous()
    if n and int(f.min().item()) < 0:
        i = int(torch.nonzero(f < 0)[0].item())
        raise ValueError("%s: %ss must be >= 0; row %d has %s %d" % (what, noun, i, noun, int(f[i].item())))
    return f


def _prepare_folds(folds, n, weights, dev, what):
    """Fold labels of this rank's n rows -> (int64 device tensor (n,), per-fold count of rows with positive weight (K_local,) int64).
    ValueError for a wrong shape, a label that is not an integer, or a negative label."""
    f = _prepare_labels(folds, n, dev, what, "fold")
    pos = f if weights is None else f[weights > 0]
    counts = torch.bincount(pos, minlength=(int(f.max().item()) + 1) if n else 0)
    return f, counts


def _prepare_groups(groups, n, dev, what):
    """Group labels of this rank's n rows -> (int64 device tensor (n,), G_local = max + 1; 0 for no rows); validated as folds are."""
    g = _prepare_labels(groups, n, dev, what, "group")
    return g, (int(g.max().item()) + 1) if n else 0


def _require_folds_populated(counts, what):
    empty = torch.nonzero(counts <= 0)
    if counts.numel() == 0 or empty.numel():
        raise ValueError("%s: %s" % (what, "no folds" if counts.numel() == 0 else
                                     "fold %d has no row of positive weight" % int(empty[0].item())))


def _score_dict(n, ld, sq, chi, D):
    """The held-out scores as Python floats, with the derived nlpd, rmse and mean_chi2 (NaN for an empty set)."""
    nan = float("nan")
    return dict(n=n, log_density=ld, sq_err=sq, chi2=chi, nlpd=-ld / n if n else nan, rmse=math.sqrt(sq / (n * D)) if n else nan,
                mean_chi2=chi / (n * D) if n else nan)


class _ShardedStats:
    """N-sharded statistics: every (re)run of the local Phi pass is followed by the ONE all-reduce of the
    packed buffer, so `_stats` (and the views KufKfu / Kuf_y / tr_yTy into it) are always the global sums."""
    _pg = None
    _distributed = False

    def _setup_dist(self, process_group, distributed):
        self._pg = process_group
        self._distributed = bool(process_group is not None if distributed is None else distributed)

    def _allreduce_stats(self):
        if self._distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size(self._pg) > 1:
            dist.all_reduce(self._stats, op=dist.ReduceOp.SUM, group=self._pg)

    def phi_pass(self, allreduce=True, **kw):
        """(Re)run the fused N-dependent pass over this rank's rows; with allreduce=True (default) a sharded model then
        sums the packed buffer across ranks, exactly as the constructor does.  allreduce=False leaves the LOCAL statistics
        in place (bench.py times the collective separately)."""
        self._phi_pass_local(**kw)
        if allreduce:
            h = getattr(self, "_h", None)
            if h is not None and h.deferred and self._distributed:
                # deferred mode parks the workgroup partials; the collective must see the reduced LOCAL statistics
                check(get_lib().asvgp_phi_reduce_1d(h.ptr, stream_ptr()), "phi_reduce_1d")
            self._allreduce_stats()
        return self._stats


def _require_derivative(kernel, what):
    """f has a mean-square derivative under Matern-3/2 and 5/2 only: Matern-1/2's k''(0) is unbounded.  Raised before any launch."""
    if kernel.kind not in (kernels.Matern32.kind, kernels.Matern52.kind):
        raise ValueError("%s: the %s kernel has no mean-square derivative (its k''(0) is unbounded); gradient predictions need "
                         "Matern32 or Matern52" % (what, type(kernel).__name__))


class HostArray(np.ndarray):
    """numpy array with the one tensor method the reference's scripts call on model outputs: `.numpy()` (electricity.py:132-138:
    `model.predict_y(X)[0].numpy()`, `model.predict_log_density((X, y)).numpy()`)."""

    def numpy(self):
        return np.asarray(self)


def _host(a):
    return np.asarray(a).view(HostArray)


class _GPModelSurface:
    """The bits of gpflow.models.GPModel the reference's scripts call on every model class: trainable_variables
    (example.py:32, eNATL60.py:89), predict_y and predict_log_density (electricity.py:132,138) for the Gaussian likelihood."""

    @property
    def trainable_variables(self):
        return self.trainable_parameters

    # per-observation weights (None: the unweighted model)
    weights = None
    weight_sum = None
    log_weight_sum = None

    def _set_weight_sums(self, n_local, wstats_local, process_group):
        """Global [N+, sum w, sum log w] of a weighted model from this rank's wstats = [sum w, sum log w, N+] (device, 3 doubles); the
        payload collective of a sharded model is the usual one, the three scalars ride with the row count."""
        if self._distributed:
            _, ws = allreduce_stats(self._stats, n_local, process_group, wstats=wstats_local)
        else:
            ws = wstats_local.tolist()
        self.weight_sum, self.log_weight_sum, self.num_data = float(ws[0]), float(ws[1]), int(round(ws[2]))

    def predict_y(self, Xnew, weights=None):
        """Mean and variance of a new observation; weights: per-point w of the NEW points (noise variance sigma2 / w; default 1)."""
        mean, var = self.predict_f(Xnew)
        noise = float(self.likelihood.variance)
        if weights is not None:
            noise = noise / _predictive_weights(weights, np.asarray(var).shape[0])
        return _host(mean), _host(var + noise)

    def predict_log_density(self, data, weights=None):
        """gpflow GPModel.predict_log_density with the Gaussian likelihood: log N(y | mean, var_f + sigma2) summed over the output
        dimension - shape (N,) (gpflow/likelihoods/scalar_continuous.py Gaussian._predict_log_density: reduce_sum over the last axis).
        weights: as predict_y."""
        Xnew, Ynew = data
        mean, var = self.predict_y(Xnew, weights)
        Ynew = np.asarray(Ynew.cpu() if isinstance(Ynew, torch.Tensor) else Ynew, dtype=np.float64).reshape(mean.shape)
        return _host(np.sum(-0.5 * (np.log(2 * np.pi * var) + (Ynew - mean) ** 2 / var), axis=-1))

    # -- closed-form leave-one-out predictions (GPR_1d, and GPR_kron with d = 2) ---------------------------------------------
    def _loo_unsupported(self, what):
        raise NotImplementedError("%s.%s: closed-form leave-one-out predictions exist for GPR_1d and for GPR_kron with d = 2 only"
                                  % (type(self).__name__, what))

    def loo_predict_f_device(self):
        self._loo_unsupported("loo_predict_f_device")

    def loo_log_density_device(self):
        self._loo_unsupported("loo_log_density_device")

    def _loo_scores_device(self):
        self._loo_unsupported("loo_scores")

    def loo_predict_f(self):
        """loo_predict_f_device as numpy: (mean (N, D), var (N, 1)) of f(x_i) given every training row but i."""
        mean, var = self.loo_predict_f_device()
        return mean.cpu().numpy(), var.cpu().numpy()

    def loo_scores(self):
        """Exact leave-one-out cross-validation scores over the rows with w_i > 0, as Python floats: n, log_density = sum_i log p(y_i | y_-i),
        sq_err = sum_i sum_d (y_id - mean_id)^2, max_leverage = max_i h_i, and the derived nlpd = -log_density / n and
        rmse = sqrt(sq_err / (n D)).  On a sharded model every rank streams its own rows against the global posterior; the sums are
        all-reduced with SUM and the leverage with MAX, so every rank returns the global scores."""
        sc = self._loo_scores_device()                      # device, 4 doubles: [n, log density, squared error, max leverage]
        if self._distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size(self._pg) > 1:
            sums, mx = sc[:3].clone(), sc[3:].clone()
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=self._pg)
            dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=self._pg)
            sc = torch.cat([sums, mx])
        n, ld, sq, mx = sc.tolist()
        D = self.y.shape[1]
        return dict(n=n, log_density=ld, sq_err=sq, max_leverage=mx, nlpd=-ld / n if n else float("nan"),
                    rmse=math.sqrt(sq / (n * D)) if n else float("nan"))

    # -- held-out scores on the device (every model class; GPR_1d fuses them into one kernel) ------------------------------
    def _is_sharded(self):
        return bool(self._distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size(self._pg) > 1)

    def _heldout(self, data, weights, what):
        return _prepare_heldout(data, weights, self.X.shape[1], self.y.shape[1], self._stats.device, "%s.%s" % (type(self).__name__, what))

    def _noise_column(self, w, n):
        """sigma2 / w_i as an (n, 1) device column (sigma2 for a row with weight 0), or the float sigma2 without weights"""
        s = float(self.likelihood.variance)
        if w is None:
            return s
        pos, sv = w > 0, torch.full_like(w, s)
        return torch.where(pos, sv / torch.where(pos, w, torch.ones_like(w)), sv).reshape(n, 1)   # (tensor / tensor: a true division)

    def predict_y_device(self, Xnew, weights=None):
        """predict_y on the device: (mean (n, D), var_f + sigma2 / w (n, 1)) as device tensors, nothing copied to the host.  weights: per-row
        w of the NEW rows, finite and >= 0 (a row with weight 0 takes noise variance sigma2)."""
        what = "%s.predict_y_device" % type(self).__name__
        dev = self._stats.device
        X = _to_device(Xnew, dev)
        if X.dim() == 1 and self.X.shape[1] == 1:
            X = X.reshape(-1, 1)
        if X.dim() != 2 or X.shape[1] != self.X.shape[1]:
            raise ValueError("%s: Xnew must have shape (n, %d); got %s" % (what, self.X.shape[1], tuple(X.shape)))
        w = None if weights is None else _prepare_weights(weights, X.shape[0], dev, what)
        mean, var = self.predict_f_device(X)
        return mean, var + self._noise_column(w, X.shape[0])

    def _heldout_moments(self, X, Y, w):
        """(mean (n, D), s2 (n, 1), squared error (n,), logdens (n,)) of validated held-out rows, composed in torch on the device"""
        mean, var = self.predict_f_device(X)
        s2 = var + self._noise_column(w, X.shape[0])
        sq = ((Y - mean) ** 2).sum(-1)
        ld = -0.5 * (Y.shape[1] * torch.log(2 * math.pi * s2.reshape(-1)) + sq / s2.reshape(-1))
        return mean, s2, sq, ld

    def predict_log_density_device(self, data, weights=None):
        """predict_log_density on the device: sum_d log N(y_id | mean_id, var_f + sigma2 / w_i) as a device tensor (n,); data = (Xnew, Ynew).
        Nothing of size n is copied to the host."""
        X, Y, w = self._heldout(data, weights, "predict_log_density_device")
        return self._heldout_moments(X, Y, w)[3]

    def _score_device(self, X, Y, w):
        """[#{w > 0}, sum logdens, sum squared error, sum squared error / s2] over the rows with w > 0: device, 4 doubles"""
        _, s2, sq, ld = self._heldout_moments(X, Y, w)
        if w is None:
            return torch.stack([torch.tensor(float(X.shape[0]), dtype=torch.float64, device=ld.device), ld.sum(), sq.sum(), (sq / s2.reshape(-1)).sum()])
        pos = w > 0
        zero = torch.zeros((), dtype=torch.float64, device=ld.device)
        return torch.stack([pos.sum().to(torch.float64), torch.where(pos, ld, zero).sum(), torch.where(pos, sq, zero).sum(),
                            torch.where(pos, sq / s2.reshape(-1), zero).sum()])

    def score(self, data, weights=None):
        """Scores of held-out rows data = (Xnew, Ynew) as Python floats: n = #{w_i > 0}, log_density = sum_i log p(y_i), sq_err =
        sum_i sum_d (y_id - mean_id)^2, chi2 = sum_i sum_d (y_id - mean_id)^2 / (var_i + sigma2 / w_i) (expectation n D), and the derived
        nlpd = -log_density / n, rmse = sqrt(sq_err / (n D)), mean_chi2 = chi2 / (n D) (NaN for n = 0).  Rows with weight 0 are left out.
        Everything of size n stays on the device.  On a sharded model each rank scores the rows it is given against the global posterior
        and the four sums are all-reduced with SUM, so every rank returns the global scores."""
        X, Y, w = self._heldout(data, weights, "score")
        return self._score_floats(X, Y, w)

    def _score_floats(self, X, Y, w):
        sc = self._score_device(X, Y, w)
        if self._is_sharded():
            sc = sc.clone()
            dist.all_reduce(sc, op=dist.ReduceOp.SUM, group=self._pg)
        n, ld, sq, chi = sc.tolist()
        return _score_dict(n, ld, sq, chi, self.y.shape[1])

    # -- changing the weights in place, and K-fold cross-validation (GPR_1d, and GPR_kron with d = 2) -----------------------
    def _weights_unsupported(self, what):
        raise NotImplementedError("%s.%s: per-observation weights exist for GPR_1d and for GPR_kron with d = 2 only"
                                  % (type(self).__name__, what))

    def set_weights(self, weights):
        self._weights_unsupported("set_weights")

    def kfold_scores(self, folds, refit=False, maxiter=None):
        self._weights_unsupported("kfold_scores")

    def _set_weights_checked(self, weights):
        """set_weights of the models that have a weighted Phi pass: validate like the constructor, copy into the existing weights tensor,
        re-run the weighted pass over this rank's rows (+ the usual all-reduce), refresh the counts, drop the theta-keyed caches."""
        name = type(self).__name__
        if self.weights is None:
            raise ValueError("%s.set_weights: this model was built without weights (pass weights= to the constructor)" % name)
        w = _prepare_weights(weights, self.X.shape[0], self._stats.device, "%s.set_weights" % name)
        self._apply_weights(w)

    def _kfold_state(self):
        """what kfold_scores changes, cloned: restored by copy, because the weighted Phi pass accumulates with atomics"""
        return dict(stats=self._stats.clone(), weights=self.weights.clone(), wstats=self._wstats.clone(),
                    sums=(self.num_data, self.weight_sum, self.log_weight_sum))

    def _kfold_restore(self, st):
        self._stats.copy_(st["stats"])
        self._wstats.copy_(st["wstats"])
        self._restore_weights(st["weights"])
        self.num_data, self.weight_sum, self.log_weight_sum = st["sums"]
        h = getattr(self, "_h", None)
        if h is not None:
            h.set_weight_sums(self.num_data, self.weight_sum, self.log_weight_sum)
        self._drop_theta_caches()

    def _kfold_scores(self, folds, refit, maxiter):
        name = "%s.kfold_scores" % type(self).__name__
        dev = self._stats.device
        fold, counts = _prepare_folds(folds, self.X.shape[0], self.weights, dev, name)
        if self._is_sharded():                                  # K and the per-fold counts are global
            K = torch.tensor([counts.numel()], dtype=torch.int64, device=dev)
            dist.all_reduce(K, op=dist.ReduceOp.MAX, group=self._pg)
            full = torch.zeros(int(K.item()), dtype=torch.int64, device=dev)
            full[:counts.numel()] = counts
            dist.all_reduce(full, op=dist.ReduceOp.SUM, group=self._pg)
            counts = full
        _require_folds_populated(counts, name)
        K = counts.numel()
        twin = self._weighted_twin() if self.weights is None else None
        m = self if twin is None else twin
        params = self.trainable_parameters
        theta0 = [(p._u, p._value) for p in params]

        def reset_theta():
            for p, (u, v) in zip(params, theta0):
                p._u, p._value = u, v

        state = m._kfold_state()
        w0, zero = state["weights"], torch.zeros((), dtype=torch.float64, device=dev)
        out = []
        try:
            for f in range(K):
                inside = fold == f
                m._apply_weights(torch.where(inside, zero, w0))
                if refit:
                    reset_theta()
                    m.fit(**({} if maxiter is None else {"maxiter": maxiter}))
                    m._drop_theta_caches()
                sc = m._score_floats(m.X, m.y, torch.where(inside, w0, zero))
                if refit:
                    sc["theta"] = m.theta()
                out.append(sc)
        finally:
            reset_theta()
            m._kfold_restore(state)
            if twin is not None:
                twin.close()
        n, ld, sq, chi = (sum(s[k] for s in out) for k in ("n", "log_density", "sq_err", "chi2"))
        return dict(folds=out, total=_score_dict(n, ld, sq, chi, self.y.shape[1]))

    # -- gradient of the bound in the weights, learned noise scales per group (GPR_1d, and GPR_kron with d = 2) -----------------
    def weight_gradient_device(self):
        self._weights_unsupported("weight_gradient_device")

    def noise_group_gradient(self, groups):
        self._weights_unsupported("noise_group_gradient")

    def fit_noise_groups(self, groups, maxiter=200, pinned=0):
        self._weights_unsupported("fit_noise_groups")

    def _bound_and_grad(self):
        """(bound as a float, its gradient in trainable_parameters as numpy): the model's analytic elbo_and_grad*"""
        raise NotImplementedError

    def _global_groups(self, groups, what):
        """validated labels of this rank's rows and G = max + 1 (global on a sharded model)"""
        labels, G = _prepare_groups(groups, self.X.shape[0], self._stats.device, what)
        if self._is_sharded():
            Gt = torch.tensor([G], dtype=torch.int64, device=labels.device)
            dist.all_reduce(Gt, op=dist.ReduceOp.MAX, group=self._pg)
            G = int(Gt.item())
        if G < 1:
            raise ValueError("%s: no rows, no groups" % what)
        return labels, G

    def _group_sums_local(self, labels, G):
        """[n_g, T_g] (G, 2) over this rank's rows, device: index_add_ on the per-row gradient"""
        gr = self.weight_gradient_device()
        w = torch.ones_like(gr) if self.weights is None else self.weights
        out = torch.zeros((G, 2), dtype=torch.float64, device=gr.device)
        out[:, 0].index_add_(0, labels, (w > 0).to(torch.float64))
        out[:, 1].index_add_(0, labels, w * gr)                 # (a row with weight 0 has gradient 0)
        return out

    def _group_sums(self, labels, G):
        """[n_g, T_g] (G, 2) as numpy, global on a sharded model (SUM, as kfold_scores adds its counts)"""
        sums = self._group_sums_local(labels, G)
        if self._is_sharded():
            sums = sums.clone()
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=self._pg)
        return sums.cpu().numpy()

    def _noise_group_gradient(self, groups):
        labels, G = self._global_groups(groups, "%s.noise_group_gradient" % type(self).__name__)
        sums = self._group_sums(labels, G)
        return dict(n=np.rint(sums[:, 0]).astype(np.int64), grad_log_weight=sums[:, 1].copy())

    def _fit_noise_groups(self, groups, maxiter, pinned):
        from scipy.optimize import minimize
        name = "%s.fit_noise_groups" % type(self).__name__
        if self.weights is None:
            raise ValueError("%s: this model was built without weights (pass weights= to the constructor)" % name)
        labels, G = self._global_groups(groups, name)
        pinned = int(pinned)
        if not 0 <= pinned < G:
            raise ValueError("%s: pinned = %d is not one of the %d groups" % (name, pinned, G))
        dev = self._stats.device
        params = self.trainable_parameters
        theta0 = [(p._u, p._value) for p in params]
        nth = len(params)
        free = np.array([g for g in range(G) if g != pinned], dtype=np.int64)
        state = self._kfold_state()
        w0 = state["weights"]

        def log_rho(u):
            lr = np.zeros(G)
            lr[free] = u[nth:]
            return lr

        def apply(u):
            """theta and the weights w0_i / rho_{g_i} of the point u"""
            for p, ui in zip(params, u[:nth]):
                p.unconstrained = float(ui)
            rho = torch.as_tensor(np.exp(log_rho(u)), dtype=torch.float64, device=dev)
            self._apply_weights(w0 / rho[labels])

        def fun(u):
            apply(u)
            try:
                e, g = self._bound_and_grad()
            except NotPositiveDefiniteError:
                return np.inf, np.zeros(len(u))
            if not np.isfinite(e):
                return np.inf, np.zeros(len(u))
            T = self._group_sums(labels, G)[:, 1]               # d bound / d log rho_g = -T_g
            grad = np.concatenate([np.asarray(g) * np.array([p.dtheta_du() for p in params]), -T[free]])
            return -e, -grad

        try:
            u0 = np.concatenate([np.array([p.unconstrained for p in params]), np.zeros(G - 1)])
            res = minimize(fun, u0, jac=True, method="L-BFGS-B", options=dict(maxiter=maxiter))
            apply(res.x)
        except BaseException:
            for p, (u, v) in zip(params, theta0):
                p._u, p._value = u, v
            self._kfold_restore(state)
            raise
        self.noise_scales = np.exp(log_rho(res.x))
        return res

    def close(self):
        """Release the model's library handle now (pinned table ring, result mirror, plan) instead of at garbage collection."""
        h = getattr(self, "_h", None)
        if h is not None:
            h.close()
        self._mirror = None                    # (the pinned mirror is gone with the handle: nothing may read through a stale view)
        self.__dict__.pop("_host_call", None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class GPR_1d(_GPModelSurface, _ShardedStats):
    def __init__(self, data, kernel, basis, process_group=None, distributed=None, *, weights=None):
        # Check inputs (gpr.py:22-26)
        assert isinstance(kernel, (kernels.Matern12, kernels.Matern32, kernels.Matern52))
        assert data[0].shape[1] == 1
        dev = basis.device
        self.X, self.y = _to_device(data[0], dev), _to_device(data[1], dev)
        if self.y.dim() == 1:
            self.y = self.y.reshape(-1, 1)
        require_cuda(self.X, self.y)
        _require_inside(self.X, basis.a, basis.b, True, "GPR_1d")
        if weights is not None:               # observation i has noise variance sigma2 / w_i; w_i = 0: the row is absent
            self.weights = _prepare_weights(weights, self.X.shape[0], dev, "GPR_1d")
        # Init model (gpr.py:29-34)
        self.kernel = kernel
        self.likelihood = kernels.Gaussian()
        self.basis = basis
        self.inducing_features = SplineFeatures1D(kernel, basis)
        self.bandwidth = self.basis.order  # gpr.py:37
        self.num_data_local = self.X.shape[0]
        self.D = self.y.shape[1]
        k, M, D = self.bandwidth, basis.m, self.D
        # Precompute static quantities (gpr.py:39-44): one fused Phi pass
        lib = get_lib()
        self._h = Handle()                    # library state of THIS model (asvgp_create)
        self._planned_kind = None
        self._stats = torch.empty((k + 1) * M + M * D + 1, dtype=torch.float64, device=dev)
        wsb = lib.asvgp_phi_workspace_bytes(M, k, D) if self.weights is None else lib.asvgp_phi_weighted_workspace_bytes(M, k, D)
        self._phi_ws = torch.empty(wsb // 8, dtype=torch.float64, device=dev)
        self._wsb = wsb
        self._setup_dist(process_group, distributed)
        if self.weights is not None:
            self._wstats = torch.zeros(3, dtype=torch.float64, device=dev)
        self._phi_pass_local()
        if self.weights is None:
            self.num_data = allreduce_stats(self._stats, self.num_data_local, process_group) if self._distributed \
                else self.num_data_local
        else:                                 # N+ rows count; the fused ELBO launch takes the three scalars from the handle
            self._set_weight_sums(self.num_data_local, self._wstats, process_group)
            self._h.set_weight_sums(self.num_data, self.weight_sum, self.log_weight_sum)
        self.KufKfu = self._stats[:(k + 1) * M].view(k + 1, M)
        self.Kuf_y = self._stats[(k + 1) * M:(k + 1) * M + M * D].view(M, D)
        self.tr_yTy = self._stats[-1]
        self._elbo_ws = torch.zeros(lib.asvgp_elbo_workspace_bytes(M, k, D) // 8, dtype=torch.float64, device=dev)  # zero-init: finalize's arrival slots
        self._out = torch.zeros(8, dtype=torch.float64, device=dev)
        self._info = torch.zeros(2, dtype=torch.int32, device=dev)
        self._post = None
        self._post_loo = None                 # (theta, alpha, W, Pinv_band) of the leave-one-out methods
        self._loo_ws = self._score_ws = None  # workgroup records of asvgp_loo_1d / asvgp_score_1d (allocated on first use)
        self._wgrad_ws = None                 # records or bin rows of asvgp_weight_grad_1d (allocated on first use, grown with G)
        self._post_cov = None                 # (theta, W_dense): the dense P^-1 - Kuu^-1 of predict_f_cov_device
        self._cov_ws = None
        self._host_result = np.zeros(10)      # [out[0..7], info[0], info[1]] of the last host-read evaluation
        self._mirror_read = lib.asvgp_result_mirror_read
        self._publish = lib.asvgp_elbo_publish_theta

    # ------------------------------------------------------------------------------------------------------
    def _phi_pass_local(self):
        """asvgp_phi_accumulate_1d over this rank's rows -> packed [band | Phi y | y^T y] (local sums)."""
        b = self.basis
        if self.weights is not None:
            check(get_lib().asvgp_phi_accumulate_1d_weighted(self._h.ptr, self.X.data_ptr(), self.y.data_ptr(), self.weights.data_ptr(),
                                                             self.X.shape[0], self.D, b.mesh.data_ptr(), b.mesh.shape[0], b.delta_np,
                                                             b.order, b.m, self._stats.data_ptr(), self._wstats.data_ptr(),
                                                             self._phi_ws.data_ptr(), self._wsb, stream_ptr()), "phi_accumulate_1d_weighted")
            return self._stats
        check(get_lib().asvgp_phi_accumulate_1d(self._h.ptr, self.X.data_ptr(), self.y.data_ptr(), self.X.shape[0], self.D,
                                                b.mesh.data_ptr(), b.mesh.shape[0], b.delta_np, b.order, b.m,
                                                self._stats.data_ptr(), self._phi_ws.data_ptr(), self._wsb,
                                                stream_ptr()), "phi_accumulate_1d")
        return self._stats

    @property
    def KufKfu_sparse(self):
        """gpr.py:42: Kuf @ Kuf.T as a sparse M x M matrix (here: symmetric torch sparse COO rebuilt from the band)."""
        low = utils.band_to_sparse(self.KufKfu)
        strict = utils.band_to_sparse(torch.cat([torch.zeros_like(self.KufKfu[:1]), self.KufKfu[1:]], 0))
        return (low + strict.t()).coalesce()

    def theta(self):
        return float(self.kernel.variance), float(self.kernel.lengthscales), float(self.likelihood.variance)

    def _statics(self):
        """Device stack of the static bands of this kernel; on first use (and when the kernel kind changes) the handle plans
        the prior chain from a host copy (asvgp_prior_plan_1d)."""
        kind = self.kernel.kind
        S = self.inducing_features.static_stack(kind)
        if self._planned_kind != kind:
            self._h.prior_plan(np.ascontiguousarray(S.cpu().numpy()), S.shape[0], self.basis.m, self.bandwidth)
            self._planned_kind = kind
        return S

    def phi_reduce(self):
        """With self._h.set_phi_deferred_reduce(1): enqueue the cross-workgroup reduce of the last phi_pass() on the CURRENT stream
        (the caller orders it behind that Phi pass); a no-op otherwise."""
        check(get_lib().asvgp_phi_reduce_1d(self._h.ptr, stream_ptr()), "phi_reduce_1d")
        return self._stats

    def _launch_elbo(self, theta=None):
        v, l, s = self.theta() if theta is None else theta
        S = self._statics()
        c = self.__dict__.get("_elbo_call")
        if c is None or c[0] is not S or c[1] is not self._stats:       # (device pointers of this model's buffers, looked up once)
            c = self._elbo_call = (S, self._stats, get_lib().asvgp_elbo_grad_1d, self._h.ptr, self._stats.data_ptr(), S.data_ptr(),
                                   self.basis.m, self.bandwidth, self.D, self._out.data_ptr(), self._info.data_ptr(),
                                   self._elbo_ws.data_ptr(), self._elbo_ws.numel() * 8)
        rc = c[2](c[3], c[4], c[5], self.kernel.kind, v, l, s, self.num_data, c[6], c[7], c[8], c[9], c[10], c[11], c[12], stream_ptr())
        if rc:
            check(rc, "elbo_grad_1d")
        return self._out

    # -- the same computation split for scheduling (asvgp_elbo_prior_chain_1d / asvgp_elbo_data_chain_1d) ------------
    def launch_prior_chain(self):
        """Enqueue the theta-only half (Kuu, its l-tangent, band(Kuu^-1), log|Kuu|) on the CURRENT stream.  It does not
        read the statistics, so it may run on a side stream while the Phi pass / all-reduce are in flight."""
        v, l, s = self.theta()
        S = self._statics()
        check(get_lib().asvgp_elbo_prior_chain_1d(self._h.ptr, S.data_ptr(), self.kernel.kind, v, l, s, self.basis.m, self.bandwidth,
                                                  self.D, self._info.data_ptr(), self._elbo_ws.data_ptr(),
                                                  self._elbo_ws.numel() * 8, stream_ptr()), "elbo_prior_chain_1d")

    def launch_data_chain(self):
        """Enqueue the data half (P chain + finalize) on the current stream; it must be ordered after launch_prior_chain
        for the same theta (same stream, or current_stream().wait_event(...))."""
        v, l, s = self.theta()
        S = self._statics()
        check(get_lib().asvgp_elbo_data_chain_1d(self._h.ptr, self._stats.data_ptr(), S.data_ptr(), self.kernel.kind, v, l, s,
                                                 self.num_data, self.basis.m, self.bandwidth, self.D, self._out.data_ptr(),
                                                 self._info.data_ptr(), self._elbo_ws.data_ptr(),
                                                 self._elbo_ws.numel() * 8, stream_ptr()), "elbo_data_chain_1d")
        return self._out

    def _check_pd(self, relaunch=None, _retry=2):
        self._h.publish_forward()
        info = self._info.tolist()
        if info[0] < 0 or info[1] < 0:
            # The fused launch gave up waiting (a workgroup of it never became resident next to other work on the device, or its table
            # never arrived).  Its results are discarded; the arrival slots of the workspace are half-armed, so the workspace is zero-filled
            # again and the SAME step is re-issued: first as it was, once the device is idle (the cause is transient co-residency, and the
            # fused launch is the accurate path - band algorithm 1 is 1e-8 of the bound away at the headline's conditioning); if that gives
            # up as well, through the multi-launch sweeps (band algorithm 1: no cross-workgroup waits).
            self.fused_launch_fallbacks = getattr(self, "fused_launch_fallbacks", 0) + 1
            torch.cuda.current_stream().synchronize()
            self._elbo_ws.zero_()
            self._info.zero_()
            if not _retry or relaunch is None:
                raise AsvgpError("the fused launch gave up waiting for its helper workgroups (they never became resident): results discarded")
            if _retry >= 2:
                relaunch()
                return self._check_pd(relaunch, _retry=1)
            previous = self._h.band_algorithm
            self._h.set_band_algorithm(1)
            try:
                relaunch()
            finally:
                self._h.set_band_algorithm(previous)   # (the handle's own setting, not the process default: ADVICE r3)
            return self._check_pd(_retry=0)
        if info[0]:
            raise NotPositiveDefiniteError("Kuu band not positive definite at column %d" % (info[0] - 1))
        if info[1]:
            raise NotPositiveDefiniteError("P = Kuu + KufKfu/sigma2 not positive definite at column %d" % (info[1] - 1))

    def elbo(self, check_pd=True):
        """Variational bound on the log marginal likelihood (gpr.py:49-89); 0-d device tensor."""
        out = self._launch_elbo()
        if check_pd:
            self._check_pd(self._launch_elbo)
        return out[0].clone()

    def maximum_log_likelihood_objective(self):
        return self.elbo()  # gpr.py:46-47 (reduce_sum of a scalar)

    def training_loss(self):
        """gpflow InternalDataTrainingLossMixin: -(objective + log_prior); no priors on this path."""
        return -self.elbo()

    def elbo_and_grad(self, check_pd=True):
        """(elbo, d elbo / d (variance, lengthscale, noise variance)) as a 4-vector device tensor [e, dv, dl, ds]."""
        out = self._launch_elbo()
        if check_pd:
            self._check_pd(self._launch_elbo)
        return out[:4].clone()

    def launch_elbo_host(self, theta=None):
        """First half of elbo_and_grad_host(): enqueue the ELBO + gradient launch on the current stream with the handle's result mirror
        armed; returns the token read_elbo_host() takes.  (Split so that a caller can enqueue other work - the next Phi pass - before it
        starts polling.)  theta = (variance, lengthscale, noise variance) evaluates at these values without touching the model's parameters
        (an optimiser's trial point)."""
        if getattr(self, "_mirror", None) is None:
            self._mirror = self._h.result_mirror(True)
        self._launch_elbo(theta)
        return self._h.result_mirror_pending()

    def launch_elbo_ahead(self):
        """Launch-ahead (asvgp_elbo_grad_ahead_1d): enqueue the NEXT evaluation's ELBO + gradient launch on the current stream BEFORE its
        theta exists; the kernel becomes resident and waits for publish_theta().  Returns the token read_elbo_host() takes, or None when
        the matrix-core launch does not apply to this model (nothing is launched then: use launch_elbo_host)."""
        S = self._statics()
        if getattr(self, "_mirror", None) is None:
            self._mirror = self._h.result_mirror(True)
        rc = get_lib().asvgp_elbo_grad_ahead_1d(self._h.ptr, self._stats.data_ptr(), S.data_ptr(), self.kernel.kind, self.num_data, self.basis.m,
                                                self.bandwidth, self.D, self._out.data_ptr(), self._info.data_ptr(), self._elbo_ws.data_ptr(),
                                                self._elbo_ws.numel() * 8, stream_ptr())
        if rc == -2:                               # ASVGP_ERR_UNSUPPORTED
            return None
        check(rc, "elbo_grad_ahead_1d")
        return self._h.result_mirror_pending()

    def publish_theta(self, theta=None):
        """Second half of launch_elbo_ahead(): hand the waiting launch its (variance, lengthscale, noise variance) - the model's own when
        theta is None - and run the host forward pass of the prior chain for it."""
        v, l, s = self.theta() if theta is None else theta
        check(self._publish(self._h.ptr, v, l, s), "elbo_publish_theta")

    def read_elbo_host(self, token, check_pd=True, poll_seconds=0.05):
        """Second half: [e, dv, dl, ds] as Python floats.  token != 0: the launch writes the pinned mirror - asvgp_result_mirror_read polls
        it from C (no device-to-host copy, no stream synchronisation) and accepts the values only with the launch-bound checksum;
        otherwise, or when nothing arrives within poll_seconds (a launch that gave up waiting never writes the mirror), read through the
        stream (and through _check_pd's re-issue)."""
        r = self._host_result
        if token and self._mirror_read(self._h.ptr, token, r.ctypes.data, poll_seconds) == 0:
            if (r[8] == 0.0 and r[9] == 0.0) or not check_pd:
                return r[:4].tolist()
        else:
            self._h.publish_forward()          # (deferred-forward-pass mode: the launch must not be left waiting for its table; else a no-op)
        if check_pd:
            self._check_pd(self._launch_elbo)
        return self._out[:4].tolist()

    def elbo_and_grad_host(self, check_pd=True, poll_seconds=0.05):
        """elbo_and_grad() for a host that needs the four numbers NOW (an optimiser step: example.py:31-32); a list [e, dv, dl, ds].
        ONE library call: asvgp_elbo_grad_host_1d launches with the result mirror armed and polls it from C."""
        v, l, s = self.theta()
        S = self._statics()
        c = self.__dict__.get("_host_call")
        if c is None or c[0] is not S or c[1] is not self._stats:
            if getattr(self, "_mirror", None) is None:
                self._mirror = self._h.result_mirror(True)
            c = self._host_call = (S, self._stats, get_lib().asvgp_elbo_grad_host_1d, self._h.ptr, self._stats.data_ptr(), S.data_ptr(),
                                   self.basis.m, self.bandwidth, self.D, self._out.data_ptr(), self._info.data_ptr(),
                                   self._elbo_ws.data_ptr(), self._elbo_ws.numel() * 8, self._host_result.ctypes.data)
        rc = c[2](c[3], c[4], c[5], self.kernel.kind, v, l, s, self.num_data, c[6], c[7], c[8], c[9], c[10], c[11], c[12], stream_ptr(),
                  c[13], poll_seconds)
        r = self._host_result
        if rc == 0 and ((r[8] == 0.0 and r[9] == 0.0) or not check_pd):
            return r[:4].tolist()
        if rc not in (0, 1):
            check(rc, "elbo_grad_host_1d")
        if check_pd:
            self._check_pd(self._launch_elbo)
        return self._out[:4].tolist()

    # -- optimiser (example.py:28-33: gpflow.optimizers.Scipy = scipy L-BFGS-B on unconstrained variables) ---
    @property
    def trainable_parameters(self):
        return [self.kernel.variance, self.kernel.lengthscales, self.likelihood.variance]

    def fit(self, maxiter=15000):
        from scipy.optimize import minimize
        params = self.trainable_parameters

        def fun(u):
            for p, ui in zip(params, u):
                p.unconstrained = float(ui)
            try:
                r = self.elbo_and_grad_host()
            except NotPositiveDefiniteError:
                return np.inf, np.zeros(3)
            g = np.array(r[1:4]) * np.array([p.dtheta_du() for p in params])
            return -r[0], -g

        u0 = np.array([p.unconstrained for p in params])
        res = minimize(fun, u0, jac=True, method="L-BFGS-B", options=dict(maxiter=maxiter))
        for p, ui in zip(params, res.x):
            p.unconstrained = float(ui)
        return res

    # -- posterior (gpr.py:91-136) -------------------------------------------------------------------------
    def _posterior(self):
        v, l, s = self.theta()
        key = (v, l, s)
        if self._post is not None and self._post[0] == key:
            return self._post[1], self._post[2]
        b = self.basis
        k, M, D = self.bandwidth, b.m, self.D
        alpha = torch.empty((M, D), dtype=torch.float64, device=self._stats.device)
        W = torch.empty((k + 1, M), dtype=torch.float64, device=self._stats.device)
        S = self._statics()
        check(get_lib().asvgp_posterior_prepare_1d(self._h.ptr, self._stats.data_ptr(), S.data_ptr(), self.kernel.kind, v, l, s, M, k,
                                                   D, alpha.data_ptr(), W.data_ptr(), self._info.data_ptr(),
                                                   self._elbo_ws.data_ptr(), self._elbo_ws.numel() * 8, stream_ptr()),
              "posterior_prepare_1d")
        self._check_pd()
        self._post = (key, alpha, W)
        return alpha, W

    def predict_f_device(self, Xnew):
        """Posterior mean (n, D) and variance (n, 1) as device tensors - one streaming kernel (8 B in, 16 B out)."""
        alpha, W = self._posterior()
        b = self.basis
        x = _to_device(Xnew, self._stats.device).reshape(-1)
        n = x.shape[0]
        mean = torch.empty((n, self.D), dtype=torch.float64, device=x.device)
        var = torch.empty((n, 1), dtype=torch.float64, device=x.device)
        check(get_lib().asvgp_predict_1d_h(self._h.ptr, x.data_ptr(), n, b.mesh.data_ptr(), b.mesh.shape[0], b.delta_np, b.order, b.m,
                                           alpha.data_ptr(), W.data_ptr(), float(self.kernel.variance), self.D,
                                           mean.data_ptr(), var.data_ptr(), stream_ptr()), "predict_1d")
        return mean, var

    # -- leave-one-out predictions in closed form (not in the reference) ------------------------------------------------------
    def _posterior_loo(self):
        """asvgp_posterior_prepare_loo_1d once per theta: (alpha, W, Pinv_band), cached beside _post (whose alpha and W these are, bit for
        bit); Pinv_band = band(P^-1) as the P chain leaves it."""
        v, l, s = self.theta()
        key = (v, l, s)
        if self._post_loo is not None and self._post_loo[0] == key:
            return self._post_loo[1:]
        b = self.basis
        k, M, D = self.bandwidth, b.m, self.D
        dev = self._stats.device
        alpha = torch.empty((M, D), dtype=torch.float64, device=dev)
        W = torch.empty((k + 1, M), dtype=torch.float64, device=dev)
        Pinv = torch.empty((k + 1, M), dtype=torch.float64, device=dev)
        S = self._statics()
        check(get_lib().asvgp_posterior_prepare_loo_1d(self._h.ptr, self._stats.data_ptr(), S.data_ptr(), self.kernel.kind, v, l, s, M, k,
                                                       D, alpha.data_ptr(), W.data_ptr(), Pinv.data_ptr(), self._info.data_ptr(),
                                                       self._elbo_ws.data_ptr(), self._elbo_ws.numel() * 8, stream_ptr()),
              "posterior_prepare_loo_1d")
        self._check_pd()
        self._post_loo = (key, alpha, W, Pinv)
        return alpha, W, Pinv

    def _row_scores(self, entry, X, Y, w, tables, want_mean, want_var, want_logdens, want_scores):
        """asvgp_loo_1d / asvgp_score_1d (entry = "loo" / "score") over the n rows X, Y, w against the posterior tables (alpha, W and, for
        "loo", Pinv_band): (mean (n, D), var (n, 1), logdens (n,), scores (4,)), None where not asked for.  (Plain statements on
        purpose: this runs on the host ahead of a kernel of 0.1 ms, where a generic loop over the outputs shows in the probes.)"""
        b = self.basis
        lib = get_lib()
        dev = self._stats.device
        n = X.shape[0]
        ws = getattr(self, "_%s_ws" % entry)      # workgroup records, allocated on first use; one per entry point: their streams may differ
        if ws is None:
            ws = torch.empty(getattr(lib, "asvgp_%s_workspace_bytes" % entry)(b.m, b.order, self.D) // 8, dtype=torch.float64, device=dev)
            setattr(self, "_%s_ws" % entry, ws)
        mean = torch.empty((n, self.D), dtype=torch.float64, device=dev) if want_mean else None
        var = torch.empty((n, 1), dtype=torch.float64, device=dev) if want_var else None
        ld = torch.empty(n, dtype=torch.float64, device=dev) if want_logdens else None
        sc = torch.empty(4, dtype=torch.float64, device=dev) if want_scores else None
        ptr = lambda t: None if t is None else t.data_ptr()
        check(getattr(lib, "asvgp_%s_1d" % entry)(self._h.ptr, X.data_ptr(), Y.data_ptr(), ptr(w), n, self.D, b.mesh.data_ptr(), b.mesh.shape[0],
                                                  b.delta_np, b.order, b.m, *[t.data_ptr() for t in tables], float(self.kernel.variance),
                                                  float(self.likelihood.variance), ptr(mean), ptr(var), ptr(ld), ptr(sc), ws.data_ptr(),
                                                  ws.numel() * 8, stream_ptr()), entry + "_1d")
        return mean, var, ld, sc

    def _loo(self, want_mean=False, want_var=False, want_logdens=False, want_scores=False):
        """asvgp_loo_1d over this rank's rows: (mean (N, D), var (N, 1), logdens (N,), scores (4,)), None where not asked for."""
        return self._row_scores("loo", self.X, self.y, self.weights, self._posterior_loo(), want_mean, want_var, want_logdens, want_scores)

    def loo_predict_f_device(self):
        """Mean (N, D) and variance (N, 1) of f(x_i) given every training row but i, for all rows of this model (this rank's rows of a
        sharded one), as device tensors: one streaming kernel (asvgp_loo_1d), no refits.  A row with weight 0 is absent from the model
        already: its entries are predict_f_device's."""
        mean, var, _, _ = self._loo(want_mean=True, want_var=True)
        return mean, var

    def loo_log_density_device(self):
        """log p(y_i | y_-i) (N,) as a device tensor, summed over the D outputs the way predict_log_density sums; the left-out
        observation's noise variance is sigma2 / w_i (sigma2 for a row with weight 0)."""
        return self._loo(want_logdens=True)[2]

    def _loo_scores_device(self):
        return self._loo(want_scores=True)[3]               # (nothing of size N is written: 24 B read per row, 16 B unweighted)

    # -- held-out scores in one streaming pass (asvgp_score_1d; not in the reference) ------------------------------------------
    def _score_call(self, X, Y, w, want_logdens=False, want_scores=False):
        """asvgp_score_1d over validated held-out rows: (logdens (n,), scores (4,)), None where not asked for"""
        return self._row_scores("score", X, Y, w, self._posterior(), False, False, want_logdens, want_scores)[2:]

    def predict_log_density_device(self, data, weights=None):
        """sum_d log N(y_id | mean_id, var_f + sigma2 / w_i) as a device tensor (n,), data = (Xnew, Ynew): one streaming kernel
        (asvgp_score_1d; 16 B in per row, 24 B weighted, 8 B out)."""
        X, Y, w = self._heldout(data, weights, "predict_log_density_device")
        return self._score_call(X, Y, w, want_logdens=True)[0]

    def _score_device(self, X, Y, w):
        return self._score_call(X, Y, w, want_scores=True)[1]      # (nothing of size n is written)

    def _drop_theta_caches(self):
        self._post = self._post_loo = self._post_cov = None

    def _restore_weights(self, w):
        self.weights.copy_(w)

    def _apply_weights(self, w):
        """validated weights (device, (N,)) into the existing tensor, then what the constructor does after its Phi pass"""
        self.weights.copy_(w)
        self._phi_pass_local()
        if self._h.deferred and self._distributed:
            check(get_lib().asvgp_phi_reduce_1d(self._h.ptr, stream_ptr()), "phi_reduce_1d")
        self._set_weight_sums(self.num_data_local, self._wstats, self._pg)
        self._h.set_weight_sums(self.num_data, self.weight_sum, self.log_weight_sum)
        self._drop_theta_caches()

    def set_weights(self, weights):
        """Replace the per-observation weights of a model built with weights= (a new mask or fold) without rebuilding it: the handle, the
        workspaces and the buffers stay; one weighted Phi pass over this rank's rows and the usual all-reduce."""
        self._set_weights_checked(weights)

    def _weighted_twin(self):
        """this model with w = 1 through the weighted pass: shares X, y, the basis, the kernel and the likelihood objects"""
        twin = GPR_1d((self.X, self.y), self.kernel, self.basis, process_group=self._pg, distributed=self._distributed,
                      weights=torch.ones(self.X.shape[0], dtype=torch.float64, device=self._stats.device))
        twin.likelihood = self.likelihood
        return twin

    def kfold_scores(self, folds, refit=False, maxiter=None):
        """K-fold cross-validation.  folds: int array (N,) over this rank's rows with values 0..K-1 (K = max + 1, global on a sharded model).
        For every fold f the model is conditioned on the weights w [fold != f] and the rows of the fold are scored with w [fold == f] - at the
        model's current theta, or with refit=True after fit() started from it (the fold's fitted theta is reported as "theta").  Returns
        dict(folds=[score() dict per fold], total=the scores of the summed n, log_density, sq_err, chi2).  On return, normal or by
        exception, the model's weights, statistics, weight sums and theta are the ones it had, bit for bit.  A model built without weights
        runs on an internal weighted twin with w = 1."""
        return self._kfold_scores(folds, refit, maxiter)

    # -- gradient of the bound in the weights (asvgp_weight_grad_1d; not in the reference) --------------------------------------
    GSUM_MAX_GROUPS = 1024                    # asvgp_weight_grad_1d keeps 2 G bins per workgroup in LDS up to this G

    def _weight_grad(self, want_grad, labels32=None, G=None):
        """asvgp_weight_grad_1d over this rank's rows on _posterior_loo()'s tables: (grad (N,) or None, gsum (G, 2) or None (G = None));
        labels32: int32 device labels, or None for the one-group fixed-order sums."""
        b = self.basis
        lib = get_lib()
        dev = self._stats.device
        n = self.X.shape[0]
        tables = self._posterior_loo()
        need = lib.asvgp_weight_grad_workspace_bytes(b.m, b.order, self.D, G or 1) // 8
        if self._wgrad_ws is None or self._wgrad_ws.numel() < need:
            self._wgrad_ws = torch.empty(need, dtype=torch.float64, device=dev)
        ws = self._wgrad_ws
        grad = torch.empty(n, dtype=torch.float64, device=dev) if want_grad else None
        gsum = torch.empty((G, 2), dtype=torch.float64, device=dev) if G else None
        ptr = lambda t: None if t is None else t.data_ptr()
        check(lib.asvgp_weight_grad_1d(self._h.ptr, self.X.data_ptr(), self.y.data_ptr(), ptr(self.weights), n, self.D, b.mesh.data_ptr(),
                                       b.mesh.shape[0], b.delta_np, b.order, b.m, *[t.data_ptr() for t in tables],
                                       float(self.kernel.variance), float(self.likelihood.variance), ptr(labels32), G or 1, ptr(grad),
                                       ptr(gsum), ws.data_ptr(), ws.numel() * 8, stream_ptr()), "weight_grad_1d")
        return grad, gsum

    def weight_gradient_device(self):
        """d ELBO_w / d w_i (N,) over this rank's rows as a device tensor (include/asvgp_hip.h: 1/2 [D / w_i - (D g_i + sum_d r_id^2 +
        var_i - g_i) / sigma2]; 0 for a row with weight 0): one streaming kernel on the leave-one-out tables.  A model built without
        weights is the model with w = 1."""
        return self._weight_grad(True)[0]

    def _group_sums_local(self, labels, G):
        if G > self.GSUM_MAX_GROUPS:
            return super()._group_sums_local(labels, G)
        return self._weight_grad(False, None if G == 1 else labels.to(torch.int32), G)[1]

    def noise_group_gradient(self, groups):
        """groups: int array (N,) over this rank's rows with values >= 0 (G = max + 1, global on a sharded model).  Returns
        dict(n (G,) int64, grad_log_weight (G,)) as numpy: n_g counts the rows of group g with w_i > 0 and grad_log_weight[g] =
        T_g = sum_{i in g} w_i d ELBO_w / d w_i is the derivative of the bound in the log of a common factor on the group's weights - the
        derivative in the log of the group's NOISE scale is -T_g.  Nothing of size N is written up to G = 1024 (the kernel's own bins);
        above that the per-row gradient is summed with index_add_.  On a sharded model the sums are all-reduced with SUM."""
        return self._noise_group_gradient(groups)

    def fit_noise_groups(self, groups, maxiter=200, pinned=0):
        """Fit the relative noise scales of the G groups together with the model's parameters: row i gets the weight w0_i / rho_{g_i} (w0:
        the weights at the call, so its noise variance is sigma2 rho_g / w0_i) and L-BFGS-B maximises the bound in trainable_parameters
        and log rho_g, g != pinned.  rho_pinned = 1: sigma2 carries the common scale, since scaling every weight by c is scaling sigma2
        by 1 / c.  Every evaluation is one weighted Phi pass, the analytic elbo_and_grad and -T_g of noise_group_gradient.  On return the
        model keeps the fitted weights and theta, noise_scales is rho (G,), and the scipy result is returned; on an exception the weights,
        statistics, weight sums and theta are the ones at the call, bit for bit.  A model built without weights= raises ValueError."""
        return self._fit_noise_groups(groups, maxiter, pinned)

    def _bound_and_grad(self):
        r = self.elbo_and_grad_host()
        return r[0], np.array(r[1:4])

    # -- full posterior covariance (not in the reference: its predict_f(full_cov=True) raises, gpr.py:113) ------------
    def _posterior_cov(self):
        """asvgp_posterior_cov_prepare_1d once per theta: W_dense = P^-1 - Kuu^-1 (M x M, device), cached beside _post."""
        v, l, s = self.theta()
        key = (v, l, s)
        if self._post_cov is not None and self._post_cov[0] == key:
            return self._post_cov[1]
        self._post_cov = None
        b = self.basis
        k, M, D = self.bandwidth, b.m, self.D
        lib = get_lib()
        dev = self._stats.device
        if self._cov_ws is None:   # zero-filled once (the chain's arrival slots), like _elbo_ws
            self._cov_ws = torch.zeros(lib.asvgp_posterior_cov_workspace_bytes(M, k, D) // 8, dtype=torch.float64, device=dev)
        alpha = torch.empty((M, D), dtype=torch.float64, device=dev)
        W = torch.empty((k + 1, M), dtype=torch.float64, device=dev)
        Wd = torch.empty((M, M), dtype=torch.float64, device=dev)
        S = self._statics()
        check(lib.asvgp_posterior_cov_prepare_1d(self._h.ptr, self._stats.data_ptr(), S.data_ptr(), self.kernel.kind, v, l, s, M, k, D,
                                                 alpha.data_ptr(), W.data_ptr(), Wd.data_ptr(), self._info.data_ptr(),
                                                 self._cov_ws.data_ptr(), self._cov_ws.numel() * 8, stream_ptr()),
              "posterior_cov_prepare_1d")
        try:
            self._check_pd()
        except AsvgpError:
            self._cov_ws.zero_()
            raise
        self._post_cov = (key, Wd)
        return Wd

    def predict_f_cov_device(self, X1, X2=None):
        """Posterior cross-covariance cov[f(X1), f(X2)] (n1, n2) as a device tensor; X2=None means X1 against itself.
        k(x, x') + phi(x)^T (P^-1 - Kuu^-1) phi(x') in one kernel (asvgp_predict_cov_1d); its diagonal is predict_f's variance."""
        Wd = self._posterior_cov()
        b = self.basis
        x1 = _to_device(X1, self._stats.device).reshape(-1)
        x2 = x1 if X2 is None else _to_device(X2, self._stats.device).reshape(-1)
        n1, n2 = x1.shape[0], x2.shape[0]
        cov = torch.empty((n1, n2), dtype=torch.float64, device=x1.device)
        check(get_lib().asvgp_predict_cov_1d(self._h.ptr, x1.data_ptr(), n1, x2.data_ptr(), n2, b.mesh.data_ptr(), b.mesh.shape[0],
                                             b.delta_np, b.order, b.m, Wd.data_ptr(), self.kernel.kind, float(self.kernel.variance),
                                             float(self.kernel.lengthscales), cov.data_ptr(), n2, stream_ptr()), "predict_cov_1d")
        return cov

    # -- posterior of the derivative f' (not in the reference) ----------------------------------------------------------------
    def predict_f_gradient_device(self, Xnew):
        """Posterior of the slope f'(x): mean (n, D) and variance (n, 1) as device tensors, one streaming kernel (asvgp_predict_deriv_1d):
        mean = phi'^T alpha, var = c v / l^2 + phi'^T W phi' with predict_f's alpha and band W (the same _posterior cache)."""
        _require_derivative(self.kernel, "GPR_1d.predict_f_gradient_device")
        alpha, W = self._posterior()
        b = self.basis
        x = _to_device(Xnew, self._stats.device).reshape(-1)
        n = x.shape[0]
        mean = torch.empty((n, self.D), dtype=torch.float64, device=x.device)
        var = torch.empty((n, 1), dtype=torch.float64, device=x.device)
        check(get_lib().asvgp_predict_deriv_1d(self._h.ptr, x.data_ptr(), n, b.mesh.data_ptr(), b.mesh.shape[0], b.delta_np, b.order, b.m,
                                               alpha.data_ptr(), W.data_ptr(), self.kernel.kind, float(self.kernel.variance),
                                               float(self.kernel.lengthscales), self.D, mean.data_ptr(), var.data_ptr(), stream_ptr()),
              "predict_deriv_1d")
        return mean, var

    def predict_f_gradient(self, Xnew):
        """predict_f_gradient_device as numpy: (mean (n, D), var (n, 1)) of f'(Xnew)."""
        mean, var = self.predict_f_gradient_device(Xnew)
        return mean.cpu().numpy(), var.cpu().numpy()

    def predict_f_gradient_cov_device(self, X1, X2=None, derivs=(1, 1)):
        """cov[f^(p)(X1), f^(q)(X2)] (n1, n2) as a device tensor, (p, q) = derivs in {0, 1}^2; X2=None means X1 against itself.
        d_x^p d_x'^q k(x, x') + phi^(p)(x)^T (P^-1 - Kuu^-1) phi^(q)(x') from predict_f_cov_device's cached W_dense
        (asvgp_predict_cov_deriv_1d); derivs=(0, 0) is predict_f_cov_device."""
        p, q = (int(d) for d in derivs)
        if p not in (0, 1) or q not in (0, 1):
            raise ValueError("GPR_1d.predict_f_gradient_cov_device: derivs must be in {0, 1}^2, got %r" % (tuple(derivs),))
        if p or q:
            _require_derivative(self.kernel, "GPR_1d.predict_f_gradient_cov_device")
        Wd = self._posterior_cov()
        b = self.basis
        x1 = _to_device(X1, self._stats.device).reshape(-1)
        x2 = x1 if X2 is None else _to_device(X2, self._stats.device).reshape(-1)
        n1, n2 = x1.shape[0], x2.shape[0]
        cov = torch.empty((n1, n2), dtype=torch.float64, device=x1.device)
        check(get_lib().asvgp_predict_cov_deriv_1d(self._h.ptr, x1.data_ptr(), n1, x2.data_ptr(), n2, b.mesh.data_ptr(), b.mesh.shape[0],
                                                   b.delta_np, b.order, b.m, Wd.data_ptr(), self.kernel.kind, float(self.kernel.variance),
                                                   float(self.kernel.lengthscales), p, q, cov.data_ptr(), n2, stream_ptr()),
              "predict_cov_deriv_1d")
        return cov

    def predict_f_full_cov(self, Xnew):
        """numpy (mean (n, D), cov (D, n, n)): gpflow's predict_f(full_cov=True) layout.  All D outputs share one covariance, so cov
        is a read-only broadcast of one n x n matrix."""
        mean, _ = self.predict_f_device(Xnew)
        cov = self.predict_f_cov_device(Xnew).cpu().numpy()
        return mean.cpu().numpy(), np.broadcast_to(cov, (self.D,) + cov.shape)

    def predict_f_samples(self, Xnew, num_samples=None, full_cov=True, jitter=1e-6, seed=None):
        """Posterior function samples, numpy (num_samples, n, D), or (n, D) when num_samples is None (gpflow's layout).
        full_cov=True: mean + L z with L = cholesky(cov + jitter I) on the device; full_cov=False: independent draws from the
        marginals of predict_f_device.  seed seeds a device torch.Generator: the same seed gives the same samples."""
        mean, var = self.predict_f_device(Xnew)
        n, D = mean.shape
        S = 1 if num_samples is None else int(num_samples)
        gen = torch.Generator(device=mean.device)
        if seed is None:
            gen.seed()
        else:
            gen.manual_seed(int(seed))
        z = torch.randn((S, n, D), generator=gen, dtype=torch.float64, device=mean.device)
        if full_cov:
            cov = self.predict_f_cov_device(Xnew)
            cov.diagonal().add_(float(jitter))
            L, info = torch.linalg.cholesky_ex(cov)
            if int(info.item()) != 0 or not bool(torch.isfinite(L).all()):
                raise NotPositiveDefiniteError("posterior covariance + jitter * I is not positive definite (jitter = %g%s)"
                                               % (jitter, ", column %d" % (int(info.item()) - 1) if int(info.item()) > 0 else ""))
            f = mean + torch.matmul(L, z)
        else:
            f = mean + var.clamp_min(0.0).sqrt() * z
        f = f.cpu().numpy()
        return f[0] if num_samples is None else f

    def close(self):
        """Also releases the cached dense W and its workspace."""
        self._post_cov = None
        self._post_loo = None
        self._cov_ws = None
        self._loo_ws = self._score_ws = self._wgrad_ws = None
        super().close()

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False, batch=False):
        """gpr.py:91-136.  Returns numpy (mean, var) like the reference.  batch=True reproduces the reference's
        10 000-row chunking including its dropped remainder (rows beyond the last full chunk stay zero, gpr.py:125-136)."""
        assert not full_output_cov
        if full_cov:
            raise NotImplementedError  # gpr.py:113
        if not batch:
            mean, var = self.predict_f_device(Xnew)
            return mean.cpu().numpy(), var.cpu().numpy()
        num_test = Xnew.shape[0]
        mean = np.zeros((num_test, 1))
        var = np.zeros((num_test, 1))
        nfull = int(num_test / 10_000) * 10_000
        if nfull:
            m_, v_ = self.predict_f_device(Xnew[:nfull])
            mean[:nfull] = m_.cpu().numpy()[:, :1]
            var[:nfull] = v_.cpu().numpy()
        return mean, var


class GPR_kron(_GPModelSurface, _ShardedStats):
    """Drop-in for asvgp/gpr.py:239-359: GPR_kron((X[N,d], y[N,1]), kernels, bases) with elbo(),
    maximum_log_likelihood_objective(), training_loss(), predict_f(Xnew).  Never densifies: KufKfu is a block band
    (asvgp_phi_accumulate_kron2d), Kuu = K1 (x) K2 is handled factor-wise (log|Kuu| = m2 log|K1| + m1 log|K2|, the trace
    needs only band(K1^-1) (x) band(K2^-1)), and P = Kuu + KufKfu/sigma2 is a bandwidth k(m2+1) band matrix factorised by a
    blocked band Cholesky - the reference runs dense O(M_tot^3) tf.linalg.cholesky (gpr.py:293).  That is the d = 2 path (every
    reference configuration); any other d takes the reference's own dense route on the device (_init_dense), small grids only."""

    def __init__(self, data, kernels, bases, process_group=None, distributed=None, *, weights=None):
        dev = bases[0].device
        if weights is not None and len(bases) != 2:
            raise NotImplementedError("GPR_kron(weights=...) is implemented for d = 2 (the block-band route) only: the dense and n-d band "
                                      "routes of d = %d have no weighted Phi pass yet" % len(bases))
        # fp32 data (BASELINE configs[3]): the cell-sorted copy the Phi pass streams stays fp32 (12 B per point); X / y themselves are
        # widened once, as the reference does (basis.py:54) - the widening is exact, so the statistics are those of the fp64 data
        self._fp32_storage = (torch.as_tensor(data[0]).dtype == torch.float32 and torch.as_tensor(data[1]).dtype == torch.float32)
        self.X, self.y = _to_device(data[0], dev), _to_device(data[1], dev)
        require_cuda(self.X, self.y)                         # (both routes below hand raw device pointers to the library)
        self.n, self.d = self.X.shape[0], self.X.shape[1]
        assert len(kernels) == len(bases) == self.d          # gpr.py:247
        if weights is not None:                              # observation i has noise variance sigma2 / w_i; w_i = 0: the row is absent
            self.weights = _prepare_weights(weights, self.n, dev, "GPR_kron")
            self._fp32_storage = False                       # (no weighted fp32-storage kernel: weighted fp32 data stream as fp64)
        assert self.y.shape[1] == 1                          # gpr.py:248
        for kern in kernels:
            assert isinstance(kern, (kernels_mod.Matern12, kernels_mod.Matern32, kernels_mod.Matern52))
        assert all(bs.order == bases[0].order for bs in bases)
        self._dense_mode = self.d != 2
        if self._dense_mode:      # d != 2 (no reference config): the reference's own dense route (gpr.py:266-308) on the device
            self._init_dense(kernels, bases, process_group, distributed)
            return
        for i, bs in enumerate(bases):
            _require_inside(self.X[:, i], bs.a, bs.b, False, "GPR_kron dimension %d" % i)
        self.kernels, self.bases = kernels, bases
        self.kernel = kernels[-1]                            # gpr.py:254 passes the leaked loop variable
        self.likelihood = kernels_mod.Gaussian()
        self.m, self.order = bases[0].m, bases[0].order      # gpr.py:260-261
        self.bandwidth = int((self.m ** self.d - 1) * self.order / (self.m - 1))   # gpr.py:262 (as written)
        self.true_bandwidth = self.order * (bases[1].m + 1)
        self.inducing_features = [SplineFeatures1D(kernels[i], bases[i]) for i in range(self.d)]
        lib = get_lib()
        m1, m2, k = bases[0].m, bases[1].m, self.order
        self.Mtot = m1 * m2
        self.noff = k * (2 * k + 1) + k + 1
        self._stats = torch.empty(lib.asvgp_kron_stats_doubles(m1, m2, k), dtype=torch.float64, device=dev)
        self._setup_dist(process_group, distributed)
        if self.weights is not None:
            self._wstats = torch.zeros(3, dtype=torch.float64, device=dev)
        self._phi_pass_local()
        if self.weights is None:
            self.num_data = allreduce_stats(self._stats, self.n, process_group) if self._distributed else self.n
        else:
            self._set_weight_sums(self.n, self._wstats, process_group)
        self.KufKfu_blockband = self._stats[:self.noff * self.Mtot].view(self.noff, self.Mtot)
        self.Kuf_y = self._stats[self.noff * self.Mtot:self.noff * self.Mtot + self.Mtot].view(self.Mtot, 1)
        self.tr_yTy = self._stats[-1]
        self._info = torch.zeros(1, dtype=torch.int32, device=dev)
        self._post = None
        self._post_cov = None                 # (key, Sigma, [K1^-1, K2^-1], the _post it was completed from) of predict_f_cov_device

    # ---- d != 2: dense tensor-product route, as the reference does it for every d (kronecker.py:32-33 folds over any d;
    # gpr.py:266-272 densifies Kuf Kuf^T, 286-308 dense Cholesky).  The statistics are [M_tot^2 dense Kuf Kuf^T | Kuf y | y^T y]
    # (one all-reduce); the Khatri-Rao rows come from the per-dimension HIP evaluate kernels, everything after that is dense
    # device linear algebra through torch.  No reference configuration uses it; sizes are limited by M_tot^2 memory.
    def _init_dense(self, kernels, bases, process_group, distributed):
        for i, bs in enumerate(bases):
            _require_inside(self.X[:, i], bs.a, bs.b, False, "GPR_kron dimension %d" % i)
        self.kernels, self.bases = kernels, bases
        self.kernel = kernels[-1]
        self.likelihood = kernels_mod.Gaussian()
        self.m, self.order = bases[0].m, bases[0].order
        self.bandwidth = int((self.m ** self.d - 1) * self.order / (self.m - 1)) if self.m > 1 else 0   # gpr.py:262 (as written)
        self.inducing_features = [SplineFeatures1D(kernels[i], bases[i]) for i in range(self.d)]
        self.Mtot = 1
        for bs in bases:
            self.Mtot *= bs.m
        if self.Mtot > 8192:
            raise NotImplementedError("GPR_kron with d != 2 takes the dense route: M_tot = %d is too large for it" % self.Mtot)
        dev = self._dev = bases[0].device
        self._stats = torch.zeros(self.Mtot * self.Mtot + self.Mtot + 1, dtype=torch.float64, device=dev)
        self._setup_dist(process_group, distributed)
        self._phi_pass_local()
        self.num_data = allreduce_stats(self._stats, self.n, process_group) if self._distributed else self.n
        self.KufKfu = self._stats[:self.Mtot * self.Mtot].view(self.Mtot, self.Mtot)
        self.Kuf_y = self._stats[self.Mtot * self.Mtot:self.Mtot * self.Mtot + self.Mtot].view(self.Mtot, 1)
        self.tr_yTy = self._stats[-1]
        self._info = torch.zeros(1, dtype=torch.int32, device=dev)
        self._post = None
        self._post_cov = None                 # (key, Sigma, [K1^-1, K2^-1], the _post it was completed from) of predict_f_cov_device

    def _dense_rows(self, X):
        """Khatri-Rao design matrix (M_tot, n) of a chunk of points, dim-0 major (kronecker.py:27-33)."""
        Phi = None
        for i, bs in enumerate(self.bases):
            P = bs.evaluate_basis(X[:, i:i + 1].contiguous(), sparse=False)              # (m_i, n)
            Phi = P if Phi is None else (Phi[:, None, :] * P[None, :, :]).reshape(-1, X.shape[0])
        return Phi

    def _dense_phi_pass(self, chunk=8192):
        M = self.Mtot
        A = torch.zeros((M, M), dtype=torch.float64, device=self._dev)
        b = torch.zeros((M, 1), dtype=torch.float64, device=self._dev)
        for lo in range(0, self.n, chunk):
            Phi = self._dense_rows(self.X[lo:lo + chunk])
            A += Phi @ Phi.t()
            b += Phi @ self.y[lo:lo + chunk]
        self._stats[:M * M] = A.reshape(-1)
        self._stats[M * M:M * M + M] = b.reshape(-1)
        self._stats[-1] = (self.y * self.y).sum()
        self._post = None
        return self._stats

    def _dense_factor(self):
        s = float(self.likelihood.variance)
        Ks, dKs = [], []
        for feat, kern in zip(self.inducing_features, self.kernels):
            K, dK, _, _, _, _ = feat.inverse_band(kern)
            Ks.append(utils.band_to_dense_sym(K)); dKs.append(utils.band_to_dense_sym(dK))
        Kuu = Ks[0]
        for K in Ks[1:]:
            Kuu = torch.kron(Kuu, K)
        LK, info = torch.linalg.cholesky_ex(Kuu)
        if int(info.item()):
            raise NotPositiveDefiniteError("Kuu = kron(K_i) not positive definite at column %d" % (int(info.item()) - 1))
        P = self.KufKfu / s + Kuu
        LP, info = torch.linalg.cholesky_ex(P)
        if int(info.item()):
            raise NotPositiveDefiniteError("P = Kuu + KufKfu/sigma2 not positive definite at column %d" % (int(info.item()) - 1))
        return dict(s=s, Ks=Ks, dKs=dKs, Kuu=Kuu, LK=LK, LP=LP)

    nd_banded = None          # d != 2: None = band route for P when its band fits (bandwidth <= 432, band storage <= 1 GiB); False: dense always

    def _nd_band_layout(self):
        """d != 2: P = kron(K_i) + Kuf Kuf^T / s is a band matrix of bandwidth bw = k (m_2 ... m_d + ... + m_d + 1) (dim-0 major index).
        Cached index arrays of its band slots (column c, offset e -> row r = c + e): the dense index r M + c, the per-dimension band
        lookups of the 1-D factors, the pattern mask (all |i_t(r) - i_t(c)| <= k) and the diagonal / off-diagonal weight."""
        lay = getattr(self, "_nd_lay", None)
        if lay is not None:
            return lay if lay else None
        self._nd_lay = {}
        k, d, M = self.order, self.d, self.Mtot
        ms = [bs.m for bs in self.bases]
        strides = [1] * d
        for t in range(d - 2, -1, -1):
            strides[t] = strides[t + 1] * ms[t + 1]
        bw = k * sum(strides)
        if self.nd_banded is False or d < 2 or bw > 432 or bw >= M or M * (bw + 1) * 8 * (d + 4) > (1 << 30):
            return None
        dev = self._dev
        c = torch.arange(M, device=dev).view(-1, 1)
        e = torch.arange(bw + 1, device=dev).view(1, -1)
        r = c + e
        inb = r < M
        rr = torch.where(inb, r, torch.zeros_like(r))
        pat = inb.clone()
        kidx = []
        for t in range(d):
            it_r = (rr // strides[t]) % ms[t]
            it_c = ((c // strides[t]) % ms[t]).expand_as(rr)
            dt = it_r - it_c
            pat &= dt.abs() <= k
            dd = dt.abs().clamp(max=k)
            kidx.append(dd * ms[t] + torch.minimum(it_r, it_c))     # lower band (k+1, m_t): entry (|d|, min(i, j))
        Bb = ((max(bw, 1) + 31) // 32) * 32
        nblk = (M + Bb - 1) // Bb
        bi, bj = rr // Bb, (c // Bb).expand_as(rr)
        per = Bb * Bb
        sidx = torch.where(bi == bj, bi * per + (rr % Bb) * Bb + (c % Bb), nblk * per + bj * per + (rr % Bb) * Bb + (c % Bb))
        self._nd_lay = dict(bw=bw, Bb=Bb, nblk=nblk, pat=pat, didx=(rr * M + c), kidx=kidx, sidx=torch.where(inb, sidx, torch.zeros_like(sidx)),
                            w=torch.where(e == 0, 1.0, 2.0).to(torch.float64).expand(M, bw + 1), rows=rr, ms=ms)
        return self._nd_lay

    def _nd_band_factor(self, lay):
        """Band Cholesky of P (asvgp_blockband_cholesky, the rhs riding along) instead of the dense O(M_tot^3) factorisations; log|Kuu| and
        tr(Kuu^-1 A) factor-wise from the 1-D chains (band(K_t^-1) is all the trace needs: A has the pattern of the band)."""
        lib = get_lib()
        s = float(self.likelihood.variance)
        M, bw, pat = self.Mtot, lay["bw"], lay["pat"]
        Ks, dKs, Ss, dSs, lds = [], [], [], [], []
        for i, (feat, kern) in enumerate(zip(self.inducing_features, self.kernels)):
            K, dK, S, dS, ld2, info = feat.inverse_band(kern)
            col = int(feat._info[0].item())
            if col:
                raise NotPositiveDefiniteError("Kuu band of dimension %d not positive definite at column %d" % (i, col - 1))
            Ks.append(K.reshape(-1)); dKs.append(dK.reshape(-1)); Ss.append(S.reshape(-1)); dSs.append(dS.reshape(-1)); lds.append(ld2)
        zero = torch.zeros((), dtype=torch.float64, device=self._dev)
        gk = [K[ix] for K, ix in zip(Ks, lay["kidx"])]
        gs = [S[ix] for S, ix in zip(Ss, lay["kidx"])]
        kuu = gk[0]
        sk = gs[0]
        for a, b in zip(gk[1:], gs[1:]):
            kuu = kuu * a
            sk = sk * b
        kuu, sk = torch.where(pat, kuu, zero), torch.where(pat, sk, zero)   # (outside the pattern the clamped lookups mean nothing)
        Ab = torch.where(pat, self.KufKfu.reshape(-1)[lay["didx"]], zero)
        Pb = (kuu + Ab / s).contiguous()
        c = self.Kuf_y.reshape(-1).clone()
        logdet_P = torch.zeros(1, dtype=torch.float64, device=self._dev)
        check(lib.asvgp_blockband_cholesky(Pb.data_ptr(), M, bw, c.data_ptr(), logdet_P.data_ptr(), self._info.data_ptr(), stream_ptr()),
              "blockband_cholesky")
        col = int(self._info.item())
        if col < 0:
            raise AsvgpError("blockband_cholesky gave up waiting for a block column (its workgroup never became resident): results discarded")
        if col:
            raise NotPositiveDefiniteError("P = Kuu + KufKfu/sigma2 not positive definite at column %d" % (col - 1))
        logdet_K = sum((M // m) * ld[0] for m, ld in zip(lay["ms"], lds))
        trace = (lay["w"] * sk * Ab).sum()
        return dict(s=s, Ks=Ks, dKs=dKs, Ss=Ss, dSs=dSs, gk=gk, gs=gs, kuu=kuu, sk=sk, Ab=Ab, Lb=Pb.reshape(-1), bw=bw, c=c / s, cc=((c / s) ** 2).sum(),
                    logdet_P=logdet_P[0], logdet_K=logdet_K, trace=trace, alpha=None)

    def _nd_band_sigma(self, lay, f):
        """band(P^-1) in the slot layout (and alpha) from the super-block selected inverse of the band factor"""
        SigD, SigS, Bb = self._selinv(f)
        flat = torch.cat((SigD.reshape(-1), SigS.reshape(-1)))
        return torch.where(lay["pat"], flat[lay["sidx"]], torch.zeros((), dtype=torch.float64, device=self._dev))

    def _nd_band_elbo_and_grad(self, lay, want_grad=True):
        f = self._nd_band_factor(lay)
        s, N, M = f["s"], float(self.num_data), self.Mtot
        vs = [float(k.variance) for k in self.kernels]
        vprod = float(np.prod(vs))
        yy = self.tr_yTy
        elbo = (-0.5 * N * math.log(2 * math.pi * s) - 0.5 * f["logdet_P"] + 0.5 * f["logdet_K"] - 0.5 * yy / s
                + 0.5 * f["cc"] - 0.5 * N * vprod / s + 0.5 * f["trace"] / s)
        if not want_grad:
            return elbo, None
        from . import banded
        sig = self._nd_band_sigma(lay, f)                           # (also fills f["alpha"])
        w, Ab, alpha = lay["w"], f["Ab"], f["alpha"]
        aa = w * alpha.view(-1, 1) * alpha[lay["rows"]]
        ws = w * sig
        tPA, aAa = (ws * Ab).sum(), (aa * Ab).sum()
        tPK, aKa = (ws * f["kuu"]).sum(), (aa * f["kuu"]).sum()
        tSA = f["trace"]
        cc = f["cc"]
        g = []
        for t in range(self.d):
            xt = f["dKs"][t][lay["kidx"][t]]
            zt = -f["dSs"][t][lay["kidx"][t]]                        # band(K^-1 dK K^-1) = -d band(K^-1)/dl
            for u in range(self.d):
                if u != t:
                    xt = xt * f["gk"][u]
                    zt = zt * f["gs"][u]
            xt = torch.where(lay["pat"], xt, torch.zeros((), dtype=torch.float64, device=self._dev))
            tPX, aXa, tZA = (ws * xt).sum(), (aa * xt).sum(), (w * Ab * zt).sum()
            mt = lay["ms"][t]
            trK = banded.band_trace_sym(f["Ss"][t].view(self.order + 1, mt), f["dKs"][t].view(self.order + 1, mt))
            g.append((0.5 * tPK - 0.5 * M + 0.5 * aKa + 0.5 * tSA / s) / vs[t] - 0.5 * N * vprod / (vs[t] * s))          # d / d v_t
            g.append(-0.5 * tPX + 0.5 * (M // mt) * trK - 0.5 * aXa - 0.5 * tZA / s)                                       # d / d l_t
        s2 = s * s
        g.append(-0.5 * N / s + 0.5 * tPA / s2 - cc / s + 0.5 * aAa / s2 + 0.5 * yy / s2 + 0.5 * N * vprod / s2 - 0.5 * tSA / s2)
        return elbo, torch.stack([torch.as_tensor(x, dtype=torch.float64, device=self._dev).reshape(()) for x in g])

    def _nd_band_predict(self, lay, Xnew, chunk=8192):
        key = self.theta()
        if self._post is None or self._post[0] != key:
            f = self._nd_band_factor(lay)
            sig = self._nd_band_sigma(lay, f)
            M, pat = self.Mtot, lay["pat"]
            rows, cols = lay["rows"][pat], torch.arange(M, device=self._dev).view(-1, 1).expand_as(pat)[pat]
            vals = sig[pat]
            off = rows != cols
            Sp = torch.sparse_coo_tensor(torch.stack((torch.cat((rows, cols[off])), torch.cat((cols, rows[off])))), torch.cat((vals, vals[off])),
                                         (M, M)).coalesce()
            Sd = [utils.band_to_dense_sym(S.view(self.order + 1, m)) for S, m in zip(f["Ss"], lay["ms"])]
            self._post = (key, f["alpha"], Sp, Sd)
        _, alpha, Sp, Sd = self._post
        X = _to_device(Xnew, self._dev)
        vprod = float(np.prod([float(k.variance) for k in self.kernels]))
        means, vars_ = [], []
        for lo in range(0, X.shape[0], chunk):
            Xc = X[lo:lo + chunk]
            Phi = self._dense_rows(Xc)
            means.append(Phi.t() @ alpha.view(-1, 1))
            qp = (Phi * torch.sparse.mm(Sp, Phi)).sum(0)            # phi*^T band(P^-1) phi*: phi* touches band entries only
            qk = None
            for i, bs in enumerate(self.bases):
                Pt = bs.evaluate_basis(Xc[:, i:i + 1].contiguous(), sparse=False)
                q = (Pt * (Sd[i] @ Pt)).sum(0)
                qk = q if qk is None else qk * q
            vars_.append((vprod + qp - qk).reshape(-1, 1))
        return torch.cat(means), torch.cat(vars_)

    def _dense_elbo_and_grad(self, want_grad=True):
        lay = self._nd_band_layout()
        if lay is not None:
            return self._nd_band_elbo_and_grad(lay, want_grad)
        f = self._dense_factor()
        s, N, A, bvec = f["s"], float(self.num_data), self.KufKfu, self.Kuf_y
        vs = [float(k.variance) for k in self.kernels]
        vprod = float(np.prod(vs))
        alpha = torch.cholesky_solve(bvec, f["LP"]) / s
        KinvA = torch.cholesky_solve(A, f["LK"])
        tr = torch.trace(KinvA)
        bTa = (bvec * alpha).sum()
        elbo = (-0.5 * N * math.log(2 * math.pi * s) - torch.log(torch.diagonal(f["LP"])).sum() + torch.log(torch.diagonal(f["LK"])).sum()
                - 0.5 * self.tr_yTy / s + 0.5 * bTa / s - 0.5 * N * vprod / s + 0.5 * tr / s)
        if not want_grad:
            return elbo, None
        Kinv = torch.cholesky_inverse(f["LK"])
        Pinv = torch.cholesky_inverse(f["LP"])
        G = 0.5 * (Kinv - Pinv - alpha @ alpha.t() - KinvA @ Kinv / s)
        g = []
        for i in range(self.d):
            Kd = None
            for j in range(self.d):
                Mj = f["dKs"][j] if j == i else f["Ks"][j]
                Kd = Mj if Kd is None else torch.kron(Kd, Mj)
            g.append((G * (-f["Kuu"] / vs[i])).sum() - 0.5 * N * vprod / (vs[i] * s))
            g.append((G * Kd).sum())
        s2 = s * s
        g.append(-0.5 * N / s + 0.5 * (Pinv * A).sum() / s2 + 0.5 * self.tr_yTy / s2 + 0.5 * (alpha.t() @ A @ alpha).reshape(()) / s2
                 - bTa / s2 + 0.5 * N * vprod / s2 - 0.5 * tr / s2)
        return elbo, torch.stack([x.reshape(()) for x in g])

    def _dense_predict(self, Xnew, chunk=8192):
        lay = self._nd_band_layout()
        if lay is not None:
            return self._nd_band_predict(lay, Xnew, chunk)
        f = self._dense_factor()
        s = f["s"]
        alpha = torch.cholesky_solve(self.Kuf_y, f["LP"]) / s
        X = _to_device(Xnew, self._dev)
        vprod = float(np.prod([float(k.variance) for k in self.kernels]))
        means, vars_ = [], []
        for lo in range(0, X.shape[0], chunk):
            Phi = self._dense_rows(X[lo:lo + chunk])
            means.append(Phi.t() @ alpha)
            tP = torch.linalg.solve_triangular(f["LP"], Phi, upper=False)
            tK = torch.linalg.solve_triangular(f["LK"], Phi, upper=False)
            vars_.append((vprod + (tP * tP).sum(0) - (tK * tK).sum(0)).reshape(-1, 1))     # gpr.py:319-330
        return torch.cat(means), torch.cat(vars_)

    def _sort_by_cell(self):
        """Rows of (X, y) permuted into 2-D cell order + the cell offsets (the data are immutable: sorted once)."""
        lib = get_lib()
        b1, b2 = self.bases
        dev = self._stats.device
        cell = torch.empty(self.n, dtype=torch.int32, device=dev)
        check(lib.asvgp_kron_cell_index(self.X.data_ptr(), self.n, b1.mesh.data_ptr(), b1.mesh.shape[0], b1.delta_np,
                                        b2.mesh.data_ptr(), b2.mesh.shape[0], b2.delta_np, cell.data_ptr(), stream_ptr()),
              "kron_cell_index")
        ncell = (b1.mesh.shape[0] - 1) * (b2.mesh.shape[0] - 1)
        order = torch.argsort(cell, stable=True)                 # (stable: the same data always stream in the same order - reproducible sums)
        counts = torch.bincount(cell, minlength=ncell)
        start = torch.zeros(ncell + 1, dtype=torch.int64, device=dev)
        start[1:] = torch.cumsum(counts, 0)
        Xs, ys = self.X[order].contiguous(), self.y[order].contiguous()
        if self.weights is not None:
            self._sort_perm = order                               # (kept: set_weights regathers the sorted weights, no new argsort)
            return Xs, ys, start, self.weights[order].contiguous()
        if getattr(self, "_fp32_storage", False):
            Xs, ys = Xs.to(torch.float32), ys.to(torch.float32)   # (exact: the data WERE fp32)
        return Xs, ys, start

    def _phi_pass_local(self, sorted_cells=True):
        """The N-dependent pass over this rank's rows -> [block band | Kuf y | y^T y].  Default: cell-sorted accumulation (one atomic per band entry and
        cell); sorted_cells=False: the per-point atomic kernel (asvgp_phi_accumulate_kron2d), same statistics."""
        if self._dense_mode:
            return self._dense_phi_pass()
        b1, b2 = self.bases
        lib = get_lib()
        if self.weights is not None:
            if sorted_cells and self.n > 0:
                if getattr(self, "_sorted", None) is None:
                    self._sorted = self._sort_by_cell()
                Xs, ys, start, ws = self._sorted
                check(lib.asvgp_phi_accumulate_kron2d_sorted_weighted(Xs.data_ptr(), ys.data_ptr(), ws.data_ptr(), self.n, start.data_ptr(),
                                                                      b1.mesh.data_ptr(), b1.mesh.shape[0], b1.delta_np, b1.m,
                                                                      b2.mesh.data_ptr(), b2.mesh.shape[0], b2.delta_np, b2.m, self.order,
                                                                      self._stats.data_ptr(), self._wstats.data_ptr(), stream_ptr()),
                      "phi_accumulate_kron2d_sorted_weighted")
            else:
                check(lib.asvgp_phi_accumulate_kron2d_weighted(self.X.data_ptr(), self.y.data_ptr(), self.weights.data_ptr(), self.n,
                                                               b1.mesh.data_ptr(), b1.mesh.shape[0], b1.delta_np, b1.m, b2.mesh.data_ptr(),
                                                               b2.mesh.shape[0], b2.delta_np, b2.m, self.order, self._stats.data_ptr(),
                                                               self._wstats.data_ptr(), stream_ptr()), "phi_accumulate_kron2d_weighted")
            return self._stats
        if sorted_cells and self.n > 0:
            if getattr(self, "_sorted", None) is None:
                self._sorted = self._sort_by_cell()
            Xs, ys, start = self._sorted
            entry = lib.asvgp_phi_accumulate_kron2d_sorted_f32 if Xs.dtype == torch.float32 else lib.asvgp_phi_accumulate_kron2d_sorted
            check(entry(Xs.data_ptr(), ys.data_ptr(), self.n, start.data_ptr(),
                        b1.mesh.data_ptr(), b1.mesh.shape[0], b1.delta_np, b1.m,
                        b2.mesh.data_ptr(), b2.mesh.shape[0], b2.delta_np, b2.m, self.order,
                        self._stats.data_ptr(), stream_ptr()), "phi_accumulate_kron2d_sorted")
        else:
            check(lib.asvgp_phi_accumulate_kron2d(self.X.data_ptr(), self.y.data_ptr(), self.n, b1.mesh.data_ptr(),
                                                  b1.mesh.shape[0], b1.delta_np, b1.m, b2.mesh.data_ptr(),
                                                  b2.mesh.shape[0], b2.delta_np, b2.m, self.order,
                                                  self._stats.data_ptr(), stream_ptr()), "phi_accumulate_kron2d")
        return self._stats

    @property
    def Kuf(self):
        """gpr.py:269 kron.make_kvs_sparse(Kuf): sparse (m1*m2, N) Khatri-Rao design matrix."""
        from . import kronecker
        return kronecker.make_kvs_sparse(self.bases, self.X)

    # gpr.py:271-273: the three views of Kuf Kuf^T the reference stores as attributes.  Here they are lazy (the model itself works on the
    # block band): built from KufKfu_blockband on first access, never from Kuf @ Kuf.T.
    @property
    def KufKfu_sparse(self):
        """gpr.py:271: symmetric sparse (M_tot, M_tot) Kuf @ Kuf.T (torch sparse COO)."""
        if self._dense_mode:
            return self.KufKfu.to_sparse()
        k, m1, m2 = self.order, self.bases[0].m, self.bases[1].m
        dev = self._stats.device
        offs = [(0, d2) for d2 in range(k + 1)] + [(d1, d2) for d1 in range(1, k + 1) for d2 in range(-k, k + 1)]
        i1 = torch.arange(m1, device=dev).repeat_interleave(m2)
        i2 = torch.arange(m2, device=dev).repeat(m1)
        col = i1 * m2 + i2
        r, c, v = [], [], []
        for o, (d1, d2) in enumerate(offs):
            ok = (i1 + d1 < m1) & (i2 + d2 >= 0) & (i2 + d2 < m2)
            rows, cols, vals = (col + d1 * m2 + d2)[ok], col[ok], self.KufKfu_blockband[o][ok]
            r.append(rows); c.append(cols); v.append(vals)
            if (d1, d2) != (0, 0):
                r.append(cols); c.append(rows); v.append(vals)
        return torch.sparse_coo_tensor(torch.stack([torch.cat(r), torch.cat(c)]), torch.cat(v), (self.Mtot, self.Mtot)).coalesce()

    @property
    def KufKfu_dense(self):
        """gpr.py:272: dense (M_tot, M_tot) Kuf @ Kuf.T."""
        return self.KufKfu if self._dense_mode else self.KufKfu_sparse.to_dense()

    @property
    def KufKfu_band(self):
        """gpr.py:273: utils.sparse_to_band(KufKfu_sparse, self.bandwidth) with the reference's own bandwidth attribute (gpr.py:262)."""
        return utils.sparse_to_band(self.KufKfu_sparse, min(self.bandwidth, self.Mtot - 1))

    def theta(self):
        return [(float(k.variance), float(k.lengthscales)) for k in self.kernels], float(self.likelihood.variance)

    twisted = None            # None: two-sided factorisation when P has >= 6 super-blocks; False / True force it off / on (>= 3 blocks per side)

    def _twist_layout(self):
        """Separator and padding of the two-sided factorisation (asvgp_kron_assemble_twisted), or None for the one-sided band Cholesky."""
        from .kronecker import twisted_layout
        m2, k = self.bases[1].m, self.order
        return twisted_layout(self.Mtot, k * m2 + k, self.twisted)

    def _factor(self, want_alpha):
        """Kuu factors per dimension, trace term, wide-band Cholesky of P with the rhs riding along."""
        from . import banded
        lib = get_lib()
        b1, b2 = self.bases
        m1, m2, k = b1.m, b2.m, self.order
        s = float(self.likelihood.variance)
        # per-dimension Kuu factors: band(K_i^-1), its exact lengthscale tangent and log|K_i| from ONE call each (gpr.py:286-291)
        Ks, dKs, Ss, dSs, lds = [], [], [], [], []
        for feat, kern in zip(self.inducing_features, self.kernels):
            K, dK, S, dS, ld2, info = feat.inverse_band(kern)
            Ks.append(K); dKs.append(dK); Ss.append(S); dSs.append(dS); lds.append(ld2)
        for i, feat in enumerate(self.inducing_features):
            col = int(feat._info[0].item())
            if col:
                raise NotPositiveDefiniteError("Kuu band of dimension %d not positive definite at column %d" % (i, col - 1))
        logdet_K = m2 * lds[0][0] + m1 * lds[1][0]
        bw = k * m2 + k
        dev = self._stats.device
        lay = self._twist_layout()
        if lay is not None:
            return self._factor_twisted(lay, dict(Ks=Ks, dKs=dKs, Ss=Ss, dSs=dSs, logdet_K=logdet_K, s=s, bw=bw))
        Pb = torch.empty(self.Mtot * (bw + 1), dtype=torch.float64, device=dev)
        tr = torch.zeros(1, dtype=torch.float64, device=dev)
        check(lib.asvgp_kron_assemble(Ks[0].data_ptr(), Ks[1].data_ptr(), Ss[0].data_ptr(), Ss[1].data_ptr(),
                                      self.KufKfu_blockband.data_ptr(), k, m1, m2, s, Pb.data_ptr(), tr.data_ptr(),
                                      stream_ptr()), "kron_assemble")
        c = self.Kuf_y.reshape(-1).clone()
        logdet_P = torch.zeros(1, dtype=torch.float64, device=dev)
        check(lib.asvgp_blockband_cholesky(Pb.data_ptr(), self.Mtot, bw, c.data_ptr(), logdet_P.data_ptr(),
                                           self._info.data_ptr(), stream_ptr()), "blockband_cholesky")
        col = int(self._info.item())
        if col < 0:
            raise AsvgpError("blockband_cholesky gave up waiting for a block column (its workgroup never became resident): results discarded")
        if col:
            raise NotPositiveDefiniteError("P = Kuu + KufKfu/sigma2 not positive definite at column %d" % (col - 1))
        alpha = None
        if want_alpha:
            alpha = c.clone()
            check(lib.asvgp_blockband_backsolve(Pb.data_ptr(), self.Mtot, bw, alpha.data_ptr(), stream_ptr()),
                  "blockband_backsolve")
            alpha = alpha / s
        return dict(Ks=Ks, dKs=dKs, Ss=Ss, dSs=dSs, logdet_K=logdet_K, logdet_P=logdet_P[0], trace=tr[0], c=c / s, cc=((c / s) ** 2).sum(),
                    Lb=Pb, bw=bw, alpha=alpha, s=s)

    def _factor_twisted(self, lay, f):
        """Two-sided band Cholesky of P (include/asvgp_hip.h, asvgp_kron_assemble_twisted): the top system and the reversed bottom system
        are factored concurrently on two streams - half the sequential chain each - and meet in the separator's Schur complement
        S = L_ss L_ss^T + J L'_ss L'_ss^T J - P_ss, a dense Bb x Bb block factored last by the same band kernel (bw = Bb - 1).
        log|P| = interior pivots of both + log|S|;  c^T P^-1 c = |y_top|^2 + |y_bottom|^2 + |L_S^-1 r_s|^2 with
        r_s = L_ss y_s + J L'_ss y'_s - c_s (each one-sided sweep has already subtracted its half from c_s)."""
        lib = get_lib()
        b1, b2 = self.bases
        m1, m2, k = b1.m, b2.m, self.order
        s, bw = f["s"], f["bw"]
        Bb, nb, top_end, h, padt, padb = lay["Bb"], lay["nb"], lay["top_end"], lay["h"], lay["padt"], lay["padb"]
        dev = self._stats.device
        M, Ms, LD = self.Mtot, nb * Bb, bw + 1
        f64 = dict(dtype=torch.float64, device=dev)
        Pt, Pr = torch.empty(Ms * LD, **f64), torch.empty(Ms * LD, **f64)
        tr = torch.zeros(1, **f64)
        check(lib.asvgp_kron_assemble_twisted(f["Ks"][0].data_ptr(), f["Ks"][1].data_ptr(), f["Ss"][0].data_ptr(), f["Ss"][1].data_ptr(),
                                              self.KufKfu_blockband.data_ptr(), k, m1, m2, s, Bb, nb, top_end, padt, padb,
                                              Pt.data_ptr(), Pr.data_ptr(), tr.data_ptr(), stream_ptr()), "kron_assemble_twisted")
        cache = getattr(self, "_twist_cache", None)
        if cache is None or cache["key"] != (Bb, nb, bw):
            r = torch.arange(Bb, device=dev).view(-1, 1).expand(Bb, Bb)
            c = torch.arange(Bb, device=dev).view(1, -1).expand(Bb, Bb)
            low = (r >= c) & (r - c <= bw)
            idx_ss = torch.where(low, (Ms - Bb + c) * LD + (r - c), torch.zeros_like(r))     # P_ss[r, c] inside the top band
            cc_, dd_ = torch.arange(Bb, device=dev).view(-1, 1).expand(Bb, Bb), torch.arange(Bb, device=dev).view(1, -1).expand(Bb, Bb)
            inside = cc_ + dd_ < Bb
            idx_pack = torch.where(inside, (cc_ + dd_) * Bb + cc_, torch.zeros_like(cc_))   # band slot (column cc, offset dd) <- S[cc + dd, cc]
            cache = self._twist_cache = dict(key=(Bb, nb, bw), low=low, idx_ss=idx_ss, inside=inside, idx_pack=idx_pack,
                                             eye=torch.eye(Bb, **f64), side=torch.cuda.Stream(device=dev),
                                             info=torch.zeros(3, dtype=torch.int32, device=dev))
        Pss = torch.where(cache["low"], Pt[cache["idx_ss"]], torch.zeros((), **f64))
        Pss = Pss + Pss.t() - torch.diag(torch.diagonal(Pss))
        c_full = self.Kuf_y.reshape(-1)
        ct, cr = torch.zeros(Ms, **f64), torch.zeros(Ms, **f64)
        ct[padt:] = c_full[:top_end]
        cr[padb:] = c_full[h:].flip(0)
        info = cache["info"]
        cur, side = torch.cuda.current_stream(dev), cache["side"]
        side.wait_stream(cur)
        check(lib.asvgp_blockband_cholesky(Pt.data_ptr(), Ms, bw, ct.data_ptr(), None, info.data_ptr(), stream_ptr()), "blockband_cholesky (top)")
        check(lib.asvgp_blockband_cholesky(Pr.data_ptr(), Ms, bw, cr.data_ptr(), None, info[1:].data_ptr(), ctypes.c_void_p(side.cuda_stream)),
              "blockband_cholesky (bottom)")
        cur.wait_stream(side)
        blocks = torch.empty((2, 2 * nb - 1, Bb, Bb), **f64)
        diag, sub = blocks[:, :nb], blocks[:, nb:]
        for i, Lb in enumerate((Pt, Pr)):
            check(lib.asvgp_blockband_to_blocks(Lb.data_ptr(), Ms, bw, Bb, diag[i].data_ptr(), sub[i].data_ptr(), stream_ptr()), "blockband_to_blocks")
        Lss, Lrs = diag[0, nb - 1], diag[1, nb - 1]
        S = Lss @ Lss.t() + (Lrs @ Lrs.t()).flip(0, 1) - Pss
        r_s = Lss @ ct[Ms - Bb:] + (Lrs @ cr[Ms - Bb:]).flip(0) - c_full[h:top_end]
        Sb = torch.where(cache["inside"], S.reshape(-1)[cache["idx_pack"]], torch.zeros((), **f64)).reshape(-1).contiguous()
        y_S = r_s.clone()
        ld_S = torch.zeros(1, **f64)
        check(lib.asvgp_blockband_cholesky(Sb.data_ptr(), Bb, Bb - 1, y_S.data_ptr(), ld_S.data_ptr(), info[2:].data_ptr(), stream_ptr()),
              "blockband_cholesky (separator)")
        L_S = torch.empty((2, Bb, Bb), **f64)                        # ([1]: the unused sub-diagonal slot of a one-block unpack)
        check(lib.asvgp_blockband_to_blocks(Sb.data_ptr(), Bb, Bb - 1, Bb, L_S[0].data_ptr(), L_S[1].data_ptr(), stream_ptr()), "blockband_to_blocks")
        codes = info.tolist()
        if min(codes) < 0:
            raise AsvgpError("blockband_cholesky gave up waiting for a block column (its workgroup never became resident): results discarded")
        if any(codes):
            where = ("top system, column %d" % (codes[0] - 1 - padt)) if codes[0] else (("bottom system (reversed), column %d" % (codes[1] - 1 - padb)) if codes[1]
                                                                                    else "separator, column %d" % (h + codes[2] - 1))
            raise NotPositiveDefiniteError("P = Kuu + KufKfu/sigma2 not positive definite (%s)" % where)
        Ptv, Prv = Pt.view(Ms, LD), Pr.view(Ms, LD)
        logdet_P = 2.0 * (torch.log(Ptv[:Ms - Bb, 0]).sum() + torch.log(Prv[:Ms - Bb, 0]).sum()) + ld_S[0]
        cc = ((ct[:Ms - Bb] ** 2).sum() + (cr[:Ms - Bb] ** 2).sum() + (y_S ** 2).sum()) / s ** 2
        f.update(logdet_P=logdet_P, trace=tr[0], cc=cc, alpha=None, twist=lay, diag=diag, sub=sub, L_S=L_S[0], y_top=ct, y_bot=cr, y_S=y_S)
        return f

    def elbo(self):
        """gpr.py:282-308."""
        if self._dense_mode:
            return self._dense_elbo_and_grad(want_grad=False)[0]
        f = self._factor(want_alpha=False)
        s = f["s"]
        N, Nw, cw = self._bound_scalars()
        vprod = 1.0
        for kern in self.kernels:
            vprod *= float(kern.variance)                    # gpr.py:284: prod of K_diag
        elbo = -0.5 * N * math.log(2 * math.pi * s)
        elbo = elbo - 0.5 * f["logdet_P"] + 0.5 * f["logdet_K"] - 0.5 * self.tr_yTy / s
        elbo = elbo + 0.5 * f["cc"] - 0.5 * Nw * vprod / s + 0.5 * f["trace"] / s
        if cw:
            elbo = elbo + cw
        return elbo

    def _bound_scalars(self):
        """(N, Nw, cw) of the bound: the -1/2 N log 2 pi s term counts the rows (N+ of a weighted model), the -1/2 Nw v / s trace term
        takes the sum of the weights, cw = 1/2 sum log w is added.  Unweighted: (N, N, 0) - the expressions are the unweighted ones."""
        N = float(self.num_data)
        if self.weights is None:
            return N, N, 0.0
        return N, self.weight_sum, 0.5 * self.log_weight_sum

    def maximum_log_likelihood_objective(self):
        return self.elbo()

    def training_loss(self):
        return -self.elbo()

    @property
    def trainable_parameters(self):
        ps = []
        for kern in self.kernels:
            ps += [kern.variance, kern.lengthscales]
        return ps + [self.likelihood.variance]

    def _selinv(self, f):
        """Sigma = P^-1 on the band, as dense super-blocks (asvgp_blockband_to_blocks + the block recursion with library
        TRSM / GEMM): SigD[i] = Sigma_ii, SigS[i] = Sigma_{i+1,i}, block size Bb = bw rounded up to a multiple of 32."""
        lib = get_lib()
        dev = self._stats.device
        if f.get("twist") is not None:
            return self._selinv_twisted(f)
        bw, M = f["bw"], self.Mtot
        Bb = ((max(bw, 1) + 31) // 32) * 32
        nblk = (M + Bb - 1) // Bb
        diag = torch.empty((nblk, Bb, Bb), dtype=torch.float64, device=dev)
        sub = torch.empty((max(nblk - 1, 1), Bb, Bb), dtype=torch.float64, device=dev)
        check(lib.asvgp_blockband_to_blocks(f["Lb"].data_ptr(), M, bw, Bb, diag.data_ptr(), sub.data_ptr(), stream_ptr()),
              "blockband_to_blocks")
        eye = torch.eye(Bb, dtype=torch.float64, device=dev).expand(nblk, Bb, Bb)
        Linv = torch.linalg.solve_triangular(diag, eye, upper=False)
        Dinv = Linv.transpose(1, 2) @ Linv                       # (L_ii L_ii^T)^-1
        SigD, SigS = torch.empty_like(diag), torch.zeros_like(sub)
        SigD[nblk - 1] = Dinv[nblk - 1]
        if nblk > 1:
            G = sub @ Linv[:-1]                                   # G_i = L_{i+1,i} L_ii^-1
            if f.get("keep_G"):
                f["G"] = G                                        # (for the dense Sigma of _posterior_cov, which drops it again)
            for i in range(nblk - 2, -1, -1):
                SigS[i] = -(SigD[i + 1] @ G[i])
                SigD[i] = Dinv[i] - G[i].t() @ SigS[i]
        if f.get("keep_G"):
            f.setdefault("G", None)                               # (one block: no G)
        if f.get("alpha") is None:   # alpha = L^-T c on the same blocks (40 small matrix-vector steps instead of 512 band launches)
            cb = torch.zeros(nblk * Bb, dtype=torch.float64, device=dev)
            cb[:M] = f["c"].reshape(-1)
            cb = cb.view(nblk, Bb)
            ab = torch.empty_like(cb)
            ab[nblk - 1] = Linv[nblk - 1].t() @ cb[nblk - 1]
            for i in range(nblk - 2, -1, -1):
                ab[i] = Linv[i].t() @ (cb[i] - sub[i].t() @ ab[i + 1])
            f["alpha"] = ab.reshape(-1)[:M].contiguous()
        return SigD, SigS, Bb

    def _selinv_twisted(self, f):
        """The same recursion run OUTWARDS from the separator in both systems at once (batch of two): Sigma_ss = S^-1 seeds the top
        stack, its reversal the bottom stack; nb - 1 dependent steps instead of ceil(M / Bb) - 1.  alpha = P^-1 c / s likewise.
        Three launches per step: N_i = Sigma_{i+1,i+1} G_i (= -Sigma_{i+1,i}), Sigma_ii = D_i^-1 + G_i^T N_i and
        alpha_i = L_i^-T y_i - G_i^T alpha_{i+1} (the triangular-solve form needs L_{i+1,i}^T alpha_{i+1} first: two more products)."""
        lay, s, M = f["twist"], f["s"], self.Mtot
        Bb, nb, top_end, padt, padb = lay["Bb"], lay["nb"], lay["top_end"], lay["padt"], lay["padb"]
        diag, sub = f["diag"], f["sub"]
        dev = diag.device
        f64 = dict(dtype=torch.float64, device=dev)
        eye = self._twist_cache["eye"]
        Linv = torch.linalg.solve_triangular(diag[:, :nb - 1], eye.expand(2, nb - 1, Bb, Bb), upper=False)
        LinvT = Linv.transpose(-1, -2)
        Dinv = (LinvT @ Linv).transpose(0, 1).contiguous()       # step-major [nb-1][2][Bb][Bb]: a step's operands are one contiguous batch
        Gs = (sub @ Linv).transpose(0, 1).contiguous()            # G_i = L_{i+1,i} L_ii^-1
        if f.get("keep_G"):
            f["G"] = Gs                                           # (for the dense Sigma of _posterior_cov, which drops it again)
        GsT = Gs.transpose(-1, -2)
        yb = torch.stack((f["y_top"], f["y_bot"])).view(2, nb, Bb) / s
        Wv = (LinvT @ yb[:, :nb - 1].unsqueeze(-1)).transpose(0, 1).contiguous()        # L_i^-T y_i, [nb-1][2][Bb][1]
        LSinv = torch.linalg.solve_triangular(f["L_S"], eye, upper=False)
        Sig_ss = LSinv.t() @ LSinv
        SigDs = torch.empty((nb, 2, Bb, Bb), **f64)
        Ns = torch.empty((nb - 1, 2, Bb, Bb), **f64)
        abs_ = torch.empty((nb, 2, Bb, 1), **f64)
        SigDs[nb - 1, 0] = Sig_ss
        SigDs[nb - 1, 1] = Sig_ss.flip(0, 1)
        a_s = LSinv.t() @ (f["y_S"] / s)
        abs_[nb - 1, 0, :, 0] = a_s
        abs_[nb - 1, 1, :, 0] = a_s.flip(0)
        for i in range(nb - 2, -1, -1):
            torch.bmm(SigDs[i + 1], Gs[i], out=Ns[i])
            torch.baddbmm(Dinv[i], GsT[i], Ns[i], out=SigDs[i])
            torch.baddbmm(Wv[i], GsT[i], abs_[i + 1], alpha=-1.0, out=abs_[i])
        SigD = SigDs.transpose(0, 1).contiguous()
        SigS = Ns.transpose(0, 1).neg()                           # (contiguous result: Sigma_{i+1,i} = -N_i)
        if not SigS.is_contiguous():
            SigS = SigS.contiguous()
        ab = abs_.squeeze(-1).transpose(0, 1).contiguous()
        alpha = torch.empty(M, **f64)
        alpha[:top_end] = ab[0].reshape(-1)[padt:]
        alpha[top_end:] = ab[1].reshape(-1)[padb:padb + (M - top_end)].flip(0)
        f["alpha"] = alpha
        return SigD, SigS, Bb

    def _grad_terms(self, f, SigD, SigS, Bb, Zs, out):
        lib = get_lib()
        b1, b2 = self.bases
        dKs = f["dKs"]
        tail = (f["alpha"].data_ptr(), self.KufKfu_blockband.data_ptr(), f["Ks"][0].data_ptr(), f["Ks"][1].data_ptr(),
                dKs[0].data_ptr(), dKs[1].data_ptr(), f["Ss"][0].data_ptr(), f["Ss"][1].data_ptr(),
                Zs[0].data_ptr(), Zs[1].data_ptr(), self.order, b1.m, b2.m, out.data_ptr(), stream_ptr())
        lay = f.get("twist")
        if lay is None:
            check(lib.asvgp_kron_grad_terms(SigD.data_ptr(), SigS.data_ptr(), Bb, *tail), "kron_grad_terms")
        else:
            check(lib.asvgp_kron_grad_terms_twisted(SigD.data_ptr(), SigS.data_ptr(), Bb, lay["nb"], lay["top_end"], lay["padt"], lay["padb"], *tail),
                  "kron_grad_terms_twisted")

    def elbo_and_grad(self):
        """(elbo, d elbo / d [v1, l1, v2, l2, sigma2]) - the gradient TF autodiff gives the reference (eNATL60.py:89), here
        analytic: tr(P^-1 dKuu), alpha^T dKuu alpha and tr(Kuu^-1 dKuu Kuu^-1 A) contracted over the block band
        (asvgp_kron_grad_terms) from the band-restricted inverse of P and the two 1-D inverse bands."""
        from . import banded
        lib = get_lib()
        if self._dense_mode:
            e, g = self._dense_elbo_and_grad()
            return float(e), g.cpu().numpy()
        f = self._factor(want_alpha=False)
        SigD, SigS, Bb = self._selinv(f)                         # (also fills f["alpha"])
        s = f["s"]
        N, Nw, cw = self._bound_scalars()
        vs = [float(k.variance) for k in self.kernels]
        ls = [float(k.lengthscales) for k in self.kernels]
        dKs = f["dKs"]
        Zs = [-dS for dS in f["dSs"]]                           # band(K^-1 dK K^-1) = -d band(K^-1)/dl: the exact tangent of the 1-D chain
        out = torch.empty(11, dtype=torch.float64, device=self._stats.device)
        b1, b2 = self.bases
        self._grad_terms(f, SigD, SigS, Bb, Zs, out)
        tPA, aAa, tPX1, aX1a, tPX2, aX2a, tPK, aKa, tZ1A, tZ2A, tSA = out.tolist()
        trK = [float(banded.band_trace_sym(S, dK)) for S, dK in zip(f["Ss"], dKs)]      # tr(K_i^-1 dK_i)
        cc = float(f["cc"])
        yy = float(self.tr_yTy)
        vprod = vs[0] * vs[1]
        elbo = (-0.5 * N * math.log(2 * math.pi * s) - 0.5 * float(f["logdet_P"]) + 0.5 * float(f["logdet_K"]) - 0.5 * yy / s
                + 0.5 * cc - 0.5 * Nw * vprod / s + 0.5 * tSA / s)
        if cw:
            elbo = elbo + cw
        mo = [b2.m, b1.m]                                        # size of the OTHER factor: tr((K1^-1 dK1) (x) I_m2) = m2 tr(K1^-1 dK1)
        g = np.zeros(5)
        for i, (tPX, aXa, tZA) in enumerate(((tPX1, aX1a, tZ1A), (tPX2, aX2a, tZ2A))):
            g[2 * i + 1] = -0.5 * tPX + 0.5 * mo[i] * trK[i] - 0.5 * aXa - 0.5 * tZA / s            # d / d l_i
            g[2 * i] = (0.5 * tPK - 0.5 * self.Mtot + 0.5 * aKa + 0.5 * tSA / s) / vs[i] - 0.5 * Nw * vprod / (vs[i] * s)   # d / d v_i  (dKuu = -Kuu / v_i)
        g[4] = (-0.5 * N / s + 0.5 * tPA / s ** 2 - cc / s + 0.5 * aAa / s ** 2 + 0.5 * yy / s ** 2 + 0.5 * Nw * vprod / s ** 2
                - 0.5 * tSA / s ** 2)
        return elbo, g

    def fit(self, maxiter=200):
        """eNATL60.py:88-89 opt.minimize(model_kron.training_loss, ...): L-BFGS-B on the unconstrained parameters with the
        analytic gradient (one band factorisation + one selected inverse per evaluation)."""
        from scipy.optimize import minimize
        params = self.trainable_parameters

        def fun(u):
            for p, ui in zip(params, u):
                p.unconstrained = float(ui)
            try:
                e, g = self.elbo_and_grad()
            except NotPositiveDefiniteError:
                return np.inf, np.zeros(len(u))
            return -e, -g * np.array([p.dtheta_du() for p in params])

        u0 = np.array([p.unconstrained for p in params])
        res = minimize(fun, u0, jac=True, method="L-BFGS-B", options=dict(maxiter=maxiter))
        for p, ui in zip(params, res.x):
            p.unconstrained = float(ui)
        self._post = None
        return res

    # -- full posterior covariance (d = 2; not in the reference: its predict_f(full_cov=True) raises, gpr.py:310-334) ---------
    def _require_2d(self, what):
        if self._dense_mode:
            raise NotImplementedError("GPR_kron.%s exists for d = 2 only (this model has d = %d)" % (what, self.d))

    def _posterior_cov(self):
        """(Sigma, [K1^-1, K2^-1]) once per theta and layout: Sigma = P^-1 dense (M_tot x M_tot) from the selected inverse of _post
        (asvgp_kron_dense_inverse), K_d^-1 dense per dimension (torch cholesky_inverse of the m_d x m_d Kuu band: negligible next to Sigma)."""
        v, s = self.theta()
        lay = self._twist_layout()
        key = (tuple(v), s, None if lay is None else tuple(sorted(lay.items())))
        if self._post_cov is not None and self._post_cov[0] == key and self._post_cov[3] is self._post:
            return self._post_cov[1], self._post_cov[2]
        self._post_cov = None
        th = self.theta()
        if self._post is None or self._post[0] != th or self._post[1].get("twist") != lay or "G" not in self._post[1]:
            f = self._factor(want_alpha=False)
            f["keep_G"] = True                                    # (_selinv keeps G_i = L_{i+1,i} L_ii^-1 until Sigma is built)
            self._post = (th, f, self._selinv(f))                # (also fills f["alpha"])
        f, (SigD, SigS, Bb) = self._post[1], self._post[2]
        lib = get_lib()
        M = self.Mtot
        dev = self._stats.device
        Sig = torch.empty((M, M), dtype=torch.float64, device=dev)
        if lay is None:
            nb = (M + Bb - 1) // Bb
            G = f.pop("G", None)
            check(lib.asvgp_kron_dense_inverse(G.data_ptr() if nb > 1 else None, SigD.data_ptr(), SigS.data_ptr() if nb > 1 else None, M, Bb,
                                               0, nb, 0, 0, 0, Sig.data_ptr(), stream_ptr()), "kron_dense_inverse")
        else:
            G = f.pop("G").transpose(0, 1).contiguous()          # step-major [nb-1][2] -> stack-major [2][nb-1], SigS's layout
            check(lib.asvgp_kron_dense_inverse(G.data_ptr(), SigD.data_ptr(), SigS.data_ptr(), M, Bb, 1, lay["nb"], lay["top_end"], lay["padt"],
                                               lay["padb"], Sig.data_ptr(), stream_ptr()), "kron_dense_inverse")
            del G
        Kinv = []
        for i, K in enumerate(f["Ks"]):
            L, info = torch.linalg.cholesky_ex(utils.band_to_dense_sym(K))
            if int(info.item()):
                raise NotPositiveDefiniteError("Kuu of dimension %d not positive definite at column %d" % (i, int(info.item()) - 1))
            Kinv.append(torch.cholesky_inverse(L).contiguous())
        self._post_cov = (key, Sig, Kinv, self._post)          # (reused while theta, the layout and the posterior it came from stand)
        return Sig, Kinv

    def predict_f_cov_device(self, X1, X2=None):
        """Posterior cross-covariance cov[f(X1), f(X2)] (n1, n2) as a device tensor; X2=None means X1 against itself.  X: (n, 2).
        k1 k2 + phi^T P^-1 phi' - (phi1^T K1^-1 phi1')(phi2^T K2^-1 phi2') in one kernel (asvgp_predict_cov_kron2d); its diagonal is
        predict_f's variance."""
        self._require_2d("predict_f_cov_device")
        Sig, (K1i, K2i) = self._posterior_cov()
        b1, b2 = self.bases
        k1, k2 = self.kernels
        dev = self._stats.device
        x1 = _to_device(X1, dev).reshape(-1, 2).contiguous()
        x2 = x1 if X2 is None else _to_device(X2, dev).reshape(-1, 2).contiguous()
        n1, n2 = x1.shape[0], x2.shape[0]
        cov = torch.empty((n1, n2), dtype=torch.float64, device=dev)
        check(get_lib().asvgp_predict_cov_kron2d(None, x1.data_ptr(), n1, x2.data_ptr(), n2, b1.mesh.data_ptr(), b1.mesh.shape[0], b1.delta_np,
                                                 b1.m, b2.mesh.data_ptr(), b2.mesh.shape[0], b2.delta_np, b2.m, self.order, Sig.data_ptr(),
                                                 K1i.data_ptr(), K2i.data_ptr(), k1.kind, float(k1.variance), float(k1.lengthscales), k2.kind,
                                                 float(k2.variance), float(k2.lengthscales), cov.data_ptr(), n2, stream_ptr()),
              "predict_cov_kron2d")
        return cov

    def predict_f_gradient_device(self, Xnew):
        """Posterior of the gradient of f at Xnew (n, 2): mean (n, 2) and covariance (n, 2, 2) as device tensors, one per-point kernel
        (asvgp_predict_grad_kron2d) on predict_f_device's factor and selected inverse (_post), in whichever layout _twist_layout() chose.
        cov[:, i, j] = Cov[d_i f, d_j f] = [i = j] c_i v_i / l_i^2 v_other + psi_i^T P^-1 psi_j - (phi1^(a)T K1^-1 phi1^(b))(phi2^(c)T K2^-1 phi2^(d))."""
        self._require_2d("predict_f_gradient_device")
        for i, kern in enumerate(self.kernels):
            _require_derivative(kern, "GPR_kron.predict_f_gradient_device (dimension %d)" % i)
        key, lay = self.theta(), self._twist_layout()
        if self._post is None or self._post[0] != key or self._post[1].get("twist") != lay:
            f = self._factor(want_alpha=False)
            self._post = (key, f, self._selinv(f))               # (also fills f["alpha"])
        f, (SigD, SigS, Bb) = self._post[1], self._post[2]
        b1, b2 = self.bases
        k1, k2 = self.kernels
        X = _to_device(Xnew, self._stats.device).reshape(-1, 2).contiguous()
        n = X.shape[0]
        mean = torch.empty((n, 2), dtype=torch.float64, device=X.device)
        c3 = torch.empty((n, 3), dtype=torch.float64, device=X.device)
        lay = f.get("twist")
        layout = (0, -(-self.Mtot // Bb), 0, 0, 0) if lay is None else (1, lay["nb"], lay["top_end"], lay["padt"], lay["padb"])
        check(get_lib().asvgp_predict_grad_kron2d(X.data_ptr(), n, b1.mesh.data_ptr(), b1.mesh.shape[0], b1.delta_np, b1.m, b2.mesh.data_ptr(),
                                                  b2.mesh.shape[0], b2.delta_np, b2.m, self.order, f["alpha"].data_ptr(), f["Ss"][0].data_ptr(),
                                                  f["Ss"][1].data_ptr(), SigD.data_ptr(), SigS.data_ptr(), Bb, *layout, k1.kind,
                                                  float(k1.variance), float(k1.lengthscales), k2.kind, float(k2.variance),
                                                  float(k2.lengthscales), mean.data_ptr(), c3.data_ptr(), stream_ptr()), "predict_grad_kron2d")
        return mean, c3[:, [0, 1, 1, 2]].reshape(n, 2, 2)

    def predict_f_gradient(self, Xnew):
        """predict_f_gradient_device as numpy: (mean (n, 2), cov (n, 2, 2))."""
        mean, cov = self.predict_f_gradient_device(Xnew)
        return mean.cpu().numpy(), cov.cpu().numpy()

    def predict_f_full_cov(self, Xnew):
        """numpy (mean (n, 1), cov (1, n, n)): gpflow's predict_f(full_cov=True) layout, cov a read-only broadcast."""
        self._require_2d("predict_f_full_cov")
        mean, _ = self.predict_f_device(Xnew)
        cov = self.predict_f_cov_device(Xnew).cpu().numpy()
        return mean.cpu().numpy(), np.broadcast_to(cov, (1,) + cov.shape)

    def predict_f_samples(self, Xnew, num_samples=None, full_cov=True, jitter=1e-6, seed=None):
        """Posterior function samples, numpy (num_samples, n, 1), or (n, 1) when num_samples is None: GPR_1d.predict_f_samples on
        this model's predict_f_device / predict_f_cov_device (same seed and jitter semantics, NotPositiveDefiniteError alike)."""
        self._require_2d("predict_f_samples")
        return GPR_1d.predict_f_samples(self, Xnew, num_samples, full_cov, jitter, seed)

    def close(self):
        """Also releases the cached dense Sigma and K_d^-1."""
        self._post_cov = None
        super().close()

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False):
        """gpr.py:310-334: (mean, var) as numpy (n,1); var = prod v + |L_P^-1 phi*|^2 - phi*^T Kuu^-1 phi*."""
        assert not full_output_cov
        if full_cov:
            raise NotImplementedError
        mean, var = self.predict_f_device(Xnew)
        return mean.cpu().numpy(), var.cpu().numpy()

    def predict_f_sparse(self, Xnew, full_cov=False, full_output_cov=False):
        """gpr.py:336-359: the CHOLMOD route of the same posterior; here both entry points share the band solver.
        Returns (mean (n,1), var (n,1))."""
        mean, var = self.predict_f(Xnew, full_cov, full_output_cov)
        return mean, var[:, :1]

    def predict_f_device(self, Xnew, chunk=4096):
        if self._dense_mode:
            return self._dense_predict(Xnew)
        key = self.theta()
        if self._post is None or self._post[0] != key:
            f = self._factor(want_alpha=False)
            self._post = (key, f, self._selinv(f))               # (also fills f["alpha"])
        mean, qk, qp = self._point_moments(_to_device(Xnew, self._stats.device))
        vprod = 1.0
        for kern in self.kernels:
            vprod *= float(kern.variance)
        var = vprod + qp - qk
        return mean.reshape(-1, 1), var.reshape(-1, 1)

    def _point_moments(self, X):
        """Per row of X (n, 2), from the cached factor and selected inverse (_post): mu = phi^T alpha, q_K = phi^T Kuu^-1 phi and
        g = phi^T P^-1 phi, each (n,)."""
        lib = get_lib()
        f, (SigD, SigS, Bb) = self._post[1], self._post[2]
        b1, b2 = self.bases
        n = X.shape[0]
        mean = torch.empty(n, dtype=torch.float64, device=X.device)
        qk = torch.empty(n, dtype=torch.float64, device=X.device)
        qp = torch.empty(n, dtype=torch.float64, device=X.device)
        check(lib.asvgp_predict_kron2d(X.data_ptr(), n, b1.mesh.data_ptr(), b1.mesh.shape[0], b1.delta_np, b1.m,
                                       b2.mesh.data_ptr(), b2.mesh.shape[0], b2.delta_np, b2.m, self.order,
                                       f["alpha"].data_ptr(), f["Ss"][0].data_ptr(), f["Ss"][1].data_ptr(), mean.data_ptr(),
                                       qk.data_ptr(), stream_ptr()), "predict_kron2d")
        # phi*^T P^-1 phi* (= |L_P^-1 phi*|^2, gpr.py:320-330) straight from the band-restricted inverse
        lay = f.get("twist")
        if lay is None:
            check(lib.asvgp_predict_kron2d_var(X.data_ptr(), n, b1.mesh.data_ptr(), b1.mesh.shape[0], b1.delta_np,
                                               b2.mesh.data_ptr(), b2.mesh.shape[0], b2.delta_np, b2.m, self.order,
                                               SigD.data_ptr(), SigS.data_ptr(), Bb, qp.data_ptr(), stream_ptr()),
                  "predict_kron2d_var")
        else:
            check(lib.asvgp_predict_kron2d_var_twisted(X.data_ptr(), n, b1.mesh.data_ptr(), b1.mesh.shape[0], b1.delta_np,
                                                       b2.mesh.data_ptr(), b2.mesh.shape[0], b2.delta_np, b1.m, b2.m, self.order,
                                                       SigD.data_ptr(), SigS.data_ptr(), Bb, lay["nb"], lay["top_end"], lay["padt"], lay["padb"],
                                                       qp.data_ptr(), stream_ptr()), "predict_kron2d_var_twisted")
        return mean, qk, qp

    # -- changing the weights in place and K-fold cross-validation (d = 2).  Held-out scores take the surface's composition: its
    # predict_f_device is _point_moments (the two kernels that are the cost) plus an elementwise tail -------------------------------
    def _drop_theta_caches(self):
        self._post = self._post_cov = None

    def _restore_weights(self, w):
        self.weights.copy_(w)
        if getattr(self, "_sorted", None) is not None:
            torch.index_select(self.weights, 0, self._sort_perm, out=self._sorted[3])

    def _apply_weights(self, w):
        """validated weights (device, (N,)) into the existing tensors - the sort permutation is kept, only the sorted weights are
        regathered - then what the constructor does after its Phi pass"""
        self._restore_weights(w)
        self._phi_pass_local()
        self._set_weight_sums(self.n, self._wstats, self._pg)
        self._drop_theta_caches()

    def set_weights(self, weights):
        """Replace the per-observation weights of a model built with weights= without rebuilding it: the cell sort of the rows is kept
        (no new argsort), one weighted Phi pass over this rank's rows and the usual all-reduce."""
        if self._dense_mode:
            self._weights_unsupported("set_weights")
        self._set_weights_checked(weights)

    def _weighted_twin(self):
        twin = GPR_kron((self.X, self.y), self.kernels, self.bases, process_group=self._pg, distributed=self._distributed,
                        weights=torch.ones(self.n, dtype=torch.float64, device=self._stats.device))
        twin.likelihood = self.likelihood
        twin.twisted = self.twisted
        return twin

    def kfold_scores(self, folds, refit=False, maxiter=None):
        """GPR_1d.kfold_scores for the d = 2 model (same arguments, same result, same guarantees)."""
        if self._dense_mode:
            self._weights_unsupported("kfold_scores")
        return self._kfold_scores(folds, refit, maxiter)

    def _training_moments(self):
        """_point_moments at this rank's training rows, on the factor and selected inverse of the current theta and layout"""
        key, lay = self.theta(), self._twist_layout()
        if self._post is None or self._post[0] != key or self._post[1].get("twist") != lay:
            f = self._factor(want_alpha=False)
            self._post = (key, f, self._selinv(f))               # (also fills f["alpha"])
        return self._point_moments(self.X)

    # -- gradient of the bound in the weights (d = 2), composed in torch from the per-point kernels as _loo is ----------------------
    def weight_gradient_device(self):
        """GPR_1d.weight_gradient_device for the d = 2 model (D = 1): 1/2 [1 / w_i - (r_i^2 + var_i) / sigma2] with
        var_i = prod v - phi_i^T Kuu^-1 phi_i + g_i; 0 for a row with weight 0."""
        if self._dense_mode:
            self._weights_unsupported("weight_gradient_device")
        mu, qk, g = self._training_moments()
        s = float(self.likelihood.variance)
        vprod = 1.0
        for kern in self.kernels:
            vprod *= float(kern.variance)
        r = self.y.reshape(-1) - mu
        tail = (g + r * r + (vprod - qk)) / s
        if self.weights is None:
            return 0.5 * (1.0 - tail)
        w = self.weights
        pos = w > 0
        return torch.where(pos, 0.5 * (1.0 / torch.where(pos, w, torch.ones_like(w)) - tail), torch.zeros_like(w))

    def noise_group_gradient(self, groups):
        """GPR_1d.noise_group_gradient for the d = 2 model: index_add_ on the per-row gradient."""
        if self._dense_mode:
            self._weights_unsupported("noise_group_gradient")
        return self._noise_group_gradient(groups)

    def fit_noise_groups(self, groups, maxiter=200, pinned=0):
        """GPR_1d.fit_noise_groups for the d = 2 model (same arguments, same result, same guarantees)."""
        if self._dense_mode:
            self._weights_unsupported("fit_noise_groups")
        return self._fit_noise_groups(groups, maxiter, pinned)

    def _bound_and_grad(self):
        e, g = self.elbo_and_grad()
        return float(e), g

    # -- leave-one-out predictions in closed form (d = 2; not in the reference) ------------------------------------------------
    def _loo(self):
        """The formulas of asvgp_loo_1d (include/asvgp_hip.h) in torch on the device, over this rank's rows, from the existing per-point
        kernels: asvgp_predict_kron2d gives mu and q_K, asvgp_predict_kron2d_var (or its twisted form, whichever layout _twist_layout()
        chose) gives g.  Returns (mean (N, 1), var (N, 1), logdens (N,), h (N,), pos (N,) bool); nothing is clamped."""
        mu, qk, g = self._training_moments()
        s = float(self.likelihood.variance)
        vprod = 1.0
        for kern in self.kernels:
            vprod *= float(kern.variance)
        y = self.y.reshape(-1)
        if self.weights is None:
            h, pos, noise = g / s, torch.ones_like(g, dtype=torch.bool), s
        else:
            w = self.weights
            h, pos = w * g / s, w > 0
            noise = torch.where(pos, s / torch.where(pos, w, torch.ones_like(w)), torch.full_like(w, s))
        om = 1.0 - h
        mean = (mu - h * y) / om
        var = vprod + g - qk + g * (h / om)
        s2 = var + noise
        ld = -0.5 * (torch.log(2 * math.pi * s2) + (y - mean) ** 2 / s2)
        return mean.reshape(-1, 1), var.reshape(-1, 1), ld, h, pos

    def loo_predict_f_device(self):
        """Mean (N, 1) and variance (N, 1) of f(x_i) given every training row but i (this rank's rows of a sharded model), as device
        tensors; no refits.  A row with weight 0 is absent from the model already: its entries are predict_f_device's."""
        self._require_2d("loo_predict_f_device")
        return self._loo()[:2]

    def loo_log_density_device(self):
        """log p(y_i | y_-i) (N,) as a device tensor; the left-out observation's noise variance is sigma2 / w_i (sigma2 for weight 0)."""
        self._require_2d("loo_log_density_device")
        return self._loo()[2]

    def _loo_scores_device(self):
        self._require_2d("loo_scores")
        mean, _, ld, h, pos = self._loo()
        zero = torch.zeros((), dtype=torch.float64, device=ld.device)
        sq = (self.y.reshape(-1) - mean.reshape(-1)) ** 2
        # (sums over the rows with w > 0 only; a NaN leverage must reach max h, which amax propagates)
        return torch.stack([pos.sum().to(torch.float64), torch.where(pos, ld, zero).sum(), torch.where(pos, sq, zero).sum(),
                            torch.where(pos, h, zero).amax() if h.numel() else zero])


class GPR_additive(_GPModelSurface, _ShardedStats):
    """Drop-in for asvgp/gpr.py:139-236: GPR_additive((X[N,d], y[N,1]), kernels, bases) with elbo(),
    maximum_log_likelihood_objective(), training_loss(), predict_f(Xnew), fit().

    Kuf = vstack(Kuf_i) is never built (gpr.py:169-172 vstack + SpGEMM + todense): the banded diagonal blocks, Kuf_i y and
    y^T y come from the 1-D Phi pass per dimension (asvgp_phi_accumulate_1d), the dense cross blocks Kuf_i Kuf_j^T from
    asvgp_phi_cross_2d; all of them live in ONE flat buffer so that N-shards need a single all-reduce.  The M_tot^3 part
    (Cholesky of P = blockdiag(Kuu_i) + KufKfu / sigma2, gpr.py:191-194) stays dense as in the reference (rocSOLVER through
    torch.linalg); log|Kuu| and tr(Kuu^-1 KufKfu) use the banded operators block by block."""

    def __init__(self, data, kernels, bases, process_group=None, distributed=None, *, weights=None):
        if weights is not None:
            raise NotImplementedError("GPR_additive(weights=...): per-observation weights are implemented for GPR_1d and GPR_kron (d = 2) "
                                      "only - the additive model's cross blocks have no weighted Phi pass yet")
        dev = bases[0].device
        self.X, self.y = _to_device(data[0], dev), _to_device(data[1], dev)
        self.n, self.d = self.X.shape[0], self.X.shape[1]
        assert len(kernels) == len(bases) == self.d          # gpr.py:147
        assert self.y.shape[1] == 1                          # gpr.py:148
        for kern in kernels:                                 # gpr.py:151-152
            assert isinstance(kern, (kernels_mod.Matern12, kernels_mod.Matern32, kernels_mod.Matern52))
        require_cuda(self.X, self.y)
        self.kernel = kernels[-1]                            # gpr.py:155 passes the leaked loop variable
        self.likelihood = kernels_mod.Gaussian()
        self.bases, self.kernels = bases, kernels
        self.inducing_features = [SplineFeatures1D(kernels[i], bases[i]) for i in range(self.d)]
        bandwidths = [bs.order for bs in bases]              # gpr.py:162-165
        assert all(x == bandwidths[0] for x in bandwidths)
        self.bandwidth = k = bases[0].order
        for i, bs in enumerate(bases):
            _require_inside(self.X[:, i], bs.a, bs.b, True, "GPR_additive dimension %d" % i)
        lib = get_lib()
        ms = [bs.m for bs in bases]
        self.offsets = [0]
        for m in ms:
            self.offsets.append(self.offsets[-1] + m)
        self.Mtot = self.offsets[-1]
        # flat statistics buffer: per dimension [(k+1) m_i band | m_i rhs | yy], then the cross blocks (i < j) row-major
        self._diag_off, self._cross_off, o = [], {}, 0
        for m in ms:
            self._diag_off.append(o)
            o += (k + 2) * m + 1
        for i in range(self.d):
            for j in range(i + 1, self.d):
                self._cross_off[(i, j)] = o
                o += ms[i] * ms[j]
        self._stats = torch.empty(o, dtype=torch.float64, device=dev)
        self._cols = [self.X[:, i].contiguous() for i in range(self.d)]
        wsb = max([lib.asvgp_phi_workspace_bytes(m, k, 1) for m in ms] +
                  [lib.asvgp_phi_cross_workspace_bytes(ms[i], ms[j]) for (i, j) in self._cross_off] + [8])
        self._ws = torch.empty(wsb // 8 + 1, dtype=torch.float64, device=dev)
        self._wsb = wsb
        self._h = Handle()
        self._setup_dist(process_group, distributed)
        self._phi_pass_local()
        self.num_data = allreduce_stats(self._stats, self.n, process_group) if self._distributed else self.n
        self.tr_yTy = self._stats[self._diag_off[0] + (k + 2) * ms[0]]      # gpr.py:168
        self._info = torch.zeros(1, dtype=torch.int32, device=dev)
        self._dense = None
        self._post_cov = None                 # (key, W, concatenated meshes) of predict_f_cov_device
        self._post_alpha = None               # (key, alpha = P^-1 Kuf y / sigma2) from the factor W came from

    # ------------------------------------------------------------------------------------------------------
    def _phi_pass_local(self):
        lib, k = get_lib(), self.bandwidth
        for i, bs in enumerate(self.bases):
            out = self._stats[self._diag_off[i]:]
            check(lib.asvgp_phi_accumulate_1d(self._h.ptr, self._cols[i].data_ptr(), self.y.data_ptr(), self.n, 1, bs.mesh.data_ptr(),
                                              bs.mesh.shape[0], bs.delta_np, k, bs.m, out.data_ptr(), self._ws.data_ptr(),
                                              self._wsb, stream_ptr()), "phi_accumulate_1d")
        # deferred-reduce mode is a GPR_1d scheduling aid; here the last dimension's parked reduce goes out before the cross blocks
        # (the earlier ones were flushed by the next accumulate call on the shared handle)
        check(lib.asvgp_phi_reduce_1d(self._h.ptr, stream_ptr()), "phi_reduce_1d")
        for (i, j), o in self._cross_off.items():
            bi, bj = self.bases[i], self.bases[j]
            check(lib.asvgp_phi_cross_2d(self._cols[i].data_ptr(), self._cols[j].data_ptr(), self.n, bi.mesh.data_ptr(),
                                         bi.mesh.shape[0], bi.delta_np, bi.m, bj.mesh.data_ptr(), bj.mesh.shape[0],
                                         bj.delta_np, bj.m, k, self._stats[o:].data_ptr(), self._ws.data_ptr(), self._wsb,
                                         stream_ptr()), "phi_cross_2d")
        self._dense = None
        self._post_cov = None                 # (W was built from the statistics just replaced)
        self._post_alpha = None
        return self._stats

    def _band(self, i):
        k, m, o = self.bandwidth, self.bases[i].m, self._diag_off[i]
        return self._stats[o:o + (k + 1) * m].view(k + 1, m)

    @property
    def KufKfu(self):
        """gpr.py:171: dense (M_tot, M_tot) Kuf @ Kuf.T assembled from the banded diagonal and dense cross blocks."""
        if self._dense is None:
            A = torch.zeros((self.Mtot, self.Mtot), dtype=torch.float64, device=self._stats.device)
            for i in range(self.d):
                a, b = self.offsets[i], self.offsets[i + 1]
                A[a:b, a:b] = utils.band_to_dense_sym(self._band(i))
            for (i, j), o in self._cross_off.items():
                mi, mj = self.bases[i].m, self.bases[j].m
                C = self._stats[o:o + mi * mj].view(mi, mj)
                A[self.offsets[i]:self.offsets[i + 1], self.offsets[j]:self.offsets[j + 1]] = C
                A[self.offsets[j]:self.offsets[j + 1], self.offsets[i]:self.offsets[i + 1]] = C.t()
            self._dense = A
        return self._dense

    @property
    def Kuf_y(self):
        """gpr.py:172: (M_tot, 1)."""
        k = self.bandwidth
        parts = [self._stats[o + (k + 1) * bs.m:o + (k + 2) * bs.m] for o, bs in zip(self._diag_off, self.bases)]
        return torch.cat(parts).reshape(-1, 1)

    def theta(self):
        return [(float(kn.variance), float(kn.lengthscales)) for kn in self.kernels], float(self.likelihood.variance)

    def _factor(self):
        from . import banded
        s = float(self.likelihood.variance)
        Ks = [f.make_Kuu(kn) for f, kn in zip(self.inducing_features, self.kernels)]
        Ls = [banded.cholesky_band(K) for K in Ks]
        logdet_K = sum(torch.log(L[0] ** 2).sum() for L in Ls)                      # gpr.py:187 (block diagonal)
        trace = sum(banded.band_trace_sym(banded.inverse_from_cholesky_band(L), self._band(i))
                    for i, L in enumerate(Ls))                                      # gpr.py:208: only diagonal blocks count
        P = self.KufKfu / s
        for i, K in enumerate(Ks):
            a, b = self.offsets[i], self.offsets[i + 1]
            P[a:b, a:b] += utils.band_to_dense_sym(K)
        L, info = torch.linalg.cholesky_ex(P)                                       # gpr.py:192
        if int(info.item()):
            raise NotPositiveDefiniteError("P = Kuu + KufKfu/sigma2 not positive definite at column %d" % (int(info.item()) - 1))
        c = torch.linalg.solve_triangular(L, self.Kuf_y, upper=False) / s           # gpr.py:194
        return dict(Ks=Ks, Ls=Ls, logdet_K=logdet_K, trace=trace, L=L, c=c, s=s)

    def elbo(self):
        """gpr.py:177-209."""
        f = self._factor()
        s, N = f["s"], float(self.num_data)
        vsum = sum(float(kn.variance) for kn in self.kernels)                      # gpr.py:181
        elbo = -0.5 * N * math.log(2 * math.pi * s)
        elbo = elbo - 0.5 * torch.log(torch.diagonal(f["L"]) ** 2).sum() + 0.5 * f["logdet_K"] - 0.5 * self.tr_yTy / s
        elbo = elbo + 0.5 * (f["c"] ** 2).sum() - 0.5 * N * vsum / s + 0.5 * f["trace"] / s
        return elbo

    def maximum_log_likelihood_objective(self):
        return self.elbo().sum()                                                    # gpr.py:174-175

    def training_loss(self):
        return -self.maximum_log_likelihood_objective()

    @property
    def trainable_parameters(self):
        ps = []
        for kn in self.kernels:
            ps += [kn.variance, kn.lengthscales]
        return ps + [self.likelihood.variance]

    def elbo_and_grad(self):
        """Bound and its ANALYTIC gradient with respect to (variance_1, lengthscale_1, ..., variance_d, lengthscale_d, noise
        variance) - what TF autodiff through gpr.py:177-209 hands the optimiser.  With G = 1/2 (Kuu^-1 - P^-1 - alpha alpha^T
        - Kuu^-1 A Kuu^-1 / s) (Kuu block diagonal, P and A dense here) d/d theta_i = <G_ii, dKuu_i/d theta_i>
        over the band of block i: band(Kuu_i^-1) and its exact lengthscale tangent come from asvgp_kuu_inverse_band_1d,
        the diagonal blocks of P^-1 from the dense factor (torch.cholesky_inverse, O(M_tot^3) like the factorisation itself)."""
        from . import banded
        s, N = float(self.likelihood.variance), float(self.num_data)
        k = self.bandwidth
        Ks, dKs, Ss, dSs, lds = [], [], [], [], []
        for feat, kern in zip(self.inducing_features, self.kernels):
            K, dK, S, dS, ld2, _ = feat.inverse_band(kern)
            Ks.append(K); dKs.append(dK); Ss.append(S); dSs.append(dS); lds.append(ld2)
        for i, feat in enumerate(self.inducing_features):
            col = int(feat._info[0].item())
            if col:
                raise NotPositiveDefiniteError("Kuu band of dimension %d not positive definite at column %d" % (i, col - 1))
        A = self.KufKfu
        P = A / s
        for i, K in enumerate(Ks):
            a, b = self.offsets[i], self.offsets[i + 1]
            P[a:b, a:b] += utils.band_to_dense_sym(K)
        L, info = torch.linalg.cholesky_ex(P)
        if int(info.item()):
            raise NotPositiveDefiniteError("P = Kuu + KufKfu/sigma2 not positive definite at column %d" % (int(info.item()) - 1))
        bvec = self.Kuf_y
        alpha = torch.cholesky_solve(bvec, L) / s                                  # P^-1 b / s
        Pinv = torch.cholesky_inverse(L)
        yy = self.tr_yTy
        vsum = sum(float(kn.variance) for kn in self.kernels)
        logdet_P = torch.log(torch.diagonal(L) ** 2).sum()
        logdet_K = sum(ld[0] for ld in lds)
        trace = sum(banded.band_trace_sym(Ss[i], self._band(i)) for i in range(self.d))
        bTa = (bvec * alpha).sum()                                                  # b^T P^-1 b / s = s |c|^2
        elbo = -0.5 * N * math.log(2 * math.pi * s) - 0.5 * logdet_P + 0.5 * logdet_K - 0.5 * yy / s
        elbo = elbo + 0.5 * bTa / s - 0.5 * N * vsum / s + 0.5 * trace / s
        grads = []
        w = torch.ones((k + 1, 1), dtype=torch.float64, device=A.device) * 2.0
        w[0, 0] = 1.0                                                               # symmetric band: off-diagonals count twice

        def band_of(Mat, m):                                                        # lower band [(k+1), m] of a dense block
            out = torch.zeros((k + 1, m), dtype=torch.float64, device=Mat.device)
            for d in range(k + 1):
                out[d, :m - d] = torch.diagonal(Mat, -d)
            return out

        for i, kern in enumerate(self.kernels):
            a, b = self.offsets[i], self.offsets[i + 1]
            m = b - a
            v = float(kern.variance)
            Pb = band_of(Pinv[a:b, a:b], m)
            al = alpha[a:b, 0]
            aab = torch.zeros((k + 1, m), dtype=torch.float64, device=A.device)     # band of alpha alpha^T
            for d in range(k + 1):
                aab[d, :m - d] = al[d:] * al[:m - d]
            Ai = self._band(i)

            def inner(Xb, Yb):
                return (w * Xb * Yb).sum()
            # <G_ii, dK> with <Kuu^-1 A Kuu^-1, dK> = -<dS, A> for the lengthscale and = <S, A> / v ... for the variance (dKuu/dv = -Kuu/v)
            d_l = 0.5 * (inner(Ss[i], dKs[i]) - inner(Pb, dKs[i]) - inner(aab, dKs[i]) + inner(dSs[i], Ai) / s)
            d_v = 0.5 * (-inner(Ss[i], Ks[i]) / v + inner(Pb, Ks[i]) / v + inner(aab, Ks[i]) / v + inner(Ss[i], Ai) / (v * s)) - 0.5 * N / s
            grads += [d_v, d_l]
        s2 = s * s
        trPA = (Pinv * A).sum()
        aAa = (alpha.t() @ A @ alpha).reshape(())
        d_s = -0.5 * N / s + 0.5 * trPA / s2 + 0.5 * yy / s2 + 0.5 * aAa / s2 - bTa / s2 + 0.5 * N * vsum / s2 - 0.5 * trace / s2
        grads.append(d_s)
        return elbo, torch.stack([g.reshape(()) if isinstance(g, torch.Tensor) else torch.tensor(g, dtype=torch.float64, device=A.device)
                                  for g in grads])

    def fit(self, maxiter=200):
        """L-BFGS-B on the softplus-unconstrained parameters with the analytic gradient of elbo_and_grad (round 1 used 2 P
        central-difference evaluations of the bound per step; the reference relies on TF autodiff through its dense ops)."""
        from scipy.optimize import minimize
        params = self.trainable_parameters

        def fun(u):
            for p, ui in zip(params, u):
                p.unconstrained = float(ui)
            try:
                e, g = self.elbo_and_grad()
            except NotPositiveDefiniteError:
                return float("inf"), np.zeros_like(u)
            g = g.cpu().numpy() * np.array([p.dtheta_du() for p in params])
            return -float(e), -g

        u0 = np.array([p.unconstrained for p in params])
        res = minimize(fun, u0, jac=True, method="L-BFGS-B", options=dict(maxiter=maxiter))
        for p, ui in zip(params, res.x):
            p.unconstrained = float(ui)
        return res

    def predict_f_device(self, Xnew, chunk=8192):
        from . import banded
        Xn = _to_device(Xnew, self._stats.device)
        assert Xn.shape[1] == self.d
        f = self._factor()
        vsum = sum(float(kn.variance) for kn in self.kernels)
        means, vars_ = [], []
        for lo in range(0, Xn.shape[0], chunk):
            xs = Xn[lo:lo + chunk]
            Kus = torch.cat([bs.evaluate_basis(xs[:, i:i + 1].contiguous(), sparse=False) for i, bs in enumerate(self.bases)], 0)
            tmp = torch.linalg.solve_triangular(f["L"], Kus, upper=False)            # gpr.py:226
            means.append(tmp.t() @ f["c"])                                          # gpr.py:227
            q = torch.zeros(xs.shape[0], dtype=torch.float64, device=xs.device)
            for i, Lb in enumerate(f["Ls"]):                                         # gpr.py:228: Kuu.solve, block by block
                Ki = Kus[self.offsets[i]:self.offsets[i + 1]]
                w = banded.solve_triang_mat(Lb, Ki)
                q += (w * w).sum(0)
            vars_.append(vsum + (tmp * tmp).sum(0) - q)                             # gpr.py:230-232
        mean = torch.cat(means, 0) if means else torch.zeros((0, 1), dtype=torch.float64, device=Xn.device)
        var = torch.cat(vars_, 0) if vars_ else torch.zeros(0, dtype=torch.float64, device=Xn.device)
        return mean, var.reshape(-1, 1).repeat(1, self.y.shape[1])                  # gpr.py:233-234

    # -- full posterior covariance (not in the reference: its predict_f ignores full_cov, gpr.py:211-236) ---------------------
    def _posterior_cov(self):
        """W = P^-1 - blockdiag(K_1^-1 .. K_d^-1) (M_tot x M_tot, device) once per theta: cholesky_inverse of the dense factor of
        _factor, then each dimension's dense K_i^-1 (torch cholesky_inverse of the m_i x m_i Kuu band) subtracted from its block.
        Cached on _post_cov with the concatenated meshes; alpha = P^-1 Kuf y / sigma2 (M_tot), from the same factor, on _post_alpha under
        the same key.  _phi_pass_local and close() drop both."""
        v, s = self.theta()
        key = (tuple(v), s)
        if self._post_cov is not None and self._post_cov[0] == key and self._post_alpha is not None and self._post_alpha[0] == key:
            return self._post_cov[1], self._post_cov[2]
        self._post_cov = self._post_alpha = None
        f = self._factor()
        alpha = torch.linalg.solve_triangular(f["L"].t(), f["c"], upper=True).reshape(-1).contiguous()   # L^-T (L^-1 Kuf y / s)
        W = self._minus_kuu_inverse(torch.cholesky_inverse(f["L"]), f["Ks"])
        meshes = torch.cat([bs.mesh.reshape(-1) for bs in self.bases]).contiguous()
        self._post_cov = (key, W, meshes)
        self._post_alpha = (key, alpha)
        return W, meshes

    def _minus_kuu_inverse(self, W, Ks):
        """W - blockdiag(K_1^-1 .. K_d^-1), symmetrised; W is overwritten.  Dimensions of equal m_i share one batched factorisation
        and inverse."""
        groups = {}
        for i, bs in enumerate(self.bases):
            groups.setdefault(bs.m, []).append(i)
        for dims in groups.values():
            L, info = torch.linalg.cholesky_ex(torch.stack([utils.band_to_dense_sym(Ks[i]) for i in dims]))
            for i, col in zip(dims, info.tolist()):
                if col:
                    raise NotPositiveDefiniteError("Kuu of dimension %d not positive definite at column %d" % (i, col - 1))
            Kinv = torch.cholesky_inverse(L)
            for j, i in enumerate(dims):
                a, b = self.offsets[i], self.offsets[i + 1]
                W[a:b, a:b] -= Kinv[j]
        return (0.5 * (W + W.t())).contiguous()   # (exactly symmetric: cov(X1, X2) = cov(X2, X1)^T up to the rounding of the sums)

    def predict_f_cov_device(self, X1, X2=None):
        """Posterior cross-covariance cov[f(X1), f(X2)] (n1, n2) as a device tensor; X2=None means X1 against itself.  X: (n, d).
        sum_i k_i(x_i, x'_i) + phi(x)^T W phi(x') in one kernel (asvgp_predict_cov_additive); its diagonal is predict_f's variance."""
        dev, d = self._stats.device, self.d
        x1 = _to_device(X1, dev).reshape(-1, d).contiguous()
        x2 = x1 if X2 is None else _to_device(X2, dev).reshape(-1, d).contiguous()
        n1, n2 = x1.shape[0], x2.shape[0]
        cov = torch.empty((n1, n2), dtype=torch.float64, device=dev)
        if n1 == 0 or n2 == 0:
            return cov
        W, meshes = self._posterior_cov()
        arr = lambda t, vals: (t * d)(*vals)
        check(get_lib().asvgp_predict_cov_additive(None, x1.data_ptr(), n1, x2.data_ptr(), n2, d, meshes.data_ptr(),
                                                   arr(ctypes.c_int64, [bs.mesh.shape[0] for bs in self.bases]),
                                                   arr(ctypes.c_double, [bs.delta_np for bs in self.bases]),
                                                   arr(ctypes.c_int64, [bs.m for bs in self.bases]), self.bandwidth,
                                                   arr(ctypes.c_int, [kn.kind for kn in self.kernels]),
                                                   arr(ctypes.c_double, [float(kn.variance) for kn in self.kernels]),
                                                   arr(ctypes.c_double, [float(kn.lengthscales) for kn in self.kernels]),
                                                   W.data_ptr(), cov.data_ptr(), n2, stream_ptr()), "predict_cov_additive")
        return cov

    def predict_f_full_cov(self, Xnew):
        """numpy (mean (n, 1), cov (1, n, n)): gpflow's predict_f(full_cov=True) layout, cov a read-only broadcast."""
        mean, _ = self.predict_f_device(Xnew)
        cov = self.predict_f_cov_device(Xnew).cpu().numpy()
        return mean.cpu().numpy(), np.broadcast_to(cov, (1,) + cov.shape)

    def predict_f_samples(self, Xnew, num_samples=None, full_cov=True, jitter=1e-6, seed=None):
        """Posterior function samples, numpy (num_samples, n, 1), or (n, 1) when num_samples is None: GPR_1d.predict_f_samples on
        this model's predict_f_device / predict_f_cov_device (same seed and jitter semantics, NotPositiveDefiniteError alike)."""
        return GPR_1d.predict_f_samples(self, Xnew, num_samples, full_cov, jitter, seed)

    # -- components f_i(x_i) and gradient d f / d x_i = f_i'(x_i) (not in the reference: its predict_f returns the sum) ---------------
    def _predict_components(self, Xnew, deriv, what):
        """mean (n, d) and cov (n, d, d) of phi_i^(p)(x_i) against alpha and W (asvgp_predict_components_additive), p = deriv."""
        if deriv:
            for i, kern in enumerate(self.kernels):
                _require_derivative(kern, "%s (dimension %d)" % (what, i))
        dev, d = self._stats.device, self.d
        X = _to_device(Xnew, dev).reshape(-1, d).contiguous()
        n = X.shape[0]
        mean = torch.empty((n, d), dtype=torch.float64, device=dev)
        cov = torch.empty((n, d, d), dtype=torch.float64, device=dev)
        if n == 0:
            return mean, cov
        W, meshes = self._posterior_cov()
        alpha = self._post_alpha[1]
        arr = lambda t, vals: (t * d)(*vals)
        check(get_lib().asvgp_predict_components_additive(None, X.data_ptr(), n, d, meshes.data_ptr(),
                                                          arr(ctypes.c_int64, [bs.mesh.shape[0] for bs in self.bases]),
                                                          arr(ctypes.c_double, [bs.delta_np for bs in self.bases]),
                                                          arr(ctypes.c_int64, [bs.m for bs in self.bases]), self.bandwidth,
                                                          arr(ctypes.c_int, [kn.kind for kn in self.kernels]),
                                                          arr(ctypes.c_double, [float(kn.variance) for kn in self.kernels]),
                                                          arr(ctypes.c_double, [float(kn.lengthscales) for kn in self.kernels]), deriv,
                                                          alpha.data_ptr(), W.data_ptr(), mean.data_ptr(), cov.data_ptr(), stream_ptr()),
              "predict_components_additive")
        return mean, cov

    def predict_f_components_device(self, Xnew):
        """Posterior of the additive components f_i(x_i) at Xnew (n, d): mean (n, d) and covariance (n, d, d) as device tensors,
        cov[:, i, j] = Cov[f_i(x_i), f_j(x_j)] = [i = j] v_i + phi_i^T W_ij phi_j, from predict_f_cov_device's cached W and alpha.
        Summed over i (and i, j) they give predict_f's mean (and variance).  Every Matern."""
        return self._predict_components(Xnew, 0, "GPR_additive.predict_f_components_device")

    def predict_f_components(self, Xnew):
        """predict_f_components_device as numpy: (mean (n, d), cov (n, d, d))."""
        mean, cov = self.predict_f_components_device(Xnew)
        return mean.cpu().numpy(), cov.cpu().numpy()

    def predict_f_gradient_device(self, Xnew):
        """Posterior of the gradient of f at Xnew (n, d): mean (n, d) and covariance (n, d, d) as device tensors, d f / d x_i = f_i'(x_i),
        cov[:, i, j] = [i = j] c_i v_i / l_i^2 + phi_i'^T W_ij phi_j' (c = 3 for Matern-3/2, 5/3 for Matern-5/2).  A Matern-1/2 dimension
        raises ValueError before anything is built or launched."""
        return self._predict_components(Xnew, 1, "GPR_additive.predict_f_gradient_device")

    def predict_f_gradient(self, Xnew):
        """predict_f_gradient_device as numpy: (mean (n, d), cov (n, d, d))."""
        mean, cov = self.predict_f_gradient_device(Xnew)
        return mean.cpu().numpy(), cov.cpu().numpy()

    def close(self):
        """Also releases the cached dense W and alpha."""
        self._post_cov = self._post_alpha = None
        super().close()

    def predict_f(self, Xnew, full_cov=False, full_output_cov=False):
        mean, var = self.predict_f_device(Xnew)
        return mean.cpu().numpy(), var.cpu().numpy()
