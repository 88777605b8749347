"""CPU: the held-out score entry points (asvgp_score_workspace_bytes, asvgp_score_1d) are exported with prototypes, their argument checks
fail loudly on the host before anything is launched, and the host-side validation of the Python surface (held-out rows and weights, fold
labels, the refusals of the models without a weighted Phi pass) needs no GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from asvgp_amd import build, _lib
    build.build(verbose=False)
    return _lib.get_lib()


NAMES = ("asvgp_score_workspace_bytes", "asvgp_score_1d")


def test_symbols_exported_with_prototypes(lib):
    from asvgp_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n)
        assert n in _lib.SIGNATURES
        assert getattr(lib, n).argtypes is not None
    # asvgp_loo_1d without Pinv_band
    loo, score = _lib.SIGNATURES["asvgp_loo_1d"], _lib.SIGNATURES["asvgp_score_1d"]
    assert score[0] is loo[0] and score[1] == loo[1][:13] + loo[1][14:]
    assert _lib.SIGNATURES["asvgp_score_workspace_bytes"] == _lib.SIGNATURES["asvgp_loo_workspace_bytes"]


def _err(lib):
    return lib.asvgp_last_error_string().decode()


FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: every call below is refused on the host (or has nothing to do)
ODD = ctypes.c_void_p(0x1008)    # 8-byte but not 16-byte aligned: accepted like any other


def _score(lib, x=FAKE, y=FAKE, w=FAKE, N=10, D=1, mesh=FAKE, n_mesh=14, order=3, M=16, alpha=FAKE, W=FAKE, variance=1.0, noise=0.1,
           mean=FAKE, var=FAKE, logdens=FAKE, scores=FAKE, ws=FAKE, wsb=None):
    if wsb is None:
        wsb = lib.asvgp_score_workspace_bytes(M, min(max(order, 1), 6), max(D, 1))
    return lib.asvgp_score_1d(None, x, y, w, N, D, mesh, n_mesh, 0.1, order, M, alpha, W, variance, noise, mean, var, logdens, scores,
                              ws, wsb, None)


def test_score_workspace_bytes(lib):
    assert lib.asvgp_score_workspace_bytes(16, 3, 1) >= 8 * 4
    for order in range(1, 7):
        assert lib.asvgp_score_workspace_bytes(2048, order, 3) > 0
    assert lib.asvgp_score_workspace_bytes(0, 3, 1) == 0 and lib.asvgp_score_workspace_bytes(-5, 3, 1) == 0
    assert lib.asvgp_score_workspace_bytes(16, 7, 1) == 0 and lib.asvgp_score_workspace_bytes(16, 0, 1) == 0
    assert lib.asvgp_score_workspace_bytes(16, 3, 0) == 0


def test_score_argument_checks(lib):
    for kw in ({"x": None}, {"y": None}, {"mesh": None}, {"alpha": None}, {"W": None}, {"N": -1}, {"D": 0}, {"D": -2},
               {"n_mesh": 15}, {"n_mesh": 13}, {"variance": 0.0}, {"variance": -1.0}, {"variance": float("nan")}, {"noise": 0.0},
               {"noise": -0.5}, {"noise": float("nan")}, {"mean": None, "var": None, "logdens": None, "scores": None}, {"ws": None}):
        rc = _score(lib, **kw)
        assert rc == (-1 if "ws" not in kw else -4), kw
        assert "score_1d" in _err(lib)
    assert _score(lib, order=7, n_mesh=10) == -2
    assert "score_1d" in _err(lib) and "order 7" in _err(lib)
    assert _score(lib, order=0, n_mesh=17) == -2 and "score_1d" in _err(lib)
    assert _score(lib, wsb=lib.asvgp_score_workspace_bytes(16, 3, 1) - 8) == -4                        # ASVGP_ERR_WORKSPACE
    assert "score_1d" in _err(lib) and "workspace" in _err(lib)


def test_score_empty_batch_is_ok(lib):
    # nothing to stream: no launch.  (scores, which an empty batch zeroes on the device, are not asked for here)
    assert _score(lib, N=0, scores=None) == 0
    assert _score(lib, N=0, scores=None, x=None, y=None, w=None) == 0
    assert _score(lib, N=0, scores=None, var=None, logdens=None, mean=ODD) == 0
    # weights are optional: NULL means all ones, so it is not among the required pointers
    assert _score(lib, N=0, w=None, scores=None) == 0


# ------------------------------------------------------------------------------------------------ Python surface, host-side logic
CPU = torch.device("cpu")


def test_heldout_validation_raises_on_host_tensors():
    from asvgp_amd.gpr import _prepare_heldout
    X, Y = np.linspace(0.1, 0.9, 6).reshape(6, 1), np.zeros((6, 2))
    Xt, Yt, w = _prepare_heldout((X, Y), None, 1, 2, CPU, "GPR_1d.score")
    assert w is None and tuple(Xt.shape) == (6, 1) and tuple(Yt.shape) == (6, 2) and Xt.dtype == Yt.dtype == torch.float64
    Xt, Yt, w = _prepare_heldout((X.reshape(-1).astype(np.float32), np.zeros(6)), np.arange(6).reshape(6, 1), 1, 1, CPU, "GPR_1d.score")
    assert tuple(Xt.shape) == (6, 1) and tuple(Yt.shape) == (6, 1) and w.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    for bad in (-1.0, float("nan"), float("inf")):
        wb = np.ones(6)
        wb[3] = bad
        with pytest.raises(ValueError, match="GPR_1d.score.*row 3"):
            _prepare_heldout((X, Y), wb, 1, 2, CPU, "GPR_1d.score")
    with pytest.raises(ValueError, match="shape"):
        _prepare_heldout((X, Y), np.ones(5), 1, 2, CPU, "GPR_1d.score")
    with pytest.raises(ValueError, match="Xnew"):
        _prepare_heldout((np.zeros((6, 2)), Y), None, 1, 2, CPU, "GPR_1d.score")
    with pytest.raises(ValueError, match="Xnew"):
        _prepare_heldout((np.zeros(6), np.zeros((6, 1))), None, 2, 1, CPU, "GPR_kron.score")
    with pytest.raises(ValueError, match="Ynew"):
        _prepare_heldout((X, np.zeros((5, 2))), None, 1, 2, CPU, "GPR_1d.score")
    with pytest.raises(ValueError, match="Ynew"):
        _prepare_heldout((X, np.zeros((6, 1))), None, 1, 2, CPU, "GPR_1d.score")


def test_fold_validation_raises_on_host_tensors():
    from asvgp_amd.gpr import _prepare_folds, _require_folds_populated
    what = "GPR_1d.kfold_scores"
    f, counts = _prepare_folds(np.array([0, 2, 1, 2, 0, 1]), 6, None, CPU, what)
    assert f.dtype == torch.int64 and counts.tolist() == [2, 2, 2]
    _require_folds_populated(counts, what)
    f, counts = _prepare_folds(torch.tensor([[0], [1], [1], [0]], dtype=torch.int32), 4, torch.tensor([1.0, 0.0, 2.0, 3.0]), CPU, what)
    assert counts.tolist() == [2, 1]
    for bad in (np.zeros(5, dtype=np.int64), np.zeros((6, 2), dtype=np.int64), np.zeros((1, 6), dtype=np.int64)):
        with pytest.raises(ValueError, match="kfold_scores.*shape"):
            _prepare_folds(bad, 6, None, CPU, what)
    with pytest.raises(ValueError, match="integer"):
        _prepare_folds(np.zeros(6), 6, None, CPU, what)
    with pytest.raises(ValueError, match="row 4 has fold -1"):
        _prepare_folds(np.array([0, 1, 0, 1, -1, -3]), 6, None, CPU, what)
    # an empty fold: a label that never occurs, or one whose rows all have weight 0
    _, counts = _prepare_folds(np.array([0, 3, 0, 3, 1, 1]), 6, None, CPU, what)
    with pytest.raises(ValueError, match="fold 2 has no row of positive weight"):
        _require_folds_populated(counts, what)
    _, counts = _prepare_folds(np.array([0, 1, 0, 1]), 4, torch.tensor([1.0, 0.0, 2.0, 0.0]), CPU, what)
    with pytest.raises(ValueError, match="fold 1 has no row of positive weight"):
        _require_folds_populated(counts, what)
    _, counts = _prepare_folds(np.zeros(0, dtype=np.int64), 0, None, CPU, what)
    with pytest.raises(ValueError, match="kfold_scores"):
        _require_folds_populated(counts, what)


class _FakeHost:
    """the attributes the surface's validation reads, on the host: nothing can be launched through it"""
    _distributed, _pg = False, None
    weights = None

    def __init__(self, n, d, D):
        self.X, self.y = torch.zeros((n, d), dtype=torch.float64), torch.zeros((n, D), dtype=torch.float64)
        self._stats = torch.zeros(4, dtype=torch.float64)

    def predict_f_device(self, X):
        raise AssertionError("validation must raise before the posterior is asked for")


def test_surface_methods_validate_before_any_gpu_call():
    import asvgp_amd as A
    from asvgp_amd.gpr import _GPModelSurface

    class Fake(_FakeHost, _GPModelSurface):
        pass

    class Fake1d(_FakeHost, A.GPR_1d):
        def __init__(self, n):
            _FakeHost.__init__(self, n, 1, 1)

    m = Fake(8, 1, 1)
    X, Y = np.full((5, 1), 0.5), np.zeros((5, 1))
    for name, args in (("score", ((X, Y),)), ("predict_log_density_device", ((X, Y),)), ("predict_y_device", (X,))):
        for bad, word in ((-np.ones(5), "row 0"), (np.array([1, 1, np.nan, 1, 1.0]), "row 2"), (np.ones(4), "shape")):
            with pytest.raises(ValueError, match=word):
                getattr(m, name)(*args, weights=bad)
        with pytest.raises(ValueError, match="Xnew"):
            getattr(m, name)(*(((np.zeros((5, 2)), Y),) if name != "predict_y_device" else (np.zeros((5, 2)),)))
    for name, args in (("set_weights", (np.ones(8),)), ("kfold_scores", (np.zeros(8, dtype=np.int64),))):
        with pytest.raises(NotImplementedError, match=name):
            getattr(m, name)(*args)
    # GPR_1d: the fused overrides validate the same way, and the fold checks come before the twin is built or a pass is launched
    g = Fake1d(8)
    with pytest.raises(ValueError, match="row 1"):
        g.score((X, Y), weights=np.array([1, -2.0, 1, 1, 1]))
    with pytest.raises(ValueError, match="row 1"):
        g.predict_log_density_device((X, Y), weights=np.array([1, -2.0, 1, 1, 1]))
    with pytest.raises(ValueError, match="shape"):
        g.kfold_scores(np.zeros(7, dtype=np.int64))
    with pytest.raises(ValueError, match="row 3 has fold -2"):
        g.kfold_scores(np.array([0, 1, 0, -2, 1, 0, 1, 0]))
    with pytest.raises(ValueError, match="fold 1 has no row"):
        g.kfold_scores(np.array([0, 2, 0, 2, 0, 2, 0, 2]))
    with pytest.raises(ValueError, match="built without weights"):
        g.set_weights(np.ones(8))


def test_score_dict_derived_quantities():
    from asvgp_amd.gpr import _score_dict
    d = _score_dict(4.0, -6.0, 8.0, 10.0, 2)
    assert d == dict(n=4.0, log_density=-6.0, sq_err=8.0, chi2=10.0, nlpd=1.5, rmse=1.0, mean_chi2=1.25)
    e = _score_dict(0.0, 0.0, 0.0, 0.0, 1)
    assert e["n"] == 0.0 and all(math.isnan(e[k]) for k in ("nlpd", "rmse", "mean_chi2"))
