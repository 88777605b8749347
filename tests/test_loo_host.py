"""CPU: the leave-one-out entry points (asvgp_posterior_prepare_loo_1d, asvgp_loo_workspace_bytes, asvgp_loo_1d) are exported with
prototypes, and their argument checks fail loudly on the host, before anything is launched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from asvgp_amd import build, _lib
    build.build(verbose=False)
    return _lib.get_lib()


NAMES = ("asvgp_posterior_prepare_loo_1d", "asvgp_loo_workspace_bytes", "asvgp_loo_1d")


def test_symbols_exported_with_prototypes(lib):
    from asvgp_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n)
        assert n in _lib.SIGNATURES
        assert getattr(lib, n).argtypes is not None
    # asvgp_posterior_prepare_1d with one more pointer (Pinv_band) behind W
    base, loo = _lib.SIGNATURES["asvgp_posterior_prepare_1d"], _lib.SIGNATURES["asvgp_posterior_prepare_loo_1d"]
    assert loo[0] is base[0] and loo[1] == base[1][:12] + [ctypes.c_void_p] + base[1][12:]


def _err(lib):
    return lib.asvgp_last_error_string().decode()


FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: every call below is refused on the host (or has nothing to do)
ODD = ctypes.c_void_p(0x1008)    # 8-byte but not 16-byte aligned: accepted like any other


def _loo(lib, x=FAKE, y=FAKE, w=FAKE, N=10, D=1, mesh=FAKE, n_mesh=14, order=3, M=16, alpha=FAKE, W=FAKE, Pinv=FAKE, variance=1.0, noise=0.1,
         mean=FAKE, var=FAKE, logdens=FAKE, scores=FAKE, ws=FAKE, wsb=None):
    if wsb is None:
        wsb = lib.asvgp_loo_workspace_bytes(M, min(max(order, 1), 6), max(D, 1))
    return lib.asvgp_loo_1d(None, x, y, w, N, D, mesh, n_mesh, 0.1, order, M, alpha, W, Pinv, variance, noise, mean, var, logdens, scores,
                            ws, wsb, None)


def test_loo_workspace_bytes(lib):
    assert lib.asvgp_loo_workspace_bytes(16, 3, 1) >= 8 * 4
    assert lib.asvgp_loo_workspace_bytes(16, 3, 1) == lib.asvgp_loo_workspace_bytes(2048, 4, 7)      # workgroup records only
    assert lib.asvgp_loo_workspace_bytes(0, 3, 1) == 0 and lib.asvgp_loo_workspace_bytes(16, 7, 1) == 0
    assert lib.asvgp_loo_workspace_bytes(16, 3, 0) == 0


def test_loo_argument_checks(lib):
    for kw in ({"x": None}, {"y": None}, {"mesh": None}, {"alpha": None}, {"W": None}, {"Pinv": None}, {"N": -1}, {"D": 0}, {"D": -2},
               {"n_mesh": 15}, {"n_mesh": 13}, {"variance": 0.0}, {"variance": -1.0}, {"noise": 0.0}, {"noise": float("nan")},
               {"mean": None, "var": None, "logdens": None, "scores": None}, {"ws": None}):
        rc = _loo(lib, **kw)
        assert rc == (-1 if "ws" not in kw else -4), kw
        assert "loo_1d" in _err(lib)
    assert _loo(lib, order=7, n_mesh=10) == -2
    assert "loo_1d" in _err(lib) and "order 7" in _err(lib)
    assert _loo(lib, order=0, n_mesh=17) == -2
    assert _loo(lib, wsb=lib.asvgp_loo_workspace_bytes(16, 3, 1) - 8) == -4                           # ASVGP_ERR_WORKSPACE
    assert "loo_1d" in _err(lib) and "workspace" in _err(lib)


def test_loo_empty_batch_is_ok(lib):
    # nothing to stream: no launch.  (scores, which an empty batch zeroes on the device, are not asked for here)
    assert _loo(lib, N=0, scores=None) == 0
    assert _loo(lib, N=0, scores=None, x=None, y=None, w=None) == 0
    assert _loo(lib, N=0, scores=None, var=None, logdens=None, mean=ODD) == 0
    # weights are optional: NULL means all ones, so it is not among the required pointers
    assert _loo(lib, N=0, w=None, scores=None) == 0


def _prep(lib, stats=FAKE, S=FAKE, M=16, k=3, D=1, alpha=FAKE, W=FAKE, Pinv=FAKE, info=FAKE, ws=FAKE, wsb=None, v=1.0, l=0.5, s=0.1):
    if wsb is None:
        wsb = lib.asvgp_elbo_workspace_bytes(M, min(max(k, 1), 6), max(D, 1))
    return lib.asvgp_posterior_prepare_loo_1d(None, stats, S, 1, v, l, s, M, k, D, alpha, W, Pinv, info, ws, wsb, None)


def test_posterior_prepare_loo_argument_checks(lib):
    for kw in ({"stats": None}, {"S": None}, {"alpha": None}, {"W": None}, {"Pinv": None}, {"info": None}, {"M": 0}, {"D": 0},
               {"v": 0.0}, {"l": -1.0}, {"s": 0.0}):
        assert _prep(lib, **kw) == -1, kw
        assert "posterior_prepare_loo_1d" in _err(lib)
    assert _prep(lib, k=7) == -2 and "posterior_prepare_loo_1d" in _err(lib)
    assert _prep(lib, ws=None) == -4 and _prep(lib, wsb=8) == -4
    assert "posterior_prepare_loo_1d" in _err(lib)
