"""CPU: the full-posterior-covariance entry points (asvgp_posterior_cov_prepare_1d, asvgp_predict_cov_1d) are exported with
prototypes, and their argument checks fail loudly on the host, before anything is launched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from asvgp_amd import build, _lib
    build.build(verbose=False)
    return _lib.get_lib()


NAMES = ("asvgp_posterior_cov_prepare_1d", "asvgp_predict_cov_1d", "asvgp_posterior_cov_workspace_bytes")


def test_symbols_exported_with_prototypes(lib):
    from asvgp_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n)
        assert n in _lib.SIGNATURES
        assert getattr(lib, n).argtypes is not None


def test_workspace_bytes(lib):
    for M, k, D in ((16, 1, 1), (257, 3, 3), (2048, 4, 1)):
        cov = lib.asvgp_posterior_cov_workspace_bytes(M, k, D)
        assert cov > lib.asvgp_elbo_workspace_bytes(M, k, D)      # an ELBO workspace of its own, plus the dense-W scratch
    assert lib.asvgp_posterior_cov_workspace_bytes(16, 7, 1) == 0
    assert lib.asvgp_posterior_cov_workspace_bytes(0, 4, 1) == 0


def _err(lib):
    return lib.asvgp_last_error_string().decode()


FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: every call below is refused on the host


def _cov(lib, x1=FAKE, n1=10, x2=FAKE, n2=10, mesh=FAKE, n_mesh=14, order=3, M=16, Wd=FAKE, kind=1, cov=FAKE, ldc=10):
    return lib.asvgp_predict_cov_1d(None, x1, n1, x2, n2, mesh, n_mesh, 0.1, order, M, Wd, kind, 1.0, 0.5, cov, ldc, None)


def test_predict_cov_argument_checks(lib):
    for kw in ({"x1": None}, {"x2": None}, {"mesh": None}, {"Wd": None}, {"cov": None}, {"n1": -1}, {"n2": -1},
               {"ldc": 9}, {"n_mesh": 15}):
        assert _cov(lib, **kw) == -1, kw
        assert "predict_cov_1d" in _err(lib)
    assert _cov(lib, order=7, n_mesh=10) == -2
    assert "predict_cov_1d" in _err(lib) and "order 7" in _err(lib)
    assert _cov(lib, kind=3) == -2
    assert _cov(lib, M=30000, n_mesh=29998) == -2            # a row of W_dense larger than the kernel's LDS plan
    assert "predict_cov_1d" in _err(lib)
    assert _cov(lib, n1=0) == 0 and _cov(lib, n2=0, ldc=0) == 0   # nothing to do: no launch


def _prep(lib, stats=FAKE, S=FAKE, M=16, k=3, D=1, alpha=FAKE, W=FAKE, Wd=FAKE, info=FAKE, ws=FAKE, wsb=None):
    if wsb is None:
        wsb = lib.asvgp_posterior_cov_workspace_bytes(M, k if 1 <= k <= 6 else 1, D)
    return lib.asvgp_posterior_cov_prepare_1d(None, stats, S, 1, 1.0, 0.5, 0.1, M, k, D, alpha, W, Wd, info, ws, wsb, None)


def test_prepare_argument_checks(lib):
    for kw in ({"stats": None}, {"S": None}, {"alpha": None}, {"W": None}, {"Wd": None}, {"info": None}, {"M": 0}, {"D": 0}):
        assert _prep(lib, **kw) == -1, kw
        assert "posterior_cov_prepare_1d" in _err(lib)
    assert _prep(lib, k=7) == -2
    assert "posterior_cov_prepare_1d" in _err(lib)
    # an ELBO-sized workspace is not enough
    assert _prep(lib, wsb=lib.asvgp_elbo_workspace_bytes(16, 3, 1)) == -4
    assert "posterior_cov_prepare_1d" in _err(lib) and "workspace" in _err(lib)
