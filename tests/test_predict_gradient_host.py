"""CPU: the posterior-gradient entry points (asvgp_predict_deriv_1d, asvgp_predict_cov_deriv_1d, asvgp_predict_grad_kron2d) are
exported with prototypes, and their argument checks fail loudly on the host, before anything is launched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from asvgp_amd import build, _lib
    build.build(verbose=False)
    return _lib.get_lib()


NAMES = ("asvgp_predict_deriv_1d", "asvgp_predict_cov_deriv_1d", "asvgp_predict_grad_kron2d")


def test_symbols_exported_with_prototypes(lib):
    from asvgp_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n)
        assert n in _lib.SIGNATURES
        assert getattr(lib, n).argtypes is not None


def _err(lib):
    return lib.asvgp_last_error_string().decode()


FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: every call below is refused on the host (or has nothing to do)
ODD = ctypes.c_void_p(0x1008)    # 8-byte but not 16-byte aligned


def _deriv(lib, x=FAKE, n=10, mesh=FAKE, n_mesh=14, order=3, M=16, alpha=FAKE, W=FAKE, kind=1, D=1, mean=FAKE, var=FAKE):
    return lib.asvgp_predict_deriv_1d(None, x, n, mesh, n_mesh, 0.1, order, M, alpha, W, kind, 1.0, 0.5, D, mean, var, None)


def test_predict_deriv_argument_checks(lib):
    for kw in ({"x": None}, {"mesh": None}, {"alpha": None}, {"W": None}, {"mean": None}, {"var": None}, {"n": -1}, {"D": 0},
               {"n_mesh": 15}):
        assert _deriv(lib, **kw) == -1, kw
        assert "predict_deriv_1d" in _err(lib)
    assert _deriv(lib, order=7, n_mesh=10) == -2
    assert "predict_deriv_1d" in _err(lib) and "order 7" in _err(lib)
    assert _deriv(lib, order=0, n_mesh=17) == -2
    for kind in (0, 3, -1):
        assert _deriv(lib, kind=kind) == -2
        assert "predict_deriv_1d" in _err(lib) and "mean-square derivative" in _err(lib)
    assert _deriv(lib, n=0) == 0                              # nothing to do: no launch


def _cov(lib, x1=FAKE, n1=10, x2=FAKE, n2=10, mesh=FAKE, n_mesh=14, order=3, M=16, Wd=FAKE, kind=1, p=1, q=1, cov=FAKE, ldc=10):
    return lib.asvgp_predict_cov_deriv_1d(None, x1, n1, x2, n2, mesh, n_mesh, 0.1, order, M, Wd, kind, 1.0, 0.5, p, q, cov, ldc, None)


def test_predict_cov_deriv_argument_checks(lib):
    for kw in ({"x1": None}, {"x2": None}, {"mesh": None}, {"Wd": None}, {"cov": None}, {"n1": -1}, {"n2": -1}, {"ldc": 9},
               {"n_mesh": 15}, {"p": 2}, {"q": -1}, {"p": -1, "q": 0}):
        assert _cov(lib, **kw) == -1, kw
        assert "predict_cov_deriv_1d" in _err(lib)
    assert _cov(lib, order=7, n_mesh=10) == -2
    assert "predict_cov_deriv_1d" in _err(lib) and "order 7" in _err(lib)
    assert _cov(lib, kind=3) == -2
    for p, q in ((1, 0), (0, 1), (1, 1)):
        assert _cov(lib, kind=0, p=p, q=q) == -2
        assert "predict_cov_deriv_1d" in _err(lib) and "Matern-1/2" in _err(lib)
    assert _cov(lib, kind=0, p=0, q=0, n1=0) == 0             # no derivative asked for: Matern-1/2 is fine
    assert _cov(lib, M=30000, n_mesh=29998) == -2             # a row of W_dense larger than the kernel's LDS plan
    assert _cov(lib, n1=0) == 0 and _cov(lib, n2=0, ldc=0) == 0


# 60 x 10 grid, k = 3: bandwidth 33, Bb = 64, M_tot = 600; a consistent twisted layout (kronecker.twisted_layout(600, 33, True))
M1, M2, K, BB = 60, 10, 3, 64


def _grad(lib, X=FAKE, n=10, mesh1=FAKE, n_mesh1=M1 - K + 1, m1=M1, mesh2=FAKE, n_mesh2=M2 - K + 1, m2=M2, order=K, alpha=FAKE,
          S1=FAKE, S2=FAKE, SigD=FAKE, SigS=FAKE, Bb=BB, twisted=0, lay=None, kind1=1, kind2=2, mean2=FAKE, cov3=FAKE):
    if lay is None:
        from asvgp_amd.kronecker import twisted_layout
        L = twisted_layout(m1 * m2, order * m2 + order, True) if twisted else None
        lay = (L["nb"], L["top_end"], L["padt"], L["padb"]) if L else (0, 0, 0, 0)
    return lib.asvgp_predict_grad_kron2d(X, n, mesh1, n_mesh1, 0.02, m1, mesh2, n_mesh2, 0.1, m2, order, alpha, S1, S2, SigD, SigS, Bb,
                                         twisted, *lay, kind1, 1.0, 0.3, kind2, 0.8, 0.5, mean2, cov3, None)


def test_predict_grad_kron2d_argument_checks(lib):
    assert _grad(lib, n=0) == 0 and _grad(lib, n=0, twisted=1) == 0      # consistent arguments, nothing to do: no launch
    for kw in ({"X": None}, {"mesh1": None}, {"mesh2": None}, {"alpha": None}, {"S1": None}, {"S2": None}, {"SigD": None},
               {"mean2": None}, {"cov3": None}, {"n": -1}, {"n_mesh1": M1 - K}, {"n_mesh2": M2}, {"twisted": 2}, {"SigS": None},
               {"Bb": K * M2 + K - 1}, {"X": ODD}):
        assert _grad(lib, **kw) == -1, kw
        assert "predict_grad_kron2d" in _err(lib)
    assert "aligned" in (_grad(lib, X=ODD), _err(lib))[1]
    # an inconsistent twisted layout (as twist_ok in kron.hip)
    from asvgp_amd.kronecker import twisted_layout
    L = twisted_layout(M1 * M2, K * M2 + K, True)
    for bad in ((L["nb"], L["top_end"] + 1, L["padt"], L["padb"]), (1, L["top_end"], L["padt"], L["padb"]),
                (L["nb"], L["top_end"], L["padt"] + 1, L["padb"])):
        assert _grad(lib, twisted=1, lay=bad) == -1, bad
        assert "predict_grad_kron2d" in _err(lib) and "layout" in _err(lib)
    assert _grad(lib, order=7, n_mesh1=M1 - 6, n_mesh2=M2 - 6, Bb=128) == -2
    assert "predict_grad_kron2d" in _err(lib) and "order 7" in _err(lib)
    for k1, k2 in ((0, 1), (2, 0), (3, 1), (1, -1)):
        assert _grad(lib, kind1=k1, kind2=k2) == -2
        assert "predict_grad_kron2d" in _err(lib) and "mean-square derivative" in _err(lib)
