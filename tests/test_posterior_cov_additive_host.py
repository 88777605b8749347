"""CPU: the additive model's full-posterior-covariance entry point (asvgp_predict_cov_additive) is exported with a prototype, and its
argument checks fail loudly on the host, before anything is launched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from asvgp_amd import build, _lib
    build.build(verbose=False)
    return _lib.get_lib()


NAME = "asvgp_predict_cov_additive"
BAD_ARG, UNSUPPORTED = -1, -2
MAX_D = 16


def test_symbol_exported_with_prototype(lib):
    from asvgp_amd import _lib
    assert hasattr(lib, NAME)
    assert NAME in _lib.SIGNATURES
    assert getattr(lib, NAME).argtypes is not None


def _err(lib):
    return lib.asvgp_last_error_string().decode()


FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: every call below is refused on the host


def _arr(t, vals):
    return None if vals is None else (t * len(vals))(*vals)


def _cov(lib, x1=FAKE, n1=10, x2=FAKE, n2=10, d=3, meshes=FAKE, n_mesh=(14, 11, 9), delta=(0.1, 0.2, 0.3), m=(16, 13, 11), order=3,
         kind=(0, 1, 2), variance=(1.0, 0.7, 0.4), lengthscale=(0.5, 0.3, 0.2), W=FAKE, cov=FAKE, ldc=10):
    return lib.asvgp_predict_cov_additive(None, x1, n1, x2, n2, d, meshes, _arr(ctypes.c_int64, n_mesh), _arr(ctypes.c_double, delta),
                                          _arr(ctypes.c_int64, m), order, _arr(ctypes.c_int, kind), _arr(ctypes.c_double, variance),
                                          _arr(ctypes.c_double, lengthscale), W, cov, ldc, None)


def test_argument_checks(lib):
    for kw in ({"x1": None}, {"x2": None}, {"meshes": None}, {"n_mesh": None}, {"delta": None}, {"m": None}, {"kind": None},
               {"variance": None}, {"lengthscale": None}, {"W": None}, {"cov": None}, {"n1": -1}, {"n2": -1}, {"ldc": 9}, {"d": 0},
               {"d": -2}, {"delta": (0.1, 0.0, 0.3)}, {"delta": (0.1, 0.2, -0.3)}, {"variance": (0.0, 0.7, 0.4)},
               {"variance": (1.0, -0.7, 0.4)}, {"lengthscale": (0.5, 0.3, 0.0)}, {"lengthscale": (-0.5, 0.3, 0.2)},
               {"delta": (float("nan"), 0.2, 0.3)}, {"n_mesh": (15, 11, 9)}, {"n_mesh": (14, 11, 10)}, {"m": (16, 13, 12)}):
        assert _cov(lib, **kw) == BAD_ARG, kw
        assert "predict_cov_additive" in _err(lib)
    assert "dimension 2" in (_cov(lib, n_mesh=(14, 11, 10)) and _err(lib))
    assert _cov(lib, order=7, n_mesh=(10, 7, 5)) == UNSUPPORTED
    assert "order 7" in _err(lib)
    assert _cov(lib, order=0, n_mesh=(17, 14, 12)) == UNSUPPORTED
    assert _cov(lib, kind=(0, 3, 2)) == UNSUPPORTED
    assert "dimension 1" in _err(lib)
    assert _cov(lib, kind=(0, 1, -1)) == UNSUPPORTED


def test_dimension_limit(lib):
    def dims(d):
        return dict(d=d, n_mesh=(6,) * d, delta=(0.2,) * d, m=(8,) * d, kind=(1,) * d, variance=(1.0,) * d, lengthscale=(0.3,) * d)
    assert _cov(lib, n1=0, **dims(MAX_D)) == 0                          # d = 16 accepted (nothing to do: no launch)
    assert _cov(lib, **dims(MAX_D + 1)) == UNSUPPORTED
    assert "d = 17" in _err(lib)
    assert _cov(lib, n1=0, **dims(1)) == 0


def test_lds_limit(lib):
    # 156 KiB of LDS = 19 968 doubles: M_tot = 19 968 fits, one more does not
    def dims(ms):
        d = len(ms)
        return dict(d=d, n_mesh=tuple(x - 2 for x in ms), delta=(0.1,) * d, m=tuple(ms), order=3, kind=(1,) * d, variance=(1.0,) * d,
                    lengthscale=(0.3,) * d)
    assert _cov(lib, n1=0, **dims((9984, 9984))) == 0
    assert _cov(lib, **dims((9984, 9985))) == UNSUPPORTED
    assert "LDS" in _err(lib) and "19969" in _err(lib)
    assert _cov(lib, **dims((2 ** 62, 16))) == UNSUPPORTED              # one m_i alone beyond the plan: no overflow in the sum
    assert "LDS" in _err(lib)
    assert _cov(lib, n1=0, **dims((256,) * 8)) == 0                     # the probe's M_tot = 2048
    assert _cov(lib, n2=0, ldc=0) == 0
