"""CPU: the additive model's components / gradient entry point (asvgp_predict_components_additive) is exported with a prototype, and its
argument checks fail loudly on the host, before anything is launched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from asvgp_amd import build, _lib
    build.build(verbose=False)
    return _lib.get_lib()


NAME = "asvgp_predict_components_additive"
BAD_ARG, UNSUPPORTED = -1, -2
MAX_D = 16


def test_symbol_exported_with_prototype(lib):
    from asvgp_amd import _lib
    assert hasattr(lib, NAME)
    assert NAME in _lib.SIGNATURES
    assert getattr(lib, NAME).argtypes is not None


def _err(lib):
    return lib.asvgp_last_error_string().decode()


FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: every call below is refused on the host (or has nothing to do)


def _arr(t, vals):
    return None if vals is None else (t * len(vals))(*vals)


def _comp(lib, X=FAKE, n=10, d=3, meshes=FAKE, n_mesh=(14, 11, 9), delta=(0.1, 0.2, 0.3), m=(16, 13, 11), order=3, kind=(0, 1, 2),
          variance=(1.0, 0.7, 0.4), lengthscale=(0.5, 0.3, 0.2), deriv=0, alpha=FAKE, W=FAKE, mean=FAKE, cov=FAKE):
    return lib.asvgp_predict_components_additive(None, X, n, d, meshes, _arr(ctypes.c_int64, n_mesh), _arr(ctypes.c_double, delta),
                                                 _arr(ctypes.c_int64, m), order, _arr(ctypes.c_int, kind), _arr(ctypes.c_double, variance),
                                                 _arr(ctypes.c_double, lengthscale), deriv, alpha, W, mean, cov, None)


def test_argument_checks(lib):
    for kw in ({"X": None}, {"meshes": None}, {"n_mesh": None}, {"delta": None}, {"m": None}, {"kind": None}, {"variance": None},
               {"lengthscale": None}, {"alpha": None}, {"W": None}, {"mean": None}, {"cov": None}, {"n": -1}, {"d": 0}, {"d": -2},
               {"deriv": 2}, {"deriv": -1}, {"delta": (0.1, 0.0, 0.3)}, {"variance": (1.0, -0.7, 0.4)}, {"lengthscale": (0.5, 0.3, 0.0)},
               {"delta": (float("nan"), 0.2, 0.3)}, {"n_mesh": (15, 11, 9)}, {"n_mesh": (14, 11, 10)}, {"m": (16, 13, 12)}):
        assert _comp(lib, **kw) == BAD_ARG, kw
        assert "predict_components_additive" in _err(lib)
    assert "dimension 2" in (_comp(lib, n_mesh=(14, 11, 10)) and _err(lib))
    assert _comp(lib, order=7, n_mesh=(10, 7, 5)) == UNSUPPORTED
    assert "predict_components_additive" in _err(lib) and "order 7" in _err(lib)
    assert _comp(lib, order=0, n_mesh=(17, 14, 12)) == UNSUPPORTED
    assert _comp(lib, kind=(0, 3, 2)) == UNSUPPORTED
    assert "predict_components_additive" in _err(lib) and "dimension 1" in _err(lib)
    assert _comp(lib, kind=(0, 1, -1)) == UNSUPPORTED


def test_matern12_gradient_refused(lib):
    for kind, dim in (((0, 1, 2), 0), ((1, 2, 0), 2), ((2, 0, 1), 1)):
        assert _comp(lib, kind=kind, deriv=1) == UNSUPPORTED
        assert "predict_components_additive" in _err(lib) and "Matern-1/2" in _err(lib) and "dimension %d" % dim in _err(lib)
        assert _comp(lib, kind=kind, deriv=1, n=0) == UNSUPPORTED            # refused before the empty batch returns
        assert _comp(lib, kind=kind, deriv=0, n=0) == 0                      # the components of the same dimensions are fine
    assert _comp(lib, kind=(1, 2, 1), deriv=1, n=0) == 0


def test_dimension_limit(lib):
    def dims(d):
        return dict(d=d, n_mesh=(6,) * d, delta=(0.2,) * d, m=(8,) * d, kind=(1,) * d, variance=(1.0,) * d, lengthscale=(0.3,) * d)
    assert _comp(lib, n=0, **dims(MAX_D)) == 0                          # d = 16 accepted (nothing to do: no launch)
    assert _comp(lib, n=0, deriv=1, **dims(MAX_D)) == 0
    assert _comp(lib, **dims(MAX_D + 1)) == UNSUPPORTED
    assert "predict_components_additive" in _err(lib) and "d = 17" in _err(lib)
    assert _comp(lib, n=0, **dims(1)) == 0


def test_no_lds_limit(lib):
    # W is read in place: an M_tot far beyond the cross-covariance kernel's 156 KiB row (19 968 doubles) is accepted
    def dims(ms):
        d = len(ms)
        return dict(d=d, n_mesh=tuple(x - 2 for x in ms), delta=(0.1,) * d, m=tuple(ms), order=3, kind=(1,) * d, variance=(1.0,) * d,
                    lengthscale=(0.3,) * d)
    assert _comp(lib, n=0, **dims((9984, 9985))) == 0
    assert _comp(lib, n=0, **dims((40_000, 40_000, 40_000))) == 0
    assert _comp(lib, n=0, **dims((256,) * 8)) == 0                     # the probe's M_tot = 2048
    assert _comp(lib, **dims((2 ** 62, 16))) == UNSUPPORTED              # M_tot beyond an int: refused without overflow
    assert "predict_components_additive" in _err(lib) and "M_tot" in _err(lib)
    assert _comp(lib, **dims((2 ** 30, 2 ** 30))) == UNSUPPORTED
    assert _comp(lib, n=0) == 0
