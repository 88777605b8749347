"""CPU: the 2-D full-posterior-covariance entry points (asvgp_kron_dense_inverse, asvgp_predict_cov_kron2d) are exported with
prototypes, and their argument checks fail loudly on the host, before anything is launched."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from asvgp_amd import build, _lib
    build.build(verbose=False)
    return _lib.get_lib()


NAMES = ("asvgp_kron_dense_inverse", "asvgp_predict_cov_kron2d")
BAD_ARG, UNSUPPORTED = -1, -2


def test_symbols_exported_with_prototypes(lib):
    from asvgp_amd import _lib
    for n in NAMES:
        assert hasattr(lib, n)
        assert n in _lib.SIGNATURES
        assert getattr(lib, n).argtypes is not None


def _err(lib):
    return lib.asvgp_last_error_string().decode()


FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: every call below is refused on the host


def _cov(lib, x1=FAKE, n1=10, x2=FAKE, n2=10, mesh1=FAKE, nm1=14, d1=0.1, m1=16, mesh2=FAKE, nm2=11, d2=0.2, m2=13, order=3,
         Sig=FAKE, K1=FAKE, K2=FAKE, kind1=1, v1=1.0, l1=0.5, kind2=2, v2=0.7, l2=0.3, cov=FAKE, ldc=10):
    return lib.asvgp_predict_cov_kron2d(None, x1, n1, x2, n2, mesh1, nm1, d1, m1, mesh2, nm2, d2, m2, order, Sig, K1, K2,
                                        kind1, v1, l1, kind2, v2, l2, cov, ldc, None)


def test_predict_cov_argument_checks(lib):
    for kw in ({"x1": None}, {"x2": None}, {"mesh1": None}, {"mesh2": None}, {"Sig": None}, {"K1": None}, {"K2": None},
               {"cov": None}, {"n1": -1}, {"n2": -1}, {"ldc": 9}, {"d1": 0.0}, {"d2": -1.0}, {"v1": 0.0}, {"v2": -2.0},
               {"l1": 0.0}, {"l2": -0.1}, {"nm1": 15}, {"nm2": 12}):
        assert _cov(lib, **kw) == BAD_ARG, kw
        assert "predict_cov_kron2d" in _err(lib)
    assert _cov(lib, order=7, nm1=10, nm2=7) == UNSUPPORTED
    assert "order 7" in _err(lib)
    assert _cov(lib, kind1=3) == UNSUPPORTED
    assert _cov(lib, kind2=-1) == UNSUPPORTED
    assert _cov(lib, m1=160, nm1=158, m2=130, nm2=128) == UNSUPPORTED     # M_tot = 20 800: a row of Sigma beyond the LDS plan
    assert "LDS" in _err(lib)
    assert _cov(lib, m1=128, nm1=126, m2=128, nm2=126, n1=0) == 0          # config 4's M_tot fits; nothing to do: no launch
    assert _cov(lib, n2=0, ldc=0) == 0


def _inv(lib, G=FAKE, SigD=FAKE, SigS=FAKE, M=1000, Bb=128, tw=0, nb=8, top_end=0, padt=0, padb=0, Sig=FAKE):
    return lib.asvgp_kron_dense_inverse(G, SigD, SigS, M, Bb, tw, nb, top_end, padt, padb, Sig, None)


def _twist(M, Bb):
    """kronecker.twisted_layout's scalars, forced on"""
    from asvgp_amd.kronecker import twisted_layout
    lay = twisted_layout(M, Bb, True)
    return dict(tw=1, nb=lay["nb"], top_end=lay["top_end"], padt=lay["padt"], padb=lay["padb"])


def test_dense_inverse_argument_checks(lib):
    for kw in ({"SigD": None}, {"Sig": None}, {"G": None}, {"SigS": None}, {"M": 0}, {"Bb": 0}, {"Bb": 48}, {"Bb": 100}, {"tw": 2},
               {"nb": 7}, {"nb": 9}, {"padt": 1}, {"top_end": 5}):
        assert _inv(lib, **kw) == BAD_ARG, kw
        assert "kron_dense_inverse" in _err(lib)
    assert "multiple of 32" in (_inv(lib, Bb=48) and _err(lib))
    tw = _twist(1000, 100)
    assert tw["nb"] >= 3
    for key, delta in (("nb", 1), ("top_end", 1), ("padt", 1), ("padb", 1), ("padb", -tw["padb"] - 1)):
        bad = dict(tw, **{key: tw[key] + delta})
        assert _inv(lib, **bad) == BAD_ARG, (key, delta)
        assert "inconsistent twisted layout" in _err(lib)
    bad = dict(tw, Bb=96)
    assert _inv(lib, **bad) == BAD_ARG
    assert _inv(lib, **dict(tw, G=None)) == BAD_ARG
