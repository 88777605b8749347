"""CPU (-m "not gpu") side of the additive model's cross-block kernel, asvgp_phi_cross_2d (csrc/additive.hip):
the long-double reference the GPU tests (tests/test_additive_cross.py) are judged by, against the scipy sparse product it
restates; the argument checks of the entry, which return before any device call; and the workspace rule."""
import ctypes
import types

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import asvgp_oracle as O

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2


def cross_basis(order, a, b, m):
    """what additive_cross_block_extended needs of a basis; O.Basis refuses B4 below m = 12 and builds every static band"""
    mesh, delta = O.make_mesh(a, b, m, order)
    return types.SimpleNamespace(order=order, a=a, b=b, m=m, mesh=mesh, delta=float(delta))


@pytest.fixture(scope="session")
def lib():
    from asvgp_amd import build, _lib
    build.build(verbose=False)
    return _lib.get_lib()


@pytest.mark.parametrize("m_i,m_j", [(1, 4), (17, 20)])                      # m = order + (m_i, m_j): one cell x four cells, and a wider pair
@pytest.mark.parametrize("order", [1, 2, 3, 4, 5, 6])
def test_extended_cross_block_equals_the_sparse_product(order, m_i, m_j):
    """The reference of the GPU tests is Phi_i Phi_j^T: equal to the scipy product of the two design matrices to 1e-13 of the
    largest entry (N eps = 7e-13 is the fp64 product's own worst case at this N; it is far inside that), with the counts of the
    product's pattern, and a partition of unity.  (0, 1) is an exact fp64 mesh, (-3.5, 10.5) the float32-linspace one."""
    N = 3001
    bi, bj = cross_basis(order, 0, 1, order + m_i), cross_basis(order, -3.5, 10.5, order + m_j)
    assert bj.mesh.shape[0] == m_j + 1 and (m_j == 4 or np.any(np.diff(bj.mesh) != bj.delta))    # 20 cells: not exactly delta wide
    rng = np.random.default_rng(100 * order + m_i)
    xi, xj = rng.uniform(0, 1, N), rng.uniform(-3.5, 10.5, N)
    nk = bj.mesh.shape[0]
    xj[:nk] = bj.mesh                                            # every knot of j, both ends included
    xi[:nk] = rng.permutation(np.resize(bi.mesh, nk))            # ... against knots and ends of i
    xi[nk:nk + 4] = [0.0, 1.0, 0.0, 1.0]
    xj[nk:nk + 4] = [-3.5, -3.5, 10.5, 10.5]                     # the four corners
    C, cnt = O.additive_cross_block_extended(bi, bj, xi, xj)
    assert C.dtype == np.longdouble and C.shape == (bi.m, bj.m) and cnt.shape == C.shape
    Pi = O.evaluate_basis(bi.mesh, bi.delta, order, bi.m, xi)
    Pj = O.evaluate_basis(bj.mesh, bj.delta, order, bj.m, xj)
    ref = (Pi @ Pj.T).toarray()
    assert float(np.max(np.abs(C - ref))) <= 1e-13 * np.max(np.abs(ref))
    ones = []
    for bs, x in ((bi, xi), (bj, xj)):                           # the pattern of the product: a piece that is exactly 0 counts too
        rows, cols, data = O.evaluate_basis_coo(bs.mesh, bs.delta, order, bs.m, x)
        ones.append(sp.csr_matrix((np.ones(data.shape[0], dtype=np.int64), (rows, cols)), shape=(bs.m, N)))
    assert np.array_equal(cnt, (ones[0] @ ones[1].T).toarray())
    assert cnt.sum() == (order + 1) ** 2 * N and (C[cnt == 0] == 0).all()
    assert abs(float(C.sum() - N)) <= 1e-15 * N
    C0, cnt0 = O.additive_cross_block_extended(bi, bj, xi[:0], xj[:0])
    assert C0.shape == C.shape and not C0.any() and not cnt0.any()


def _cross_args(**kw):
    """a consistent order-3 20 x 17 call with dummy non-null pointers; every check under test returns before they are read"""
    p = ctypes.c_void_p(8)
    a = dict(x_i=p, x_j=p, N=10, mesh_i=p, n_mesh_i=18, delta_i=0.1, m_i=20, mesh_j=p, n_mesh_j=15, delta_j=0.2, m_j=17,
             order=3, out=p, workspace=p, workspace_bytes=1 << 30, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return tuple(a.values())


BAD = [dict(x_i=None), dict(x_j=None), dict(mesh_i=None), dict(mesh_j=None), dict(out=None), dict(N=-1),
       dict(delta_i=0.0), dict(delta_i=-0.1), dict(delta_i=float("nan")),
       dict(delta_j=0.0), dict(delta_j=-0.1), dict(delta_j=float("nan")),
       dict(n_mesh_i=17), dict(n_mesh_i=19), dict(n_mesh_j=14), dict(n_mesh_j=16), dict(m_i=21), dict(m_j=16),
       dict(n_mesh_i=1, m_i=3), dict(n_mesh_j=1, m_j=3), dict(n_mesh_i=0, m_i=2), dict(n_mesh_j=-1, m_j=1)]


def test_cross_entry_argument_checks_fail_loudly(lib):
    for kw in BAD:
        assert lib.asvgp_phi_cross_2d(*_cross_args(**kw)) == BAD_ARG, kw
        assert b"phi_cross_2d" in lib.asvgp_last_error_string(), kw
    for order in (0, 7):                                          # n_mesh = m - order + 1 holds: the order itself is refused
        kw = dict(order=order, n_mesh_i=20 - order + 1, n_mesh_j=17 - order + 1)
        assert lib.asvgp_phi_cross_2d(*_cross_args(**kw)) == UNSUPPORTED, kw
        msg = lib.asvgp_last_error_string()
        assert b"phi_cross_2d" in msg and str(order).encode() in msg
    assert lib.asvgp_status_name(BAD_ARG) == b"ASVGP_ERR_BAD_ARG" and lib.asvgp_status_name(UNSUPPORTED) == b"ASVGP_ERR_UNSUPPORTED"


def test_cross_workspace_bytes(lib):
    """256 partial images where the block can take the LDS path at some order, 8 bytes where it cannot at any."""
    for m_i, m_j in ((0, 5), (5, 0), (-1, 5), (0, 0)):
        assert lib.asvgp_phi_cross_workspace_bytes(m_i, m_j) == 0
    for m_i, m_j in ((50, 40), (147, 137), (142, 141), (1, 1)):
        assert lib.asvgp_phi_cross_workspace_bytes(m_i, m_j) == 256 * 8 * m_i * m_j
        assert lib.asvgp_phi_cross_workspace_bytes(m_j, m_i) == 256 * 8 * m_i * m_j
    for m_i, m_j in ((150, 140), (142, 142)):
        assert lib.asvgp_phi_cross_workspace_bytes(m_i, m_j) == 8
        assert lib.asvgp_phi_cross_workspace_bytes(m_j, m_i) == 8
