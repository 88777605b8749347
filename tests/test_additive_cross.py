"""GPU: asvgp_phi_cross_2d (csrc/additive.hip), the kernel behind every dense off-diagonal block C_ij = Phi_i Phi_j^T of
GPR_additive, called directly through the C-ABI on every branch of its launch (launch_cross) and judged by the long-double
reference O.additive_cross_block_extended (tests/test_additive_cross_host.py pins that one to the scipy product).

Gate (the band gate of test_additive_statistics_elbo_predict_vs_oracle): max |got - ref| <= 1e-12 max |ref|,
got == 0 exactly where no product lands, sum(got) == N to 1e-12 N.  It is not fitted to the kernel: the LDS path rounds each
product once to a multiple of 2^-s0 with s0 >= 48 at every size here, so an entry of `count` products is off by at most
count 2^-49, below 1e-14 of the largest entry even when all points share one cell pair (largest entry ~0.21 N); the L2 path
adds fp64 atomics of positive terms.  An overflow of the 64-bit accumulator or a lost bit of s0 misses the gate by orders of
magnitude.  Each case prints its largest relative error (pytest -s).

out and the whole workspace are NaN before every call unless a test says otherwise: the kernel must overwrite, not add."""
import types

import numpy as np
import pytest
import torch

from oracle import asvgp_oracle as O

pytestmark = pytest.mark.gpu

GATE = 1e-12
OK, ERR_WORKSPACE = 0, -4
KINDS = {0: "Matern12", 1: "Matern32", 2: "Matern52"}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from asvgp_amd import _lib
    return _lib.get_lib()  # must load: no fallback


def cross_basis(order, a, b, m):
    """what the entry and the reference need of a basis (A.B4Spline / O.Basis refuse m < 12; the kernel does not)"""
    mesh, delta = O.make_mesh(a, b, m, order)
    return types.SimpleNamespace(order=order, a=a, b=b, m=m, mesh=mesh, delta=float(delta))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def nan_buffer(n_bytes):
    return torch.full((max(int(n_bytes) // 8, 1),), float("nan"), dtype=torch.float64, device="cuda")


def cross(lib, bi, bj, xi, xj, ws_bytes=None, ws=None, null_x=False):
    """one call on fresh device copies; returns (status, out as m_i x m_j numpy).  ws: a caller-owned workspace, used as it is."""
    from asvgp_amd._lib import stream_ptr
    assert bi.order == bj.order and len(xi) == len(xj)
    N = len(xi)
    dxi, dxj, mi, mj = dev(xi), dev(xj), dev(bi.mesh), dev(bj.mesh)
    if ws_bytes is None:
        ws_bytes = lib.asvgp_phi_cross_workspace_bytes(bi.m, bj.m)
    if ws is None:
        ws = nan_buffer(ws_bytes)
    assert ws.numel() * 8 >= ws_bytes
    out = nan_buffer(8 * bi.m * bj.m)
    st = lib.asvgp_phi_cross_2d(None if null_x else dxi.data_ptr(), None if null_x else dxj.data_ptr(), N, mi.data_ptr(),
                                mi.shape[0], bi.delta, bi.m, mj.data_ptr(), mj.shape[0], bj.delta, bj.m, bi.order,
                                out.data_ptr(), ws.data_ptr(), ws_bytes, stream_ptr())
    torch.cuda.synchronize()
    return st, out.cpu().numpy().reshape(bi.m, bj.m)


def gate(got, ref, cnt, N, what):
    """the module's gate; returns the largest error relative to the largest entry"""
    assert np.isfinite(got).all(), what
    err = float(np.max(np.abs(got.astype(np.longdouble) - ref)) / np.max(np.abs(ref)))
    tot = float(abs(np.sum(got.astype(np.longdouble)) - N)) / N
    print("cross block %s: max rel err %.2e, |sum - N| / N %.2e" % (what, err, tot))
    assert err <= GATE, (what, err)
    assert (got[cnt == 0] == 0).all(), what
    assert tot <= GATE, (what, tot)
    return err


def run_and_gate(lib, bi, bj, xi, xj, what, **kw):
    st, got = cross(lib, bi, bj, xi, xj, **kw)
    assert st == OK, (what, st, lib.asvgp_last_error_string())
    ref, cnt = O.additive_cross_block_extended(bi, bj, xi, xj)
    return gate(got, ref, cnt, len(xi), what), got


def launch_plan(N, E, n_i, n_j):
    """launch_cross's rule, restated: (LDS path?, workgroups G, reduce slices, points per workgroup ppb, fixed-point scale s0)"""
    def ceil_div(a, b):
        return -(-a // b)
    G = min(max(ceil_div(N, 2048), 1), 256)
    ppb = ceil_div(ceil_div(N, G), 1024) * 1024
    s0 = min(50, 62 - (ppb - 1).bit_length())                     # ceil(log2 ppb), ppb >= 1024
    return 8 * (E + n_i + n_j) <= 160 * 1024 - 512, G, 8 if G >= 64 else 1, ppb, s0


# ------------------------------------------------------------------------------------------------ a. every order, smallest shapes
def planted_pairs(rng, bi, bj):
    """(x_i, x_j) pairs on the edges: the four corners, every knot of the j mesh (its ends among them) and one ulp either side of two
    interior knots of it.  The first two are corners, so N = 1 and N = 2 run on nothing else."""
    kn = bj.mesh
    xj = [kn[-1], kn[0], kn[0], kn[-1]] + list(kn)
    for k in (kn[1], kn[-2]):
        xj += [np.nextafter(k, -np.inf), np.nextafter(k, np.inf)]
    xi = [bi.mesh[0], bi.mesh[-1], bi.mesh[0], bi.mesh[-1]] + list(rng.uniform(bi.mesh[0], bi.mesh[-1], len(xj) - 4))
    return np.array(xi), np.array(xj)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("order", [1, 2, 3, 4, 5, 6])
def test_every_order_on_one_cell_and_on_the_edges(lib, order, swap):
    """phi_cross_kernel<1..6, LDS>: a one-cell basis (m = order + 1) on (0, 1) against m = order + 4 on (-3.5, 10.5), either
    one as i (a swap of the two mesh origins or widths shows at once); points on a, b, every knot, and one ulp off two knots;
    N = 1, 2, below and above one workgroup's first sweep (1024), two workgroups (2049), three (4097)."""
    one, four = cross_basis(order, 0, 1, order + 1), cross_basis(order, -3.5, 10.5, order + 4)
    assert one.mesh.shape[0] == 2 and four.mesh.shape[0] == 5
    rng = np.random.default_rng(10 * order + swap)
    p_one, p_four = planted_pairs(rng, one, four)
    worst = 0.0
    for N in (1, 2, 1023, 1025, 2049, 4097):
        x_one, x_four = rng.uniform(0, 1, N), rng.uniform(-3.5, 10.5, N)
        at = rng.permutation(N)[:len(p_one)]                       # (N = 1, 2: the first planted pairs, the corners)
        x_one[at], x_four[at] = p_one[:len(at)], p_four[:len(at)]
        bi, bj, xi, xj = (four, one, x_four, x_one) if swap else (one, four, x_one, x_four)
        assert launch_plan(N, bi.m * bj.m, bi.mesh.shape[0], bj.mesh.shape[0])[:2] == (True, -(-N // 2048))
        err, _ = run_and_gate(lib, bi, bj, xi, xj, "a order %d %dx%d N %d" % (order, bi.m, bj.m, N))
        worst = max(worst, err)
    print("group a order %d swap %d: worst %.2e" % (order, swap, worst))


# ------------------------------------------------------------------------------------------------ b. launch branches by N
def _b_bases():
    return cross_basis(3, 0, 1, 20), cross_basis(3, -1, 2, 17)


#       N        G   reduce slices   ppb   s0 = min(50, 62 - ceil(log2 ppb))
PLAN_B = [(129024, 63, 1, 2048, 50),         # the last one-slice reduce
          (129025, 64, 8, 2048, 50),         # the first 8-way reduce
          (143361, 71, 8, 2048, 50),         # 8 slices of 9 images, the last one ragged (71 = 7 x 9 + 8)
          (524288, 256, 8, 2048, 50),        # G at its cap, every workgroup full
          (524289, 256, 8, 3072, 50),        # ppb 3072: workgroups 171 .. 255 own no points
          (1048576, 256, 8, 4096, 50),       # the last size at s0 = 50
          (1048577, 256, 8, 5120, 49),
          (2097153, 256, 8, 9216, 48)]


@pytest.mark.parametrize("N,G,slices,ppb,s0", PLAN_B)
def test_launch_branches_by_point_count(lib, N, G, slices, ppb, s0):
    """Order 3, 20 x 17 on (0, 1) x (-1, 2), uniform data, at the sizes either side of each branch of launch_cross (PLAN_B, derived
    by hand from the rule and checked against its restatement)."""
    bi, bj = _b_bases()
    assert launch_plan(N, 340, 18, 15) == (True, G, slices, ppb, s0)
    owners = (N - 1) // ppb + 1                                    # workgroups that own points: the rounding of ppb to 1024 idles the rest
    assert owners == {524289: 171, 1048577: 205, 2097153: 228}.get(N, G)
    rng = np.random.default_rng(N)
    run_and_gate(lib, bi, bj, rng.uniform(0, 1, N), rng.uniform(-1, 2, N), "b uniform N %d (G %d ppb %d s0 %d)" % (N, G, ppb, s0))


@pytest.mark.parametrize("N,G,slices,ppb,s0", PLAN_B[-3:])
def test_every_point_in_one_cell_pair(lib, N, G, slices, ppb, s0):
    """The least headroom of the 64-bit LDS accumulator and the most contention on its adds: all N points inside
    mesh_i[3] .. mesh_i[4] x mesh_j[5] .. mesh_j[6], so each workgroup adds ppb products into each of 16 entries
    (the largest holds ~0.21 ppb 2^s0 < 2^62)."""
    bi, bj = _b_bases()
    assert launch_plan(N, 340, 18, 15) == (True, G, slices, ppb, s0)
    rng = np.random.default_rng(N + 1)
    xi, xj = rng.uniform(bi.mesh[3], bi.mesh[4], N), rng.uniform(bj.mesh[5], bj.mesh[6], N)
    _, got = run_and_gate(lib, bi, bj, xi, xj, "b one cell pair N %d (ppb %d s0 %d)" % (N, ppb, s0))
    assert np.count_nonzero(got) == 16 and np.count_nonzero(got[3:7, 5:9]) == 16


def test_every_point_on_one_knot_pair_counts_exactly(lib):
    """The accumulator's true worst case, beyond the order-3 cases above: order 1, every point on the interior knots mesh_i[4] and
    mesh_j[6], where one hat function of each basis is exactly 1.  Each workgroup adds ppb times 2^s0 into ONE LDS word
    (9216 2^48 = 2^61.2 of the 2^62 the rule leaves), and every operation on the way is exact in integers: the entry is N
    to the last bit, the other three entries of the cell pair receive exact zeros, nothing else is touched."""
    N = 2097153
    bi, bj = cross_basis(1, 0, 1, 17), cross_basis(1, -1, 3, 9)          # 16 cells of 1/16, 8 cells of 1/2: t = 1 exactly
    assert bi.delta == 0.0625 and bj.delta == 0.5 and launch_plan(N, 17 * 9, 17, 9) == (True, 256, 8, 9216, 48)
    st, got = cross(lib, bi, bj, np.full(N, bi.mesh[4]), np.full(N, bj.mesh[6]))
    assert st == OK, (st, lib.asvgp_last_error_string())
    ref = np.zeros((17, 9))
    ref[4, 6] = N                       # the knot belongs to the cell on its left, t = 1: piece 0 is 1 (row idx + 1), piece 1 is 0
    print("cross block b one knot pair N %d: entry - N = %g" % (N, got[4, 6] - N))
    assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------------ c. LDS threshold
N_C = 20000                                   # G = 10 partial images on the LDS path


def _c_case(order, m_i, m_j, seed):
    bi, bj = cross_basis(order, 0, 1, m_i), cross_basis(order, -3.5, 10.5, m_j)      # j: float32-linspace mesh, cells not exactly delta wide
    assert np.any(np.diff(bj.mesh) != bj.delta)
    rng = np.random.default_rng(seed)
    return bi, bj, rng.uniform(0, 1, N_C), rng.uniform(-3.5, 10.5, N_C)


def _refused_for_workspace(lib, bi, bj, xi, xj):
    """8 bytes of workspace: the LDS path needs G partial images and says so; out is not judged"""
    st, _ = cross(lib, bi, bj, xi, xj, ws_bytes=8)
    assert st == ERR_WORKSPACE, (st, lib.asvgp_last_error_string())
    msg = lib.asvgp_last_error_string()
    assert b"phi_cross_2d" in msg and b" 8 B" in msg and b" %d B" % (10 * 8 * bi.m * bj.m) in msg, msg


def test_largest_block_on_the_lds_path(lib):
    """Order 3, 142 x 141: 8 (20022 + 140 + 139) = 162 408 B of LDS under 1024 threads, the largest request the kernel makes
    (the budget is 163 328 B)."""
    bi, bj, xi, xj = _c_case(3, 142, 141, 1)
    assert launch_plan(N_C, 142 * 141, 140, 139)[:2] == (True, 10) and 8 * (142 * 141 + 140 + 139) == 162408
    assert lib.asvgp_phi_cross_workspace_bytes(142, 141) == 256 * 8 * 142 * 141
    run_and_gate(lib, bi, bj, xi, xj, "c order 3 142x141 (LDS path)")
    _refused_for_workspace(lib, bi, bj, xi, xj)


def test_first_block_on_the_l2_path(lib):
    """Order 3, 142 x 142: one entry row more, 163 552 B, L2 atomics; the 8 bytes the workspace function returns suffice."""
    bi, bj, xi, xj = _c_case(3, 142, 142, 2)
    assert not launch_plan(N_C, 142 * 142, 140, 140)[0] and lib.asvgp_phi_cross_workspace_bytes(142, 142) == 8
    run_and_gate(lib, bi, bj, xi, xj, "c order 3 142x142 (L2 path, 8 B)", ws_bytes=8)


def test_workspace_rule_and_launch_rule_disagree_safely(lib):
    """Order 1, 147 x 137: the workspace function sizes for the LDS path (it assumes the shortest meshes, order 6: E + n_min =
    20 413 doubles fit), the launch takes the L2 path (order 1 meshes: E + n_i + n_j = 20 423 do not).  Both sizes run, both right."""
    bi, bj, xi, xj = _c_case(1, 147, 137, 3)
    assert not launch_plan(N_C, 147 * 137, 147, 137)[0]
    assert lib.asvgp_phi_cross_workspace_bytes(147, 137) == 256 * 8 * 147 * 137
    ref, cnt = O.additive_cross_block_extended(bi, bj, xi, xj)
    for wsb in (None, 8):
        st, got = cross(lib, bi, bj, xi, xj, ws_bytes=wsb)
        assert st == OK, (wsb, st, lib.asvgp_last_error_string())
        gate(got, ref, cnt, N_C, "c order 1 147x137 (L2 path, workspace %s)" % ("full" if wsb is None else "8 B"))


@pytest.mark.parametrize("order", [1, 2, 4, 5, 6])
def test_l2_path_at_every_order(lib, order):
    """phi_cross_kernel<order, L2>: 150 x 140 (21 000 entries) at the orders the model tests never run there."""
    bi, bj, xi, xj = _c_case(order, 150, 140, 10 + order)
    assert not launch_plan(N_C, 21000, bi.mesh.shape[0], bj.mesh.shape[0])[0]
    run_and_gate(lib, bi, bj, xi, xj, "c order %d 150x140 (L2 path, 8 B)" % order, ws_bytes=8)


# ------------------------------------------------------------------------------------------------ d. buffers
def test_no_points_gives_zeros(lib):
    bi, bj = _b_bases()
    st, got = cross(lib, bi, bj, np.zeros(0), np.zeros(0), null_x=True)
    assert st == OK and got.shape == (20, 17) and (got == 0).all()


def test_stale_workspace_is_ignored(lib):
    """One workspace, N = 600 000 (256 partial images) and then N = 3000 (2 images) without clearing it: the second reduce must
    not read what the first launch left behind."""
    bi, bj = _b_bases()
    assert launch_plan(600000, 340, 18, 15)[1] == 256 and launch_plan(3000, 340, 18, 15)[1] == 2
    ws = nan_buffer(lib.asvgp_phi_cross_workspace_bytes(20, 17))
    rng = np.random.default_rng(6)
    for N in (600000, 3000):
        xi, xj = rng.uniform(0, 1, N), rng.uniform(-1, 2, N)
        run_and_gate(lib, bi, bj, xi, xj, "d shared workspace N %d" % N, ws=ws)
        assert torch.isfinite(ws[:340 * launch_plan(N, 340, 18, 15)[1]]).all()       # (the images this launch wrote)


def test_lds_path_with_one_reduce_slice_is_deterministic(lib):
    """N = 100 000, G = 49: integer LDS sums, then one fixed-order sum per entry onto a zeroed out - the same bits every time.
    (G >= 64 and the L2 path add with fp64 atomics in arrival order; no bit equality is promised there.)"""
    bi, bj = _b_bases()
    assert launch_plan(100000, 340, 18, 15)[:3] == (True, 49, 1)
    rng = np.random.default_rng(7)
    xi, xj = rng.uniform(0, 1, 100000), rng.uniform(-1, 2, 100000)
    err, first = run_and_gate(lib, bi, bj, xi, xj, "d determinism N 100000")
    st, second = cross(lib, bi, bj, xi, xj)
    assert st == OK and torch.equal(torch.from_numpy(first), torch.from_numpy(second))


# ------------------------------------------------------------------------------------------------ e. through the model
def elbo_tol(e, N, v, s, yy):
    """tests/test_gpu_parity.py elbo_tol, sequential sweeps"""
    return 1e-9 * abs(e) + 2e-11 * (0.5 * N * v / s + 0.5 * yy / s)


#                (order, a, b, m, kind, variance, lengthscale) per dimension
MODEL_CASES = [[(1, 0, 1, 9, 0, 1.0, 0.3), (1, -3.5, 10.5, 24, 0, 0.8, 3.0)],
               [(5, 0, 1, 12, 2, 1.0, 0.3), (5, -1, 2, 17, 1, 0.8, 1.2), (5, -3.5, 10.5, 24, 0, 1.2, 4.0)],
               [(6, -1, 2, 14, 1, 0.9, 1.0), (6, -3.5, 10.5, 20, 0, 1.1, 5.0)]]      # (the static bands need m >= 2 order + 2)


@pytest.mark.parametrize("specs", MODEL_CASES, ids=["order1-d2", "order5-d3", "order6-d2"])
def test_additive_model_at_unused_orders_and_mixed_domains(lib, specs):
    """GPR_additive at orders 1, 5 and 6 with every dimension on another domain (a swap of mesh_i[0] and mesh_j[0] shows here):
    statistics, bound and posterior against the dense oracle with the gates of test_additive_statistics_elbo_predict_vs_oracle;
    the cross blocks also against the long-double reference.  Prediction points include both ends of every domain."""
    import asvgp_amd as A
    N, s = 3001, 0.05
    d = len(specs)
    rng = np.random.default_rng(100 * specs[0][0] + d)
    lo = np.array([float(a) for (_, a, _, _, _, _, _) in specs])
    hi = np.array([float(b) for (_, _, b, _, _, _, _) in specs])
    U = rng.uniform(0.001, 0.999, (N, d))
    X = lo + U * (hi - lo)
    y = (np.sin(6 * U[:, 0]) + U[:, 1] ** 2 - (np.cos(5 * U[:, 2]) if d > 2 else 0) + 0.1 * rng.normal(size=N)).reshape(-1, 1)
    bases = [getattr(A, "B%dSpline" % o)(a, b, m) for (o, a, b, m, _, _, _) in specs]
    obases = [O.Basis(o, a, b, m) for (o, a, b, m, _, _, _) in specs]
    kerns = [getattr(A, KINDS[kd])(variance=v, lengthscales=l) for (_, _, _, _, kd, v, l) in specs]
    kinds = [kd for (_, _, _, _, kd, _, _) in specs]
    thetas = [(v, l) for (_, _, _, _, _, v, l) in specs]
    model = A.GPR_additive((X, y), kerns, bases)
    model.likelihood.variance.assign(s)
    Aref, bref, yy = O.additive_stats(obases, X, y)
    got = model.KufKfu.cpu().numpy()
    assert got.shape == Aref.shape
    assert np.max(np.abs(got - Aref)) <= 1e-12 * np.max(np.abs(Aref))
    assert (got[Aref == 0] == 0).all()
    off = np.concatenate([[0], np.cumsum([bs.m for bs in obases])])
    for i in range(d):
        for j in range(i + 1, d):
            ref, cnt = O.additive_cross_block_extended(obases[i], obases[j], X[:, i], X[:, j])
            gate(got[off[i]:off[i + 1], off[j]:off[j + 1]], ref, cnt, N, "e order %d block (%d, %d)" % (specs[0][0], i, j))
            assert np.array_equal(got[off[j]:off[j + 1], off[i]:off[i + 1]], got[off[i]:off[i + 1], off[j]:off[j + 1]].T)
    np.testing.assert_allclose(model.Kuf_y.cpu().numpy(), bref, rtol=0, atol=1e-12 * np.max(np.abs(bref)))
    assert abs(model.tr_yTy.item() - yy) <= 1e-12 * yy
    oe, _ = O.elbo_additive(obases, kinds, thetas, s, X, y)
    e = model.elbo().item()
    print("group e order %d: elbo %.15g oracle %.15g tol %.3g" % (specs[0][0], e, oe, elbo_tol(oe, N, sum(v for v, _ in thetas), s, yy)))
    assert abs(e - oe) <= elbo_tol(oe, N, sum(v for v, _ in thetas), s, yy), (e, oe)
    Xs = lo + rng.uniform(0.01, 0.99, (300, d)) * (hi - lo)
    Xs[0], Xs[1] = lo, hi                                           # both ends of every domain
    Xs[2, 0], Xs[3, d - 1] = hi[0], lo[d - 1]                       # (and an end against interior points)
    om, ov = O.predict_f_additive(obases, kinds, thetas, s, X, y, Xs)
    mean, var = model.predict_f(Xs)
    assert mean.shape == (300, 1) and var.shape == (300, 1)
    print("group e order %d: posterior mean err %.2e var err %.2e" % (specs[0][0], np.max(np.abs(mean - om)), np.max(np.abs(var - ov))))
    np.testing.assert_allclose(mean, om, rtol=0, atol=1e-8)
    np.testing.assert_allclose(var, ov, rtol=0, atol=1e-8)
