"""CPU (-m "not gpu"): the C-ABI library builds, loads and exports every symbol include/asvgp_hip.h declares
(no compute calls), host-side argument checking, host logic of the package (mesh, static bands, parameter
transforms), and the N>1 sharding + collective path on gloo with world_size 2."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import asvgp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def lib():
    from asvgp_amd import build, _lib
    build.build(verbose=False)
    return _lib.get_lib()


def test_library_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(ROOT, "include", "asvgp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(asvgp_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 24
    from asvgp_amd import _lib
    for n in names:
        assert hasattr(lib, n), "libasvgp_hip.so does not export %s" % n
        assert n in _lib.SIGNATURES, "no ctypes prototype for %s" % n
    assert lib.asvgp_version() >= 100
    assert lib.asvgp_status_name(0) == b"ASVGP_OK"
    assert lib.asvgp_status_name(-3) == b"ASVGP_ERR_LDS_CAPACITY"


def test_host_side_argument_checks_fail_loudly(lib):
    from asvgp_amd import _lib
    assert lib.asvgp_cholesky_band(None, None, 10, 4, None, None) == -1
    assert b"cholesky_band" in lib.asvgp_last_error_string()
    assert lib.asvgp_cholesky_band(ctypes.c_void_p(8), ctypes.c_void_p(8), 10, 9, None, None) == -2   # bandwidth > 8
    assert lib.asvgp_phi_accumulate_1d(None, ctypes.c_void_p(8), ctypes.c_void_p(8), 10, 1, ctypes.c_void_p(8), 7, 0.1, 4, 10,
                                       ctypes.c_void_p(8), None, 0, None) == -4                         # no workspace
    assert lib.asvgp_phi_accumulate_1d(None, ctypes.c_void_p(8), ctypes.c_void_p(8), 10, 1, ctypes.c_void_p(8), 5, 0.1, 4, 10,
                                       ctypes.c_void_p(8), ctypes.c_void_p(8), 1 << 30, None) == -1     # n_mesh != M-k+1
    assert lib.asvgp_phi_accumulate_1d(None, ctypes.c_void_p(8), ctypes.c_void_p(8), 10, 1, ctypes.c_void_p(8), 7, 0.1, 7, 13,
                                       ctypes.c_void_p(8), ctypes.c_void_p(8), 1 << 30, None) == -2     # order 7
    assert lib.asvgp_set_band_algorithm(None, 7) == -1 and lib.asvgp_set_phi_algorithm(None, 2) == -1
    assert lib.asvgp_destroy(None) == 0
    assert lib.asvgp_phi_workspace_bytes(2048, 4, 1) == 8 * 256 * (7 * 2048 + 1)
    assert lib.asvgp_elbo_workspace_bytes(2048, 4, 1) >= 8 * (9 * 5 * 2048 + 2 * 2048)
    with pytest.raises(_lib.AsvgpError):
        _lib.check(-2, "x")
    with pytest.raises(_lib.AsvgpError):
        _lib.require_cuda(torch.zeros(3))


def test_matern_coefficient_table(lib):
    for kind in (0, 1, 2):
        for v, l in ((1.0, 1.0), (0.8, 1.03), (2.5, 0.05)):
            c = (ctypes.c_double * 9)()
            dc = (ctypes.c_double * 9)()
            n = ctypes.c_int(0)
            assert lib.asvgp_matern_coeffs(kind, v, l, c, dc, ctypes.byref(n)) == 0
            terms = O.kuu_terms(kind, v, l)
            assert n.value == len(terms)
            for t, (nm, cc, dcc) in enumerate(terms):
                assert c[t] == cc, (kind, nm)                      # same rounding sequence as inducing_features.py
                assert abs(dc[t] - dcc) <= 1e-15 * abs(dcc) if dcc else dc[t] == 0
    n = ctypes.c_int(0)
    c = (ctypes.c_double * 9)()
    assert lib.asvgp_matern_coeffs(7, 1.0, 1.0, c, c, ctypes.byref(n)) == -2
    assert lib.asvgp_matern_coeffs(1, -1.0, 1.0, c, c, ctypes.byref(n)) == -1


def test_package_host_logic_mesh_and_static_bands(golden_dir):
    import asvgp_amd as A
    F = np.load(os.path.join(golden_dir, "basis_fixtures.npz"))
    cpu = torch.device("cpu")
    for tag in F["tags"]:
        order, a, b, m, isf = F[tag + "/spec"]
        order, m = int(order), int(m)
        a, b = (float(a), float(b)) if isf else (int(a), int(b))
        bs = getattr(A, "B%dSpline" % order)(a, b, m, device=cpu)
        assert bs.order == order and bs.m == m
        assert np.array_equal(bs.mesh_np, F[tag + "/mesh"]) and bs.delta_np == float(F[tag + "/delta"])
        for nm in ("A", "B", "C", "D", "BC", "BC_grad", "BC_ggrad", "BC_ggrad_none", "BC_none_ggrad"):
            if tag + "/" + nm in F:
                ref = F[tag + "/" + nm]
                assert np.max(np.abs(ref - bs.static_np[nm])) <= 4e-15 * max(np.max(np.abs(ref)), 1e-300), (tag, nm)
            else:
                assert not hasattr(bs, nm) or m > 100
    with pytest.raises(NameError):
        A.B4Spline(0, 1, 11, device=cpu)
    # compute entry points refuse to run without the GPU
    from asvgp_amd import _lib
    bs = A.B3Spline(0, 1, 20, device=cpu)
    with pytest.raises(_lib.AsvgpError):
        bs.neighbour_index(np.array([0.5]))


def test_parameter_transforms():
    from asvgp_amd import kernels as K
    p = K.Parameter(1.0)
    assert abs(float(p) - 1.0) < 1e-15 and abs(p.unconstrained - O.softplus_inv(1.0)) < 1e-15
    g = K.Gaussian()
    assert abs(float(g.variance) - 1.0) < 1e-15 and abs(g.variance.unconstrained - O.softplus_inv(1.0 - 1e-6)) < 1e-15
    for u in (-30.0, -1.0, 0.0, 2.0, 40.0):
        p.unconstrained = u
        assert abs(float(p) - O.softplus(u)) <= 1e-15 * max(1.0, abs(u))
        assert abs(p.dtheta_du() - O.sigmoid(u)) < 1e-15
    k = K.Matern52(variance=2.0, lengthscales=0.3)
    assert k.kind == 2 and abs(2 * k.variance - 4.0) < 1e-14 and abs(k.lengthscales ** 2 - 0.09) < 1e-15


def test_shard_bounds_cover_and_align():
    from asvgp_amd.dist import shard_bounds
    for N in (0, 1, 7, 1000, 10_000_000, 10_000_001):
        for W in (1, 2, 3, 4, 8):
            spans = [shard_bounds(N, W, r) for r in range(W)]
            assert spans[0][0] == 0 and spans[-1][1] == N
            for (l0, h0), (l1, h1) in zip(spans, spans[1:]):
                assert h0 == l1 and l0 <= h0
            assert all(lo % 2 == 0 for lo, hi in spans if hi > lo)


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from asvgp_amd.dist import allreduce_stats, shard_bounds
    rng = np.random.default_rng(99)
    N, M = 5001, 40
    x = rng.uniform(0.001, 0.999, N)
    y = rng.normal(size=(N, 1))
    bs = O.Basis(4, 0, 1, M)
    lo, hi = shard_bounds(N, world, rank)
    band, rhs, yy = O.sufficient_stats_direct(bs, x[lo:hi], y[lo:hi])     # the oracle stands in for the HIP Phi pass
    packed = torch.from_numpy(np.concatenate([band.reshape(-1), rhs.reshape(-1), [yy]]))
    n_glob = allreduce_stats(packed, hi - lo, None)
    q.put((rank, n_glob, packed.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_band_allreduce_matches_single_rank():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    rng = np.random.default_rng(99)
    N, M = 5001, 40
    x = rng.uniform(0.001, 0.999, N)
    y = rng.normal(size=(N, 1))
    band, rhs, yy = O.sufficient_stats_direct(O.Basis(4, 0, 1, M), x, y)
    full = np.concatenate([band.reshape(-1), rhs.reshape(-1), [yy]])
    for rank, n_glob, packed in res:
        assert n_glob == N
        np.testing.assert_allclose(packed, full, rtol=0, atol=1e-12 * np.max(np.abs(full)))   # sum order differs: tolerance
    # the ELBO from the all-reduced statistics equals the single-rank one
    e1, _ = O.elbo_1d(O.make_Kuu(O.Basis(4, 0, 1, M), 1, 1.0, 0.1), band, rhs, yy, N, 1.0, 0.05)
    p = res[0][2]
    e2, _ = O.elbo_1d(O.make_Kuu(O.Basis(4, 0, 1, M), 1, 1.0, 0.1), p[:5 * M].reshape(5, M), p[5 * M:6 * M].reshape(M, 1),
                      p[-1], N, 1.0, 0.05)
    assert abs(e1 - e2) <= 1e-10 * abs(e1)


def test_bench_self_launch_dry_two_ranks():
    """bench.py --gpus 2 without a torchrun environment spawns its own workers before any GPU call;
    ASVGP_BENCH_DRY=1 stops after the rendezvous + one all-reduce so that the launcher can be rehearsed without a GPU."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["ASVGP_BENCH_DRY"] = "1"
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == {"dry": True, "n_gpus": 2, "ranks_seen": 2}


# ------------------------------------------------------------------------------------------------ planned prior chain (host part)
def _bcr_forward_long_double(K, B):
    """Forward pass of block cyclic reduction (odd-even elimination of the B x B block-tridiagonal view of the lower band K),
    every node, in numpy long double: what asvgp_prior_forward_host must reproduce on its de-duplicated nodes."""
    ld = np.longdouble
    k, M = K.shape[0] - 1, K.shape[1]
    nb = (M + B - 1) // B
    D = [np.zeros((B, B), ld) for _ in range(nb)]
    E = [np.zeros((B, B), ld) for _ in range(nb)]
    for j in range(M):
        for d in range(k + 1):
            i = j + d
            if i < M:
                if i // B == j // B:
                    D[i // B][i % B, j % B] = D[i // B][j % B, i % B] = K[d, j]
                else:
                    E[j // B][i % B, j % B] = K[d, j]
    for r in range(M, nb * B):
        D[r // B][r % B, r % B] = 1

    def chol(A):
        L = np.zeros_like(A)
        for j in range(B):
            L[j, j] = np.sqrt(A[j, j] - np.sum(L[j, :j] ** 2))
            for i in range(j + 1, B):
                L[i, j] = (A[i, j] - np.sum(L[i, :j] * L[j, :j])) / L[j, j]
        return L

    def solve(L, X):
        X = X.copy()
        for i in range(B):
            X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
        return X
    fac, logdet, h = {}, ld(0), 1
    while h < nb:
        for i in range(h, nb, 2 * h):
            a, b = i - h, i + h
            L = chol(D[i])
            logdet += 2 * np.sum(np.log(np.diag(L)))
            Ua = solve(L, E[a])
            Ub = solve(L, E[i].T) if b < nb else np.zeros((B, B), ld)
            fac[i] = (L, Ua, Ub)
            D[a] = D[a] - Ua.T @ Ua
            if b < nb:
                D[b] = D[b] - Ub.T @ Ub
                E[a] = -(Ub.T @ Ua)
        h *= 2
    L0 = chol(D[0])
    logdet += 2 * np.sum(np.log(np.diag(L0)))
    return fac, L0, logdet


@pytest.mark.parametrize("order,M,kind,l", [(4, 2048, 1, 0.05), (4, 2047, 1, 0.05), (4, 1024, 0, 0.1), (4, 512, 2, 0.03), (3, 333, 2, 0.03), (4, 64, 1, 0.3)])
def test_closed_form_kuu_equals_the_assembled_band_bit_for_bit(lib, order, M, kind, l):
    """The matrix-core P chain does not wait for the assembled Kuu: it receives diagonal values on the Toeplitz interior and a table of
    the boundary columns (prior_plan_interior_kuu).  Every entry must be the very double inducing_features.py:12-44 produces."""
    import ctypes
    bs = O.Basis(order, 0, 1, M)
    terms = O.kuu_terms(kind, 0.9, l)
    S = np.ascontiguousarray(np.stack([getattr(bs, nm) for nm, _, _ in terms]))
    c = np.array([t[1] for t in terms])
    kd, bnd = np.zeros(8), np.zeros(256)
    lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.asvgp_prior_interior_kuu_host(S.ctypes.data, len(terms), M, order, c.ctypes.data, kd.ctypes.data, ctypes.byref(lo),
                                             ctypes.byref(hi), bnd.ctypes.data) == 0
    lo, hi = lo.value, hi.value
    assert 0 < lo <= 16 and M - 16 <= hi <= M - order and hi - lo > M // 2
    K = O.make_Kuu(bs, kind, 0.9, l)                       # (order + 1, M) lower band
    for d in range(order + 1):
        assert np.array_equal(K[d, lo:hi], np.full(hi - lo, kd[d])), d
        assert np.array_equal(K[d, :lo], bnd[d * 16:d * 16 + lo]), d
        n_right = M - d - hi                                # entries of diagonal d that exist to the right of the interior
        assert np.array_equal(K[d, hi:M - d], bnd[(8 + d) * 16:(8 + d) * 16 + n_right]), d


def test_host_forward_pass_runs_in_x87_extended_precision(lib):
    """VERDICT r2 #1d: prior_plan.cpp static_asserts LDBL_MANT_DIG == 64; the library reports the width it was built with, and numpy's
    longdouble on this host - the oracle's extended evaluation - is the same format."""
    assert lib.asvgp_host_mantissa_bits() == 64
    assert np.finfo(np.longdouble).nmant == 63          # (numpy counts the stored fraction bits: 64-bit mantissa with its explicit leading bit)


@pytest.mark.parametrize("order,M,kind,l", [(4, 2048, 1, 0.05), (4, 2047, 1, 0.05), (4, 1024, 0, 0.1), (3, 333, 2, 0.03), (5, 129, 2, 0.1),
                                            (6, 90, 1, 0.08), (1, 37, 0, 0.08), (2, 64, 1, 0.08), (4, 13, 0, 0.3)])
def test_prior_plan_host_forward_vs_long_double_bcr(lib, order, M, kind, l):
    """asvgp_prior_forward_host eliminates ONE representative per class of bit-identical nodes; every node's factors
    (through the node -> record map), the log-determinant and the l-tangents must equal the all-nodes long-double forward pass."""
    bs = O.Basis(order, 0, 1, M)
    terms = O.kuu_terms(kind, 0.9, l)
    S = np.ascontiguousarray(np.stack([getattr(bs, nm) for nm, _, _ in terms]))
    c = np.array([t[1] for t in terms])
    dc = np.array([t[2] for t in terms])
    n = lib.asvgp_prior_table_doubles(S.ctypes.data, len(terms), M, order)
    assert n > 0
    tab = np.zeros(n)
    nb = (M + order - 1) // order
    rec = np.zeros(nb, dtype=np.int32)
    assert lib.asvgp_prior_forward_host(S.ctypes.data, len(terms), M, order, c.ctypes.data, dc.ctypes.data, tab.ctypes.data, n,
                                        rec.ctypes.data) == 0
    B, R = order, int(tab[3])
    W = 6 * B * B + B          # L, 1/diag, U_a, U_b | G_a^T, G_b^T, D^-1 (the matrix-core backward pass's operands)
    assert n == 8 + 2 * R * W and tab[2] == 0 and R <= 3 * 12 and rec.min() >= 0 and rec.max() == R - 1 == rec[0]
    val, tan = tab[8:8 + R * W].reshape(R, W), tab[8 + R * W:].reshape(R, W)
    K, dK = O.make_Kuu(bs, kind, 0.9, l, want_dl=True)
    fac, L0, logdet = _bcr_forward_long_double(K, B)
    cond_slack = 1e-9 if kind == 2 else 1e-11      # two 64-bit-mantissa evaluations in different operation orders, times cond(Kuu)
    for i, (L, Ua, Ub) in fac.items():
        for off, X in ((0, L), (B * B + B, Ua), (2 * B * B + B, Ub)):
            got = val[rec[i], off:off + B * B].reshape(B, B)
            assert np.max(np.abs(got - X.astype(np.float64))) <= cond_slack * max(1.0, float(np.max(np.abs(X)))), (i, off)
        np.testing.assert_allclose(val[rec[i], B * B:B * B + B] * np.diag(L).astype(np.float64), 1.0, rtol=cond_slack)
        Li = np.linalg.inv(L.astype(np.float64)).astype(np.longdouble)      # (4 x 4 .. 6 x 6 triangular: well conditioned)
        Li = Li + Li @ (np.eye(B, dtype=np.longdouble) - L @ Li)             # one refinement step in long double
        for off, X in ((3 * B * B + B, Ua.T @ Li), (4 * B * B + B, Ub.T @ Li), (5 * B * B + B, Li.T @ Li)):
            got = val[rec[i], off:off + B * B].reshape(B, B)
            assert np.max(np.abs(got - X.astype(np.float64))) <= 10 * cond_slack * max(1.0, float(np.max(np.abs(X)))), (i, off)
    np.testing.assert_allclose(val[rec[0], :B * B].reshape(B, B), L0.astype(np.float64), rtol=0, atol=cond_slack * float(np.max(L0)))
    assert abs(tab[0] - float(logdet)) <= max(1e-12, cond_slack * 1e-2) * abs(float(logdet))
    # tangents against central differences of the long-double pass (well-conditioned cases only resolve this)
    h = 1e-6 * l
    fp, _, ldp = _bcr_forward_long_double(O.make_Kuu(bs, kind, 0.9, l + h), B)
    fm, _, ldm = _bcr_forward_long_double(O.make_Kuu(bs, kind, 0.9, l - h), B)
    assert abs(tab[1] - float((ldp - ldm) / (2 * h))) <= 2e-5 * abs(tab[1])
    if M <= 129:
        for i in fac:
            for off, q in ((0, 0), (B * B + B, 1), (2 * B * B + B, 2)):
                fd = ((fp[i][q] - fm[i][q]) / (2 * h)).astype(np.float64)
                got = tan[rec[i], off:off + B * B].reshape(B, B)
                assert np.max(np.abs(got - fd)) <= 1e-5 * max(1e-12, float(np.max(np.abs(fd)))), (i, off)

            def gmats(f):
                L_, Ua_, Ub_ = f
                Li_ = np.linalg.inv(L_.astype(np.float64))
                return Ua_.astype(np.float64).T @ Li_, Ub_.astype(np.float64).T @ Li_, Li_.T @ Li_
            for off, Xp, Xm in zip((3 * B * B + B, 4 * B * B + B, 5 * B * B + B), gmats(fp[i]), gmats(fm[i])):
                fd = (Xp - Xm) / (2 * h)
                got = tan[rec[i], off:off + B * B].reshape(B, B)
                assert np.max(np.abs(got - fd)) <= 1e-4 * max(1e-12, float(np.max(np.abs(fd)))), (i, off)
    # a band without Toeplitz structure has no plan
    rng = np.random.default_rng(0)
    Sr = np.ascontiguousarray(S + rng.uniform(0, 1e-3, S.shape) * (np.abs(S) > 0))
    if nb > 64:
        assert lib.asvgp_prior_table_doubles(Sr.ctypes.data, len(terms), M, order) == 0


@pytest.mark.parametrize("order,M,kind", [(4, 2048, 1), (4, 2047, 1), (3, 333, 2), (6, 90, 1), (1, 37, 0), (4, 13, 0), (4, 4096, 2)])
def test_prior_plan_device_image_is_consistent_with_the_host_plan(lib, order, M, kind):
    """The GPU forward pass (csrc/prior_dd.hpp, asvgp_set_prior_forward(h, 1)) walks a flat image of the plan: class maps per level as ints,
    the static-band entries of the level-0 representative blocks as doubles.  Host-only checks: header fields, level offsets inside the
    image, class indices inside the previous level's class counts, node counts summing to the number of nodes a level eliminates, record
    numbering equal to the host table's, and the level-0 entries reproducing Kuu's blocks exactly (same rounding sequence as make_Kuu)."""
    bs = O.Basis(order, 0, 1, M)
    terms = O.kuu_terms(kind, 0.9, 0.07)
    S = np.ascontiguousarray(np.stack([getattr(bs, nm) for nm, _, _ in terms]))
    ni, nd = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.asvgp_prior_plan_image_host(S.ctypes.data, len(terms), M, order, None, ctypes.byref(ni), None, ctypes.byref(nd)) == 0
    ints = np.zeros(ni.value, dtype=np.int32)
    dbl = np.zeros(max(nd.value, 1))
    assert lib.asvgp_prior_plan_image_host(S.ctypes.data, len(terms), M, order, ints.ctypes.data, ctypes.byref(ni), dbl.ctypes.data, ctypes.byref(nd)) == 0
    B, nt, levels, n_rec, nd0, ne0, off_lv, total, off_dc, off_ec = [int(v) for v in ints[:10]]
    nb = (M + B - 1) // B
    assert B == order and nt == len(terms) and total == ni.value and off_lv == 16 and (1 << levels) >= nb > (1 << levels) // 2
    n = lib.asvgp_prior_table_doubles(S.ctypes.data, len(terms), M, order)
    assert n == 8 + 2 * n_rec * (6 * B * B + B)
    prev_d, prev_e, rec, left = nd0, ne0, 0, nb
    for l in range(levels):
        nq, ndn, o_node, o_rep, o_dn, rec0 = [int(v) for v in ints[off_lv + 8 * l: off_lv + 8 * l + 6]]
        assert rec0 == rec and 0 < nq <= 24 and 0 < ndn <= 24 and 16 + 8 * levels <= o_node < o_rep <= o_dn < off_dc
        node = ints[o_node:o_node + 4 * nq].reshape(nq, 4)
        assert node[:, 0].min() >= 0 and node[:, 0].max() < prev_d and node[:, 1].min() >= 0 and node[:, 1].max() < prev_e
        assert node[:, 2].min() >= -1 and node[:, 2].max() < prev_e
        assert int(node[:, 3].sum()) == left // 2                    # every second node of the level is eliminated
        reps = ints[o_rep:o_rep + nq]
        assert reps.min() >= 0 and reps.max() < nb
        dn = ints[o_dn:o_dn + 3 * ndn].reshape(ndn, 3)
        assert dn[:, 0].min() >= 0 and dn[:, 0].max() < prev_d and dn[:, 1:].min() >= -1 and dn[:, 1:].max() < nq
        rec += nq
        left -= left // 2
        prev_d, prev_e = ndn, nq                                     # next level: D classes; couplings = the fills of the eliminated nodes
    assert rec == n_rec - 1 and left == 1
    # level-0 entries: sum_t c_t * entry_t equals the Kuu block entries of a representative (class 0 = block 0: the top-left corner)
    c = np.array([t[1] for t in terms])
    K = O.make_Kuu(bs, kind, 0.9, 0.07)
    codes = ints[off_dc:off_dc + B * B].reshape(B, B)
    ent = dbl[:B * B * nt].reshape(B, B, nt)
    for r in range(B):
        for cc in range(r + 1):
            if r < M:
                acc = c[0] * ent[r, cc, 0]
                for t in range(1, nt):
                    acc = acc + c[t] * ent[r, cc, t]
                assert codes[r, cc] == 0 and acc == K[r - cc, cc], (r, cc)


SWEEPS, BCR, BCR_PRIOR, BCR_DATA, PLANNED_BCR, MATRIX_CORE = range(6)          # plan12[1] of asvgp_elbo_launch_plan_host
FWD_NOBODY, FWD_INLINE, FWD_BEFORE, FWD_CALLER, FWD_WORKER, FWD_GPU, FWD_PUBLISH_THETA = range(7)   # plan12[9]
OK, BAD_ARG, UNSUPPORTED, LDS_CAPACITY = 0, -1, -2, -3
_N_REC = {}


def _launch_plan(lib, M, k, algo=0, plan=True, D=1, part=0, tangent=1, fin=None, **flags):
    """(status, fields by name) of asvgp_elbo_launch_plan_host.  plan=True: the handle holds the plan of the uniform B-spline basis of this
    (M, k) - its record count from the host planner, its static bands Toeplitz in the interior.  fin=None: offered as the entry points do
    (the ELBO + gradient launcher, except in the prior half)."""
    n_rec = 0
    if plan:
        if (M, k) not in _N_REC:
            bs = O.Basis(k, 0, 1, M)
            terms = O.kuu_terms(1, 0.9, 0.07)
            S = np.ascontiguousarray(np.stack([getattr(bs, nm) for nm, _, _ in terms]))
            ni, nd = ctypes.c_size_t(0), ctypes.c_size_t(0)
            assert lib.asvgp_prior_plan_image_host(S.ctypes.data, len(terms), M, k, None, ctypes.byref(ni), None, ctypes.byref(nd)) == 0
            ints = np.zeros(ni.value, dtype=np.int32)
            dbl = np.zeros(max(nd.value, 1))
            assert lib.asvgp_prior_plan_image_host(S.ctypes.data, len(terms), M, k, ints.ctypes.data, ctypes.byref(ni), dbl.ctypes.data, ctypes.byref(nd)) == 0
            _N_REC[(M, k)] = int(ints[3])
        n_rec = _N_REC[(M, k)]
    if fin is None:
        fin = 1 if tangent and part != 1 else 0
    f = dict(ahead=0, gpu=0, worker=0, defer=0, no_split=0, plan_first=0)
    f.update(flags)
    out = np.full(12, -99, dtype=np.int64)
    rc = lib.asvgp_elbo_launch_plan_host(algo, int(plan), n_rec, int(plan), M, k, D, part, tangent, fin, f["ahead"], f["gpu"], f["worker"], f["defer"],
                                         f["no_split"], f["plan_first"], out.ctypes.data)
    names = ("status", "path", "part", "nothing", "big", "lds", "grid", "helpers", "split", "fwd", "scale_alpha", "scale_c")
    p = dict(zip(names, (int(v) for v in out)))
    assert p["status"] == rc
    return rc, p


def test_fused_elbo_launch_plan_follows_the_documented_rules(lib):
    """asvgp_elbo_launch_plan_host is the plan_chains the launchers of csrc/elbo.hip call before they take a table slot or launch anything.
    Which path a given (algorithm, plan, M, k, D, entry point, flags) takes, written down from the rules (include/asvgp_hip.h:
    asvgp_set_band_algorithm, asvgp_elbo_grad_ahead_1d) - the cases sit away from the LDS thresholds, so no expectation is a byte count."""
    def plan(*a, **kw):
        rc, p = _launch_plan(lib, *a, **kw)
        assert rc == OK, lib.asvgp_last_error_string()
        return p

    def refused(*a, **kw):
        return _launch_plan(lib, *a, **kw)[0]

    # the headline shape: both chains on the matrix cores, the P chain on two workgroups, no helpers, forward pass behind the launch
    p = plan(2048, 4)
    assert (p["path"], p["split"], p["grid"], p["helpers"], p["fwd"], p["nothing"]) == (MATRIX_CORE, 1, 3, 0, FWD_INLINE, 0)
    assert (p["scale_alpha"], p["scale_c"]) == (0, 0) and 0 < p["lds"] <= 160 * 1024
    p = plan(2048, 4, no_split=1)
    assert (p["path"], p["split"], p["grid"]) == (MATRIX_CORE, 0, 2)
    p = plan(64, 4)
    assert (p["path"], p["split"], p["grid"]) == (MATRIX_CORE, 0, 2)
    assert plan(2048, 4, algo=4)["path"] == MATRIX_CORE
    # where the matrix cores do not apply: the planned chain on the BCR kernel, forward pass in front of the launch, up to six helpers
    p = plan(2052, 4)                                              # 513 block nodes
    assert (p["path"], p["grid"], p["helpers"], p["fwd"]) == (PLANNED_BCR, 8, 6, FWD_BEFORE)
    assert plan(2048, 4, D=2)["path"] == PLANNED_BCR
    p = plan(200, 3)
    assert (p["path"], p["grid"], p["helpers"], p["split"]) == (PLANNED_BCR, 3, 1, 0)
    assert plan(200, 3, algo=3)["path"] == PLANNED_BCR
    p = plan(2048, 4, tangent=0)                                   # the posterior launchers offer no fused finalize
    assert (p["path"], p["scale_alpha"], p["scale_c"]) == (PLANNED_BCR, 1, 0)
    assert plan(2048, 4, fin=0)["path"] == PLANNED_BCR
    # no plan, or an algorithm that does not use it
    p = plan(200, 3, plan=False)
    assert (p["path"], p["grid"], p["fwd"], p["scale_alpha"], p["scale_c"]) == (BCR, 2, FWD_NOBODY, 0, 0)
    p = plan(2048, 4, algo=2)
    assert (p["path"], p["fwd"]) == (BCR, FWD_NOBODY)
    p = plan(2048, 4, algo=1)
    assert (p["path"], p["grid"], p["lds"], p["fwd"], p["scale_alpha"], p["scale_c"]) == (SWEEPS, 2, 0, FWD_NOBODY, 1, 1)
    assert plan(200000, 4, plan=False)["path"] == SWEEPS          # auto: the chains do not fit the LDS
    # refusals
    assert refused(2048, 4, algo=3, plan=False) == BAD_ARG and refused(2048, 4, algo=4, plan=False) == BAD_ARG
    assert b"asvgp_prior_plan_1d" in lib.asvgp_last_error_string()
    assert refused(200, 3, algo=4) == UNSUPPORTED
    assert b"matrix-core" in lib.asvgp_last_error_string()
    assert refused(2052, 4, algo=4) == UNSUPPORTED and refused(2048, 4, algo=4, D=2) == UNSUPPORTED
    assert refused(200000, 4, algo=2, plan=False) == LDS_CAPACITY
    assert b"LDS" in lib.asvgp_last_error_string()
    # the split entry points: halves on the all-GPU BCR path only; elsewhere the prior half has nothing to do and the data half runs whole
    p = plan(200, 3, plan=False, part=1)
    assert (p["path"], p["part"], p["grid"], p["nothing"]) == (BCR_PRIOR, 1, 1, 0)
    p = plan(200, 3, plan=False, part=2)
    assert (p["path"], p["part"], p["grid"], p["nothing"]) == (BCR_DATA, 2, 1, 0)
    assert plan(2048, 4, algo=1, part=1)["nothing"] == 1
    p = plan(2048, 4, algo=1, part=2)
    assert (p["path"], p["part"], p["nothing"]) == (SWEEPS, 0, 0)
    assert plan(2048, 4, part=1)["nothing"] == 1 and plan(200, 3, part=1)["nothing"] == 1
    p = plan(2048, 4, part=2)
    assert (p["path"], p["part"], p["nothing"], p["grid"]) == (MATRIX_CORE, 0, 0, 3)
    p = plan(200, 3, part=2)
    assert (p["path"], p["part"], p["nothing"]) == (PLANNED_BCR, 0, 0)
    # who runs the forward pass of the planned Kuu chain
    assert plan(2048, 4, defer=1)["fwd"] == FWD_CALLER
    assert plan(2048, 4, worker=1)["fwd"] == FWD_WORKER and plan(2048, 4, worker=1, defer=1)["fwd"] == FWD_WORKER
    assert plan(2048, 4, gpu=1)["fwd"] == FWD_GPU and plan(2048, 4, gpu=1, worker=1)["fwd"] == FWD_GPU
    assert plan(2048, 4, plan_first=1)["fwd"] == FWD_BEFORE
    assert plan(200, 3, gpu=1)["fwd"] == FWD_GPU and plan(200, 3, worker=1, defer=1)["fwd"] == FWD_BEFORE
    # launch-ahead: the matrix-core launch with the host forward pass, and nothing else
    p = plan(2048, 4, ahead=1)
    assert (p["path"], p["fwd"], p["grid"]) == (MATRIX_CORE, FWD_PUBLISH_THETA, 3)
    assert plan(2048, 4, ahead=1, worker=1)["fwd"] == FWD_PUBLISH_THETA and plan(2048, 4, ahead=1, defer=1)["fwd"] == FWD_PUBLISH_THETA
    for kw in (dict(gpu=1), dict(plan_first=1)):                   # matrix-core, but not the host forward pass behind the launch
        assert refused(2048, 4, ahead=1, **kw) == UNSUPPORTED
        assert b"launch-ahead" in lib.asvgp_last_error_string()
    for a, kw in (((200, 3), {}), ((2052, 4), {}), ((2048, 4), dict(D=2)),                                 # planned chain on the BCR kernel
                  ((200, 3), dict(plan=False)), ((2048, 4), dict(algo=2)),                                # BCR
                  ((200, 3), dict(plan=False, part=1)), ((200, 3), dict(plan=False, part=2)),             # its halves
                  ((2048, 4), dict(algo=1)), ((200000, 4), dict(plan=False)), ((2048, 4), dict(plan=False, algo=1))):   # sweeps
        assert plan(*a, **kw)["path"] != MATRIX_CORE
        assert refused(*a, ahead=1, **kw) == UNSUPPORTED, (a, kw)
        assert b"launch-ahead" in lib.asvgp_last_error_string()
    # argument checks of the entry itself
    assert lib.asvgp_elbo_launch_plan_host(0, 0, 0, 0, 64, 4, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, None) == BAD_ARG
    out = np.zeros(12, dtype=np.int64)
    assert lib.asvgp_elbo_launch_plan_host(0, 0, 0, 0, 64, 7, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, out.ctypes.data) == UNSUPPORTED


PHI_FIELDS = ("status", "kernel", "series", "shape", "lds", "G", "ppb", "chunks", "cells", "launches", "reduces", "reduce_y", "s0", "asked_mesh",
              "asked_order", "zero")                                              # plan16 of asvgp_phi_launch_plan_host
LDS_MAX = 160 * 1024


def _phi_plan(lib, N=10 ** 7, M=2048, k=4, D=1, algo=0, wg=0, defer=0, weighted=0, aligned=1, regular=1, first=0.0, last=1.0, series=0, delta=None,
              n_mesh=None):
    """(status, fields by name) of asvgp_phi_launch_plan_host for the uniform mesh of (M, k) on [first, last]"""
    n_mesh = M - k + 1 if n_mesh is None else n_mesh
    delta = (last - first) / (n_mesh - 1) if delta is None else delta
    out = np.full(16, -99, dtype=np.int64)
    rc = lib.asvgp_phi_launch_plan_host(algo, wg, defer, weighted, N, D, M, k, n_mesh, delta, aligned, regular, first, last, series, out.ctypes.data)
    p = dict(zip(PHI_FIELDS, (int(v) for v in out)))
    assert p["status"] == rc and p["zero"] == 0
    return rc, p


def test_phi_launch_plan_follows_the_documented_rules(lib):
    """asvgp_phi_launch_plan_host is the plan_phi that asvgp_phi_accumulate_1d and asvgp_phi_accumulate_1d_weighted call before they launch
    anything (csrc/phi_launch.hpp).  Which kernel and shape a given input gets, written down from the rules (include/asvgp_hip.h:
    asvgp_set_phi_algorithm, asvgp_phi_accumulate_1d_weighted) and the constants of the sources: 1024 threads, 6 / 4 points per thread and
    tile at k = 4 (plain / time series), 2048-cell images, plane strides 512 / 1024 / 2048, at most 256 workgroups, reduce slices 16 / 4 / 1
    from 64 / 8 workgroups on.  The cases sit away from the LDS thresholds, so no expectation is a byte count."""
    def plan(**kw):
        rc, p = _phi_plan(lib, **kw)
        assert rc == OK, lib.asvgp_last_error_string()
        assert 0 < p["lds"] <= LDS_MAX and p["G"] >= 1 and p["launches"] >= 1
        return p

    def refused(**kw):
        return _phi_plan(lib, **kw)[0]

    def s0_of(ppb):                                                # 62 - ceil(log2(points per workgroup)), at most 50
        return min(50, 62 - int(np.ceil(np.log2(ppb))))

    # the headline shape: the tile sort, plain instantiation, one launch and one reduce over 16 slices of the 256 partials
    p = plan()
    assert (p["kernel"], p["series"], p["shape"], p["G"]) == (6, 0, 6, 256) and p["ppb"] % 2 == 0 and p["ppb"] * 256 >= 10 ** 7
    assert (p["launches"], p["reduces"], p["reduce_y"], p["chunks"], p["cells"], p["s0"]) == (1, 1, 16, 1, 2044, -1)
    assert (p["asked_mesh"], p["asked_order"]) == (1, 1)
    p = plan(series=1)
    assert (p["kernel"], p["series"], p["shape"], p["G"]) == (6, 1, 4, 256) and p["ppb"] % 128 == 0
    assert plan(wg=240)["G"] == 240
    p = plan(defer=1)
    assert (p["kernel"], p["launches"], p["reduces"]) == (6, 1, 0)
    assert plan(algo=6)["kernel"] == 6
    # the tile sort does not apply: the centred moments, and the input order is never consulted
    for kw in (dict(N=1), dict(regular=0), dict(first=1e15, last=1e15 + 2.044, delta=1e-3)):   # one point | irregular mesh | no margin for the cell guess
        p = plan(**kw)
        assert (p["kernel"], p["shape"], p["asked_mesh"], p["asked_order"]) == (5, 2048, 1, 0), kw
        assert (p["launches"], p["reduces"], p["chunks"]) == (1, 1, 1) and p["ppb"] % 2048 == 0 and p["s0"] == s0_of(p["ppb"]), kw
    assert plan(N=1)["G"] == 1 and plan(regular=0)["G"] == 256
    assert plan(regular=0, defer=1)["reduces"] == 0
    assert plan(M=64, regular=0)["shape"] == 512 and plan(M=1000, regular=0)["shape"] == 1024   # the smallest stride that holds the cells
    assert plan(algo=5)["kernel"] == 5
    # M = 2049: the first the tile sort's 2048-cell image does not hold; its 2045 cells still lie under the moments' largest stride.
    # M = 3000: neither image holds it - the fixed-point band scatter, in column chunks
    p = plan(M=2049)
    assert (p["kernel"], p["shape"], p["asked_order"]) == (5, 2048, 0)
    p = plan(M=3000)
    assert (p["kernel"], p["series"], p["shape"]) == (3, 0, 0) and p["chunks"] > 1 and p["chunks"] * p["cells"] >= 3000 - 4
    assert (p["chunks"] - 1) * p["cells"] < 3000 - 4 and p["launches"] == p["chunks"] and p["reduces"] == p["launches"]
    assert p["ppb"] % 2048 == 0 and p["s0"] == s0_of(p["ppb"])
    # more than one output column, or inputs off the 16-byte boundary: the band scatter, and the mesh is never consulted
    for kw in (dict(D=2), dict(aligned=0)):
        p = plan(**kw)
        assert (p["kernel"], p["asked_mesh"], p["asked_order"], p["chunks"], p["cells"]) == (3, 0, 0, 1, 2044), kw
        assert p["launches"] == kw.get("D", 1) and p["reduces"] == p["launches"] and p["s0"] == s0_of(p["ppb"]), kw
    p = plan(M=3000, D=2)
    assert p["kernel"] == 3 and p["launches"] == 2 * p["chunks"]
    assert plan(D=2, defer=1)["reduces"] == 2                     # (only the single-launch kernels park their reduce)
    # forced algorithms
    p = plan(algo=1)
    assert (p["kernel"], p["s0"], p["asked_mesh"], p["asked_order"]) == (1, -1, 0, 0)
    p = plan(algo=3)
    assert (p["kernel"], p["asked_mesh"]) == (3, 0) and p["s0"] == s0_of(p["ppb"])
    for kw in (dict(D=2), dict(M=2049)):
        assert refused(algo=6, **kw) == UNSUPPORTED, kw
        assert b"tile sort" in lib.asvgp_last_error_string()
    assert refused(algo=5, D=2) == UNSUPPORTED
    assert b"algorithm 5" in lib.asvgp_last_error_string()
    # weighted: the register moments where the tile sort would apply, else the weighted band scatter; never fixed point, never deferred
    p = plan(weighted=1)
    assert (p["kernel"], p["series"], p["shape"], p["G"], p["s0"], p["asked_mesh"], p["asked_order"]) == (16, 0, 4, 256, -1, 1, 0)
    assert (p["launches"], p["reduces"], p["reduce_y"]) == (1, 1, 16) and p["ppb"] % 2 == 0
    assert plan(weighted=1, series=1)["series"] == 0 and plan(weighted=1, algo=6)["kernel"] == 16
    for kw in (dict(D=2), dict(algo=1), dict(regular=0), dict(M=2049), dict(aligned=0), dict(N=1)):
        p = plan(weighted=1, **kw)
        assert (p["kernel"], p["s0"], p["chunks"]) == (11, -1, 1) and p["ppb"] % 64 == 0, kw
    assert plan(weighted=1, D=2)["asked_mesh"] == 0 and plan(weighted=1, algo=1)["asked_mesh"] == 0
    p = plan(weighted=1, M=3000)                                   # (without the fixed-point plane the LDS holds about 2900 columns at k = 4)
    assert p["kernel"] == 11 and p["chunks"] > 1 and p["chunks"] * p["cells"] >= 3000 - 4 and p["launches"] == p["chunks"]
    for algo in (3, 5):
        assert refused(weighted=1, algo=algo) == UNSUPPORTED
        err = lib.asvgp_last_error_string()
        assert b"fixed point" in err and b"algorithm %d" % algo in err and b"phi_accumulate_1d_weighted" in err
    assert refused(weighted=1, algo=6, D=3) == UNSUPPORTED
    assert b"register moments" in lib.asvgp_last_error_string()
    assert plan(weighted=1, defer=1)["reduces"] == 1 and plan(weighted=1, D=2, defer=1)["reduces"] == 2
    # small grids: at least one tile (6 x 1024 points) per workgroup; the reduce takes 16 / 4 / 1 slices from 64 / 8 workgroups on
    p = plan(N=5000)
    assert (p["kernel"], p["G"], p["reduce_y"]) == (6, 1, 1) and p["ppb"] >= 5000
    p = plan(N=20 * 6144)
    assert (p["kernel"], p["G"], p["reduce_y"]) == (6, 20, 4)
    assert [plan(wg=g)["reduce_y"] for g in (7, 8, 63, 64)] == [1, 4, 4, 16]
    assert plan(N=0)["kernel"] == 3 and plan(N=0)["G"] == 1       # nothing to stream: the band scatter zeroes the statistics
    # argument checks of the entry itself
    assert lib.asvgp_phi_launch_plan_host(0, 0, 0, 0, 1000, 1, 64, 4, 61, 0.1, 1, 1, 0.0, 6.0, 0, None) == BAD_ARG
    assert refused(M=64, k=7, n_mesh=58) == UNSUPPORTED and b"order 7" in lib.asvgp_last_error_string()
    assert refused(M=64, n_mesh=60) == BAD_ARG and b"n_mesh" in lib.asvgp_last_error_string()
    assert refused(algo=2) == BAD_ARG and refused(wg=257) == BAD_ARG and refused(D=0) == BAD_ARG


BAND_FIELDS = ("status", "kernel", "threads", "lds", "seg", "cap", "cap_fq", "arrays_in_lds")   # plan8 of asvgp_band_launch_plan_host
CHOL, INVERSE, CHOL_VJP, INVERSE_VJP = range(4)                                                 # its op
SWEEP, STREAMED, WAVE, SEQUENTIAL = range(4)                                                    # plan8[1]


def _band_plan(lib, op, M, k=4, lds=1, seg_blocks=0):
    out = np.full(8, -99, dtype=np.int64)
    rc = lib.asvgp_band_launch_plan_host(op, M, k, lds, seg_blocks, out.ctypes.data)
    p = dict(zip(BAND_FIELDS, (int(v) for v in out)))
    assert p["status"] == rc
    return rc, p


def test_band_launch_plan_follows_the_documented_rules(lib):
    """asvgp_band_launch_plan_host is the plan_band_op that asvgp_cholesky_band, asvgp_inverse_from_cholesky_band and their two adjoints
    call before they launch anything (csrc/band_launch.hpp), with the two environment variables as arguments.  Every row is written down
    from the rules ("Which kernel an operator call runs"): W = k + 1; the forward operators divide 156 KiB by 8 W bytes per
    column (k = 4: 3993 columns; segments of (3993 - W) / W = 797 blocks of W columns, the inverse (3993 - 1) / k = 998 blocks of k), the
    Cholesky adjoint 160 KiB by 16 W (k = 4: 2048; (2048 - W) / W = 408 blocks), the inverse's adjoint holds seg W + W rows and
    seg W^2 + 1 factor doubles (k = 4: ((20479 / 5) - 5) / 10 = 409 blocks).  A row lists every field the plan fills for its kernel; the
    others are 0."""
    def plan(op, M, **kw):
        rc, p = _band_plan(lib, op, M, **kw)
        assert rc == OK, lib.asvgp_last_error_string()
        assert 0 <= p["lds"] <= LDS_MAX
        return (p["kernel"], p["threads"], p["seg"], p["cap"], p["cap_fq"], p["lds"], p["arrays_in_lds"])

    # cholesky_band, k = 4:        (kernel, threads, seg, cap, cap_fq, bytes, arrays_in_lds)
    assert plan(CHOL, 5) == (SWEEP, 64, 0, 0, 0, 0, 0)                      # M = k + 1: nothing beyond the register window
    assert plan(CHOL, 6) == (STREAMED, 256, 2, 6, 0, 240, 0)
    assert plan(CHOL, 3993) == (STREAMED, 256, 799, 3993, 0, 159720, 0)     # the last M in one segment
    assert plan(CHOL, 3994) == (STREAMED, 256, 797, 3993, 0, 159720, 0)
    assert plan(CHOL, 100, seg_blocks=2) == (STREAMED, 256, 2, 15, 0, 600, 0)
    assert plan(CHOL, 100, seg_blocks=1) == (STREAMED, 256, 1, 10, 0, 400, 0)
    assert plan(CHOL, 100, seg_blocks=20) == plan(CHOL, 100) == (STREAMED, 256, 20, 100, 0, 4000, 0)   # an override only shortens
    for M in (1, 5, 6, 100, 3994, 20000):
        assert plan(CHOL, M, lds=0) == (SWEEP, 64, 0, 0, 0, 0, 0), M
    # inverse_from_cholesky_band, k = 4
    assert plan(INVERSE, 9) == (SWEEP, 64, 0, 0, 0, 0, 0)
    assert plan(INVERSE, 10) == (STREAMED, 256, 3, 10, 0, 400, 0)
    assert plan(INVERSE, 3994) == (STREAMED, 256, 998, 3993, 0, 159720, 0)
    assert plan(INVERSE, 100, seg_blocks=2) == (STREAMED, 256, 2, 9, 0, 360, 0)
    assert plan(INVERSE, 3994, lds=0) == (SWEEP, 64, 0, 0, 0, 0, 0)
    # cholesky_band_vjp
    assert plan(CHOL_VJP, 10) == (WAVE, 256, 0, 0, 0, 800, 0)               # M = 2 (k + 1)
    assert plan(CHOL_VJP, 11) == (STREAMED, 256, 3, 11, 0, 880, 0)
    assert plan(CHOL_VJP, 2048) == (STREAMED, 256, 410, 2048, 0, 163840, 0)
    assert plan(CHOL_VJP, 2049) == (STREAMED, 256, 408, 2048, 0, 163840, 0)
    assert plan(CHOL_VJP, 100, seg_blocks=1) == (STREAMED, 256, 20, 100, 0, 8000, 0)   # the adjoints take an override from 2 on: 1 is ignored
    assert plan(CHOL_VJP, 100, seg_blocks=2) == (STREAMED, 256, 2, 15, 0, 1200, 0)
    assert plan(CHOL_VJP, 18, k=8) == (SEQUENTIAL, 256, 0, 0, 0, 2592, 1)   # M = 2 (k + 1), and 81 lanes are no wave
    assert plan(CHOL_VJP, 19, k=8) == (STREAMED, 256, 3, 19, 0, 2736, 0)
    assert plan(CHOL_VJP, 1138, k=8) == (STREAMED, 256, 125, 1137, 0, 163728, 0)
    assert plan(CHOL_VJP, 2048, lds=0) == (WAVE, 256, 0, 0, 0, 163840, 0)
    assert plan(CHOL_VJP, 3000, lds=0) == (SEQUENTIAL, 256, 0, 0, 0, 0, 0)
    # inverse_from_cholesky_band_vjp
    assert plan(INVERSE_VJP, 10) == (WAVE, 256, 0, 0, 0, 800, 0)
    assert plan(INVERSE_VJP, 11) == (STREAMED, 256, 3, 11, 55, 880, 0)
    assert plan(INVERSE_VJP, 2048) == (STREAMED, 256, 410, 2048, 10240, 163840, 0)
    assert plan(INVERSE_VJP, 2049) == (STREAMED, 256, 409, 2050, 10226, 163808, 0)
    assert plan(INVERSE_VJP, 100, seg_blocks=2) == (STREAMED, 256, 2, 15, 51, 1008, 0)
    assert plan(INVERSE_VJP, 100, seg_blocks=1) == plan(INVERSE_VJP, 100) == (STREAMED, 256, 20, 100, 500, 8000, 0)
    assert plan(INVERSE_VJP, 3000, k=6) == (STREAMED, 256, 208, 1463, 10193, 163472, 0)   # the widest band with the streamed form
    assert plan(INVERSE_VJP, 300, k=7) == (WAVE, 256, 0, 0, 0, 38400, 0)
    assert plan(INVERSE_VJP, 1280, k=7) == (WAVE, 256, 0, 0, 0, 163840, 0)
    assert plan(INVERSE_VJP, 1281, k=7) == (SEQUENTIAL, 256, 0, 0, 0, 0, 0)
    assert plan(INVERSE_VJP, 18, k=8) == (SEQUENTIAL, 256, 0, 0, 0, 2592, 1)
    assert plan(INVERSE_VJP, 19, k=8) == (SEQUENTIAL, 256, 0, 0, 0, 2736, 1)
    assert plan(INVERSE_VJP, 1137, k=8) == (SEQUENTIAL, 256, 0, 0, 0, 163728, 1)
    assert plan(INVERSE_VJP, 1138, k=8) == (SEQUENTIAL, 256, 0, 0, 0, 0, 0)
    assert plan(INVERSE_VJP, 2048, lds=0) == (WAVE, 256, 0, 0, 0, 163840, 0)
    # the forward operators' two segments at their smallest M, k = 8: 159744 / 72 = 2218 columns
    assert plan(CHOL, 2218, k=8) == (STREAMED, 256, 247, 2218, 0, 159696, 0)
    assert plan(CHOL, 2219, k=8) == (STREAMED, 256, 245, 2218, 0, 159696, 0)
    assert plan(INVERSE, 2219, k=8) == (STREAMED, 256, 277, 2218, 0, 159696, 0)
    # no plan asks for more than the 160 KiB a workgroup gets, whatever the override (a sparse walk; 1 <= M <= 20000 was walked exhaustively
    # against the previous launch code when the plan was written)
    for op in range(4):
        for k in range(1, 9):
            for M in list(range(1, 60)) + list(range(60, 20000, 97)) + [20000, 10 ** 6, 2 ** 30 - 1]:
                for sb in (0, 1, 2, 3):
                    plan(op, M, k=k, seg_blocks=sb)
    # argument checks of the entry itself
    assert lib.asvgp_band_launch_plan_host(CHOL, 64, 4, 1, 0, None) == BAD_ARG
    assert _band_plan(lib, 4, 64)[0] == BAD_ARG and _band_plan(lib, -1, 64)[0] == BAD_ARG
    for k in (0, 9):
        assert _band_plan(lib, CHOL, 64, k=k)[0] == UNSUPPORTED and b"bandwidth %d" % k in lib.asvgp_last_error_string()
    for M in (0, -5, 2 ** 30):
        assert _band_plan(lib, INVERSE_VJP, M)[0] == UNSUPPORTED and b"M = %d" % M in lib.asvgp_last_error_string()


KRON_PHI_FIELDS = ("status", "kernel", "grid", "threads", "gather_grid", "staging", "ncell", "ncell_pad", "clear_all", "rhs_off", "yy_off",
                   "zero")                                                  # plan12 of asvgp_kron_phi_launch_plan_host
KP_NONE, KP_POINT, KP_CELLS, KP_MFMA = range(4)                             # plan12[1]
ERR_HIP = -5
KP_FORMS = {"point": (0, 0, 0), "point_w": (0, 1, 0), "sorted": (1, 0, 0), "sorted_f32": (1, 0, 1), "sorted_w": (1, 1, 0)}   # (sorted, weighted, f32)
KP_SORTED = ("sorted", "sorted_f32", "sorted_w")


def _kron_phi_plan(lib, form, N=1000, mesh=(2, 3), k=1, m=None, atomics=0, grid=512, staging=1):
    """(status, fields by name) of asvgp_kron_phi_launch_plan_host for a mesh of mesh[0] x mesh[1] knots and order k (m = n_mesh + k - 1)"""
    m = m or (mesh[0] + k - 1, mesh[1] + k - 1)
    out = np.full(12, -99, dtype=np.int64)
    rc = lib.asvgp_kron_phi_launch_plan_host(*KP_FORMS[form], N, m[0], m[1], mesh[0], mesh[1], k, atomics, grid, staging, out.ctypes.data)
    p = dict(zip(KRON_PHI_FIELDS, (int(v) for v in out)))
    assert p["status"] == rc and p["zero"] == 0
    return rc, p


def test_kron_phi_launch_plan_follows_the_documented_rules(lib):
    """asvgp_kron_phi_launch_plan_host is the plan_kron_phi that the five asvgp_phi_accumulate_kron2d* entries call before they allocate,
    clear or launch anything (csrc/kron_phi_launch.hpp), with the two environment variables and the outcome of the allocation as
    arguments.  Every row is written down from the rules (the table of the Kronecker Phi pass): stats is
    [n_off m1 m2 | m1 m2 | 1] with n_off = k (2k + 1) + k + 1 (5 at k = 1, 25 at k = 3, 41 at k = 4); the cells are rounded up to strips of
    8; a cell leaves 14, 54, 152, 350, 702, 1274 doubles in the staging buffer at k = 1..6; the gather has one thread per (n_off + 1) m1 m2
    outputs.  A row is (kernel, grid, threads, gather grid, staging bytes, cells, padded cells, clear all, rhs offset, yy offset)."""
    def plan(form, **kw):
        rc, p = _kron_phi_plan(lib, form, **kw)
        assert rc == OK, lib.asvgp_last_error_string()
        return tuple(p[f] for f in KRON_PHI_FIELDS[1:-1])

    # N = 0 in every form: all of stats is cleared, nothing is launched
    for form in KP_FORMS:
        assert plan(form, N=0) == (KP_NONE, 0, 0, 0, 0, 2, 8, 1, 30, 36), form
        assert plan(form, N=0, atomics=1, staging=0) == (KP_NONE, 0, 0, 0, 0, 2, 8, 1, 30, 36), form
    # per point: one thread per point, at most 4096 workgroups of 256
    for N, grid in ((1, 1), (256, 1), (257, 2), (4095 * 256 + 1, 4096), (4096 * 256, 4096), (4096 * 256 + 1, 4096)):
        for form in ("point", "point_w"):
            assert plan(form, N=N) == (KP_POINT, grid, 256, 0, 0, 2, 8, 1, 30, 36), (form, N)
    assert plan("point", atomics=1, grid=7, staging=0) == plan("point") == (KP_POINT, 4, 256, 0, 0, 2, 8, 1, 30, 36)
    # sorted, 2 x 3 mesh points: 2 cells, one strip of 8, 6 (5 + 1) = 36 gather outputs
    for form in KP_SORTED:
        assert plan(form) == (KP_MFMA, 1, 512, 1, 14 * 8 * 8, 2, 8, 0, 30, 36), form
    # sorted, 66 x 66 mesh points: 4225 cells, pad 4232, 529 strips; 6 * 4356 = 26136 gather outputs = 102.1 workgroups
    big = dict(mesh=(66, 66))
    for form in KP_SORTED:
        assert plan(form, **big) == (KP_MFMA, 512, 512, 103, 14 * 4232 * 8, 4225, 4232, 0, 21780, 26136), form
        assert [plan(form, grid=g, **big)[1] for g in (600, 529, 528, 1, 0, -5)] == [529, 529, 528, 1, 1, 1], form
    # the staging buffer: doubles per padded cell (152 and 350 are the figures of asvgp_hip.h)
    assert [plan("sorted", k=k)[4] // (8 * 8) for k in range(1, 7)] == [14, 54, 152, 350, 702, 1274]
    assert plan("sorted_w", k=3) == (KP_MFMA, 1, 512, 3, 152 * 8 * 8, 2, 8, 0, 500, 520)          # m = 4 x 5: 26 * 20 = 520 outputs
    assert plan("sorted_f32", k=4) == (KP_MFMA, 1, 512, 5, 350 * 8 * 8, 2, 8, 0, 1230, 1260)      # m = 5 x 6: 42 * 30 = 1260 outputs
    # the gather clamp at order 3: 26 m^2 outputs; m = 283: 8134.04 workgroups, 284: 8191.6 -> 8192 (the last grid that is not cut), 285: 8249.4
    for m, ncell_pad, gather in ((283, 78400, 8135), (284, 78968, 8192), (285, 79528, 8192)):
        for form in KP_SORTED:
            assert plan(form, mesh=(m - 2, m - 2), k=3) == (KP_MFMA, 512, 512, gather, 152 * ncell_pad * 8, (m - 3) ** 2, ncell_pad, 0, 25 * m * m,
                                                            26 * m * m), (form, m)
    # ASVGP_KRON_PHI_ATOMICS: the per-cell kernel, which only plain fp64 has - one workgroup per cell, at most 4096, all of stats cleared
    assert plan("sorted", atomics=1) == (KP_CELLS, 2, 256, 0, 0, 2, 8, 1, 30, 36)
    assert plan("sorted", atomics=1, **big) == (KP_CELLS, 4096, 256, 0, 0, 4225, 4232, 1, 21780, 26136)
    assert plan("sorted", atomics=1, mesh=(65, 65)) == (KP_CELLS, 4096, 256, 0, 0, 4096, 4096, 1, 21125, 25350)
    for form in ("sorted_f32", "sorted_w"):
        assert plan(form, atomics=1, **big) == plan(form, **big), form
    # no room for the staging buffer: plain fp64 takes the per-cell kernel, the other two refuse
    assert plan("sorted", staging=0, **big) == plan("sorted", staging=0, atomics=1, **big) == plan("sorted", atomics=1, **big)
    rc, p = _kron_phi_plan(lib, "sorted_f32", staging=0, **big)
    assert rc == ERR_HIP and lib.asvgp_last_error_string() == b"phi_accumulate_kron2d_sorted_f32: no room for the staging buffer (4225 cells)"
    rc, p = _kron_phi_plan(lib, "sorted_w", staging=0, atomics=1, **big)
    assert rc == ERR_HIP
    assert lib.asvgp_last_error_string() == b"phi_accumulate_kron2d_sorted_weighted: no room for the staging buffer (4225 cells); the per-point entry needs none"
    # the refusals of the argument check: nothing but the status is filled
    def refused(form, **kw):
        rc, p = _kron_phi_plan(lib, form, **kw)
        assert rc != OK and not any(p[f] for f in KRON_PHI_FIELDS[1:])
        assert lib.asvgp_last_error_string().startswith(b"kron_phi_launch_plan_host: ")
        return rc

    for form in KP_FORMS:
        for k in (0, 7):
            assert refused(form, k=k) == UNSUPPORTED and b"order %d unsupported" % k in lib.asvgp_last_error_string(), (form, k)
        for mesh in ((1, 3), (2, 1), (1, 1)):
            assert refused(form, mesh=mesh, k=3) == BAD_ARG, (form, mesh)
        assert refused(form, mesh=(8, 9), k=3, m=(10, 12)) == BAD_ARG and refused(form, mesh=(8, 9), k=3, m=(11, 11)) == BAD_ARG
        assert refused(form, N=-1) == BAD_ARG
        assert b"bad argument" in lib.asvgp_last_error_string()
        # what the kernels take as int: 46341^2 = 2147488281 cells; 2 * 1073741823 = 2^31 - 2 cells fit, their 2^31 padded cells do not
        assert refused(form, mesh=(46342, 46342)) == UNSUPPORTED and b"2147488281 cells" in lib.asvgp_last_error_string(), form
        assert refused(form, mesh=(3, 1073741824)) == UNSUPPORTED and b"2147483646 cells" in lib.asvgp_last_error_string(), form
        assert refused(form, mesh=(2, 2 ** 31 - 1), k=2) == UNSUPPORTED and b"m2 = 2147483648" in lib.asvgp_last_error_string(), form
        assert refused(form, mesh=(2 ** 31, 2)) == UNSUPPORTED and b"m1 = 2147483648" in lib.asvgp_last_error_string(), form
        rc, p = _kron_phi_plan(lib, form, mesh=(9, 268435456))               # 8 * 268435455 = 2^31 - 8 cells: whole strips, the most an int holds
        assert rc == OK and p["ncell"] == p["ncell_pad"] == 2 ** 31 - 8, form
    assert lib.asvgp_kron_phi_launch_plan_host(1, 0, 0, 1000, 2, 3, 2, 3, 1, 0, 512, 1, None) == BAD_ARG
    out = np.zeros(12, dtype=np.int64)
    for sorted_, weighted in ((0, 0), (0, 1), (1, 1)):                       # fp32 storage: the plain sorted entry only
        assert lib.asvgp_kron_phi_launch_plan_host(sorted_, weighted, 1, 1000, 2, 3, 2, 3, 1, 0, 512, 1, out.ctypes.data) == BAD_ARG


KRON_ENTRIES = ("phi_accumulate_kron2d", "phi_accumulate_kron2d_sorted", "phi_accumulate_kron2d_sorted_f32")


@pytest.mark.parametrize("name", KRON_ENTRIES)
def test_accumulate_kron2d_unweighted_argument_checks(lib, name):
    """The twin of test_accumulate_kron2d_weighted_argument_checks for the three unweighted entries: the same cases, refused on the host
    with the entry's own name in front - nothing is dereferenced or launched."""
    FAKE = ctypes.c_void_p(0x1000)
    ODD = ctypes.c_void_p(0x1004 if name.endswith("f32") else 0x1008)       # off the (x1, x2) pair: 8 bytes of fp32, 16 of fp64
    sorted_ = "sorted" in name

    def call(X=FAKE, y=FAKE, N=10, start=FAKE, mesh1=FAKE, n1=8, m1=10, mesh2=FAKE, n2=9, m2=11, order=3, stats=FAKE):
        args = (X, y, N) + ((start,) if sorted_ else ()) + (mesh1, n1, 0.1, m1, mesh2, n2, 0.1, m2, order, stats, None)
        return getattr(lib, "asvgp_" + name)(*args)

    err = lambda: lib.asvgp_last_error_string().decode()
    cases = [{"X": None}, {"y": None}, {"mesh1": None}, {"mesh2": None}, {"stats": None}, {"N": -1}, {"n1": 9}, {"n2": 8}, {"X": ODD},
             {"n1": 1, "m1": 3}, {"n2": 1, "m2": 3}]                        # (a mesh of one knot has no cell)
    if sorted_:
        cases.append({"start": None})
    for kw in cases:
        assert call(**kw) == BAD_ARG, kw
        assert err().startswith(name + ": "), (kw, err())
    assert "aligned" in (call(X=ODD), err())[1]
    assert call(order=7, n1=4, n2=5) == UNSUPPORTED and err() == name + ": order 7 unsupported"
    assert call(order=0, n1=11, n2=12) == UNSUPPORTED and err() == name + ": order 0 unsupported"
    assert call(n1=46342, m1=46344, n2=46342, m2=46344) == UNSUPPORTED and err().startswith(name + ": 2147488281 cells")


def test_two_sided_factorisation_layout_invariants():
    """asvgp_amd.kronecker.twisted_layout (host logic of GPR_kron's two-sided band Cholesky): for every size both systems have nb super-blocks,
    the separator is their last block, paddings are non-negative, the interiors do not overlap and together with the separator cover
    [0, M); small matrices keep the one-sided factorisation unless forced."""
    from asvgp_amd.kronecker import twisted_layout
    seen = 0
    for M in list(range(40, 3000, 37)) + [16384, 10000, 128 * 128, 100 * 100]:
        for bw in (3, 10, 26, 36, 60, 147, 387, 404):
            for force in (None, True, False):
                lay = twisted_layout(M, bw, force)
                Bb = ((max(bw, 1) + 31) // 32) * 32
                if force is False:
                    assert lay is None
                    continue
                if lay is None:
                    nb = -(-(M + Bb) // (2 * Bb))
                    assert nb < 3 or (force is None and -(-M // Bb) < 6)
                    continue
                seen += 1
                nb, top_end, h, padt, padb = lay["nb"], lay["top_end"], lay["h"], lay["padt"], lay["padb"]
                assert lay["Bb"] == Bb and Bb >= bw and Bb % 32 == 0 and nb >= 3
                assert padt >= 0 and padb >= 0 and h == top_end - Bb and 0 <= h and top_end <= M
                assert padt + top_end == nb * Bb                      # top system: padding + columns [0, top_end)
                assert padb + (M - h) == nb * Bb                      # bottom system: padding + columns [h, M)
                assert abs(padt - padb) <= 1                          # balanced chains
                assert (nb - 1) * Bb >= padt + h and (nb - 1) * Bb >= padb + (M - top_end)   # interiors fit in front of the separator block
    assert seen > 100
    lay = twisted_layout(128 * 128, 3 * 128 + 3)
    assert lay == dict(Bb=416, nb=21, top_end=8400, h=7984, padt=336, padb=336, bw=387)

