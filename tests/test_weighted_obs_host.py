"""CPU: the per-observation-weight entry points (asvgp_phi_accumulate_1d_weighted, asvgp_phi_weighted_workspace_bytes,
asvgp_set_weight_sums, asvgp_phi_accumulate_kron2d_weighted, asvgp_phi_accumulate_kron2d_sorted_weighted) are exported with prototypes,
their argument checks fail loudly on the host before anything is launched, and the host-side logic of the Python surface
(weight validation, the widened count collective, the refusals of the models without a weighted Phi pass) needs no GPU."""
import ctypes
import inspect

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from asvgp_amd import build, _lib
    build.build(verbose=False)
    return _lib.get_lib()


NAMES = ("asvgp_phi_accumulate_1d_weighted", "asvgp_phi_weighted_workspace_bytes", "asvgp_set_weight_sums",
         "asvgp_phi_accumulate_kron2d_weighted", "asvgp_phi_accumulate_kron2d_sorted_weighted")


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
BIG = 1 << 40


def test_weighted_workspace_query(lib):
    for M, k, D in ((2048, 4, 1), (8, 1, 1), (5000, 6, 3), (2, 1, 1)):
        own, base = lib.asvgp_phi_weighted_workspace_bytes(M, k, D), lib.asvgp_phi_workspace_bytes(M, k, D)
        assert own >= base                                   # (a model keeps one workspace for both entries)
        assert own >= 8 * 256 * ((k + 2) * M + 1 + 4 + 1)    # 256 partial images, records of the weight sums, column ranges
    assert lib.asvgp_phi_workspace_bytes(2048, 4, 1) == 8 * 256 * (7 * 2048 + 1)     # the existing query keeps its values
    assert lib.asvgp_phi_weighted_workspace_bytes(0, 4, 1) == 0 and lib.asvgp_phi_weighted_workspace_bytes(64, 7, 1) == 0


def _acc(lib, x=FAKE, y=FAKE, w=FAKE, N=10, D=1, mesh=FAKE, n_mesh=13, delta=0.1, order=4, M=16, stats=FAKE, wstats=FAKE, ws=FAKE, wsb=BIG):
    return lib.asvgp_phi_accumulate_1d_weighted(None, x, y, w, N, D, mesh, n_mesh, delta, order, M, stats, wstats, ws, wsb, None)


def test_accumulate_1d_weighted_argument_checks(lib):
    for kw in ({"x": None}, {"y": None}, {"w": None}, {"mesh": None}, {"stats": None}, {"wstats": None}, {"N": -1}, {"D": 0}, {"M": 0},
               {"delta": 0.0}, {"delta": float("nan")}, {"n_mesh": 12}, {"n_mesh": 1, "M": 4}):
        assert _acc(lib, **kw) == -1, kw
        assert "phi_accumulate_1d_weighted" in _err(lib)
    assert _acc(lib, order=7, n_mesh=10) == -2 and "order 7" in _err(lib)
    assert _acc(lib, order=0, n_mesh=17) == -2
    assert _acc(lib, ws=None) == -4 and "workspace too small" in _err(lib)            # ASVGP_ERR_WORKSPACE
    assert _acc(lib, wsb=lib.asvgp_phi_weighted_workspace_bytes(16, 4, 1) - 8) == -4
    # the fixed-point algorithms (3, 5) have no weighted form; 6 forced where the register-moment kernel does not apply (here: D = 3):
    # refused before any launch
    try:
        assert lib.asvgp_set_phi_algorithm(None, 6) == 0
        assert _acc(lib, D=3) == -2 and "register moments" in _err(lib)
        for algo, word in ((3, "fixed point"), (5, "fixed point")):
            assert lib.asvgp_set_phi_algorithm(None, algo) == 0
            assert _acc(lib) == -2, algo
            assert "phi_accumulate_1d_weighted" in _err(lib) and word in _err(lib) and "algorithm %d" % algo in _err(lib)
    finally:
        assert lib.asvgp_set_phi_algorithm(None, 0) == 0


def test_set_weight_sums_argument_checks(lib):
    for bad in ((10.5, 10.0, 0.0), (float("nan"), 1.0, 0.0), (10.0, -1.0, 0.0), (10.0, float("inf"), 0.0), (10.0, float("nan"), 0.0),
                (10.0, 12.0, float("nan")), (10.0, 12.0, float("inf")), (1e17, 1.0, 0.0)):
        assert lib.asvgp_set_weight_sums(None, *bad) == -1, bad
        assert "set_weight_sums" in _err(lib)
    assert lib.asvgp_set_weight_sums(None, 10.0, 12.5, -3.0) == 0
    assert lib.asvgp_set_weight_sums(None, 0.0, 0.0, 0.0) == 0                        # every row masked: a valid (empty) model
    assert lib.asvgp_set_weight_sums(None, -1.0, 0.0, 0.0) == 0                       # back to the unweighted bound


def _kron(lib, sorted_, X=FAKE, y=FAKE, w=FAKE, N=10, start=FAKE, mesh1=FAKE, n1=8, m1=10, mesh2=FAKE, n2=9, m2=11, order=3, stats=FAKE, wstats=FAKE):
    if sorted_:
        return lib.asvgp_phi_accumulate_kron2d_sorted_weighted(X, y, w, N, start, mesh1, n1, 0.1, m1, mesh2, n2, 0.1, m2, order, stats, wstats, None)
    return lib.asvgp_phi_accumulate_kron2d_weighted(X, y, w, N, mesh1, n1, 0.1, m1, mesh2, n2, 0.1, m2, order, stats, wstats, None)


@pytest.mark.parametrize("sorted_", [False, True])
def test_accumulate_kron2d_weighted_argument_checks(lib, sorted_):
    name = "phi_accumulate_kron2d_sorted_weighted" if sorted_ else "phi_accumulate_kron2d_weighted"
    cases = [{"X": None}, {"y": None}, {"w": None}, {"mesh1": None}, {"mesh2": None}, {"stats": None}, {"wstats": None}, {"N": -1},
             {"n1": 9}, {"n2": 8}, {"X": ODD}]
    if sorted_:
        cases.append({"start": None})
    for kw in cases:
        assert _kron(lib, sorted_, **kw) == -1, kw
        assert name in _err(lib)
    assert "aligned" in (_kron(lib, sorted_, X=ODD), _err(lib))[1]
    assert _kron(lib, sorted_, order=7, n1=4, n2=5) == -2 and "order 7" in _err(lib)


# ------------------------------------------------------------------------------------------------ Python surface, host-side logic
def test_weight_validation_names_the_first_bad_row():
    from asvgp_amd.gpr import _predictive_weights, _prepare_weights
    cpu = torch.device("cpu")
    w = _prepare_weights(np.arange(6, dtype=np.float32).reshape(6, 1), 6, cpu, "GPR_1d")
    assert w.dtype == torch.float64 and tuple(w.shape) == (6,) and w.is_contiguous()
    assert _prepare_weights([0, 1, 2], 3, cpu, "GPR_1d").tolist() == [0.0, 1.0, 2.0]      # zeros are valid: absent rows
    for bad in (-1e-300, float("nan"), float("inf"), float("-inf")):
        w = np.ones(9)
        w[4] = bad
        w[7] = -1.0
        with pytest.raises(ValueError, match="GPR_kron.*row 4"):
            _prepare_weights(w, 9, cpu, "GPR_kron")
    for shape in ((5,), (6, 2), (2, 3), (1, 6)):
        with pytest.raises(ValueError, match="shape"):
            _prepare_weights(np.ones(shape), 6, cpu, "GPR_1d")
    assert _predictive_weights(torch.ones(4), 4).shape == (4, 1)
    for bad in (np.zeros(4), -np.ones(4), np.full(4, np.nan), np.ones(3)):
        with pytest.raises(ValueError):
            _predictive_weights(bad, 4)


def test_weights_are_keyword_only_behind_the_existing_parameters():
    import asvgp_amd as A
    for cls in (A.GPR_1d, A.GPR_kron, A.GPR_additive):
        sig = inspect.signature(cls.__init__)
        names = list(sig.parameters)
        assert names[-1] == "weights" and sig.parameters["weights"].kind is inspect.Parameter.KEYWORD_ONLY
        assert sig.parameters["weights"].default is None
        assert names[1:6] == ["data", names[2], names[3], "process_group", "distributed"]     # no positional call changes meaning
    for name in ("predict_y", "predict_log_density"):
        p = inspect.signature(getattr(A.GPR_1d, name)).parameters
        assert list(p)[-1] == "weights" and p["weights"].default is None


def test_models_without_a_weighted_phi_pass_refuse_before_anything_is_launched():
    """GPR_additive and GPR_kron with d != 2 raise NotImplementedError naming the limitation - on host tensors and fake bases, so
    nothing can have been launched."""
    import asvgp_amd as A

    class FakeBasis:
        device = torch.device("cpu")
        order, m = 3, 6

    X3, y = np.zeros((10, 3)), np.zeros((10, 1))
    with pytest.raises(NotImplementedError, match="d = 2"):
        A.GPR_kron((X3, y), [A.Matern32()] * 3, [FakeBasis()] * 3, weights=np.ones(10))
    with pytest.raises(NotImplementedError, match="GPR_additive"):
        A.GPR_additive((X3[:, :2], y), [A.Matern32()] * 2, [FakeBasis()] * 2, weights=np.ones(10))


def test_allreduce_stats_carries_the_weight_sums():
    """single process: no collective, (N, the three sums) come back; without wstats the return value is the row count, as before"""
    from asvgp_amd.dist import allreduce_stats, shard_bounds
    stats = torch.arange(5, dtype=torch.float64)
    assert allreduce_stats(stats, 17) == 17
    n, ws = allreduce_stats(stats, 17, wstats=torch.tensor([20.5, -3.25, 12.0], dtype=torch.float64))
    assert n == 17 and ws == [20.5, -3.25, 12.0]
    n, ws = allreduce_stats(stats, 17, wstats=[1.0, 2.0, 3.0])
    assert n == 17 and ws == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        allreduce_stats(stats, 17, wstats=[1.0, 2.0])
    assert stats.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    # weights shard with the rows: contiguous, balanced, covering
    N = 1001
    w = np.arange(N, dtype=np.float64)
    parts = [w[slice(*shard_bounds(N, 4, r))] for r in range(4)]
    assert np.array_equal(np.concatenate(parts), w)


def test_two_process_gloo_collective_sums_the_weight_sums():
    """two CPU ranks over gloo: the payload is summed once, the second collective carries [n, sum w, sum log w, N+]"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 32600 + (__import__("os").getpid() % 2000)
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, n, ws, stats in res:
        assert n == 30 and ws == [3.5, -1.0, 25.0] and stats == [3.0, 6.0]


def _gloo_worker(rank, world, port, q):
    import os
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from asvgp_amd.dist import allreduce_stats
    stats = torch.tensor([1.0, 2.0], dtype=torch.float64) * (rank + 1)
    n, ws = allreduce_stats(stats, 10 + 10 * rank, dist.group.WORLD, wstats=[1.0 + 1.5 * rank, -0.5, 12.0 + rank])
    q.put((rank, n, ws, stats.tolist()))
    dist.barrier()
    dist.destroy_process_group()
