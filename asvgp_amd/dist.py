"""Multi-GPU data parallelism for the Phi pass: contiguous N-shards per rank, ONE sum-reduction of the
packed [(k+1) M band | M D rhs | 1 yy] fp64 buffer (+ the row count) over RCCL (torch.distributed 'nccl' backend on
ROCm) - or gloo on CPU in the tests.  The reference has no distributed code; the statistics are plain sums over
datapoints (gpr.py:41-44) which is what makes this exact up to fp64 summation order."""
import torch
import torch.distributed as dist


def shard_bounds(N, world_size, rank):
    """contiguous, balanced [lo, hi) shard of N rows; even shard starts keep the 16-B vector-load path aligned."""
    per = (N + world_size - 1) // world_size
    per += per & 1
    lo = min(rank * per, N)
    hi = min(lo + per, N)
    return lo, hi


def allreduce_stats(stats, n_local, group=None, wstats=None):
    """Sum the packed statistics buffer and the local row count across ranks.  Returns global N (python int).
    One collective for the payload (98 312 B at M=2048, k=4); the count rides in a second 8-byte all-reduce.
    wstats (weighted models): this rank's [sum w, sum log w, N+] (3 doubles, device or host) rides with the count - the second
    collective is then 32 bytes, the payload collective is unchanged - and (N, [the three global sums]) is returned."""
    scalars = [float(n_local)]                 # what the second collective carries: the count, then the three weight sums
    if wstats is not None:
        w = torch.as_tensor(wstats, dtype=torch.float64).reshape(-1)
        if w.numel() != 3:
            raise ValueError("allreduce_stats: wstats must hold [sum w, sum log w, N+]")
        scalars += w.tolist()
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(stats, op=dist.ReduceOp.SUM, group=group)
        n = torch.tensor(scalars, dtype=torch.float64, device=stats.device)
        dist.all_reduce(n, op=dist.ReduceOp.SUM, group=group)
        scalars = n.tolist()
    n_global = int(round(scalars[0]))
    return n_global if wstats is None else (n_global, scalars[1:])
