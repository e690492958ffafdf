"""Sequence-level data parallelism: one process per GPU, each owning different tracking windows.

Windows are independent graphs (batch size 1 per forward in the reference, utils/graph.py:117), so
the data path has NO collective; the only exchange is the gradient sum before the optimizer step.
The parameter set is tiny (55 k .. 860 k fp32), i.e. the all-reduce is latency bound: all gradients
live in ONE contiguous fp32 bucket (each `p.grad` is a view into it, so autograd accumulates in
place and nothing is packed or unpacked) and ONE `all_reduce(SUM)` (RCCL over xGMI with the `nccl`
backend; `gloo` in the CPU tests) is issued per step.  BatchNorm running statistics stay per rank,
as in the reference (it has no SyncBN).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
import torch.distributed as dist


class GradBucket:
    """Flat gradient storage for a module; `p.grad` of every parameter aliases a slice of `flat`."""

    def __init__(self, module: torch.nn.Module):
        params = [p for p in module.parameters() if p.requires_grad]
        if not params:
            raise ValueError('module has no trainable parameters')
        dev, dt = params[0].device, torch.float32
        n = sum(p.numel() for p in params)
        self.flat = torch.zeros(n, dtype=dt, device=dev)
        self.params: List[torch.nn.Parameter] = params
        o = 0
        for p in params:
            p.grad = self.flat[o:o + p.numel()].view_as(p)
            o += p.numel()
        # the bucket owns every p.grad for the module's lifetime, so the HIP backward may add into it directly
        # (functional.INPLACE_GRADS: plain loss.backward() only -- no hooks / DDP / torch.autograd.grad)
        if hasattr(module, 'inplace_param_grads'):
            module.inplace_param_grads = True

    def zero(self) -> None:
        """zero_grad(set_to_none=False) in one launch: every p.grad is a slice of `flat`."""
        self.flat.zero_()

    def check_alias(self) -> bool:
        """True while every p.grad still aliases the bucket (zero_grad(set_to_none=True) breaks it)."""
        o = 0
        for p in self.params:
            if p.grad is None or p.grad.data_ptr() != self.flat.data_ptr() + 4 * o:
                return False
            o += p.numel()
        return True


def allreduce_grads(module: torch.nn.Module, bucket: GradBucket, world: int, average: bool = True) -> None:
    """Sum the gradient bucket over ranks and average it (one collective).  average=False leaves the plain sum in the
    bucket: `BucketAdam.step(grad_scale=1 / world)` folds the division into the optimizer's launch (same bits)."""
    if not bucket.check_alias():
        raise RuntimeError('parameter gradients no longer alias the bucket; use zero_grad(set_to_none=False)')
    dist.all_reduce(bucket.flat, op=dist.ReduceOp.SUM)
    if average:
        bucket.flat.mul_(1.0 / world)


def shard_windows(n_windows: int, rank: int, world: int, edge_counts: Optional[Sequence[int]] = None) -> List[int]:
    """The windows (tracking chunks / sequences) rank `rank` of `world` owns.

    Without `edge_counts`: windows {i : i mod world == r} (the reference shuffles chunks, train.py:22, so any fixed
    deal is balanced in expectation).  With `edge_counts[i]` = sum of E over the forward calls of window i (the unit of
    the metric and of the work): longest-processing-time greedy -- windows in descending order of work, each to the
    rank with the least work so far, ties to the lowest rank -- so that every rank's step takes about the same time
    (graph sizes vary by an order of magnitude between KITTI and BDD scenes).  Deterministic: every rank
    computes the same partition from the same counts; each rank's list is returned in ascending window order.

    Contract of the balanced deal: ranks may hold DIFFERENT NUMBERS of windows (a rank can even get none), so the training
    loop must issue exactly ONE `allreduce_grads` per rank and optimizer step over the rank's whole shard -- never one per
    window -- and the shard's loss must be a SUM over its windows (`allreduce_grads` divides the summed gradient by `world`,
    not by a window count): a per-rank mean would weight windows of small shards more.  bench.py's step does both."""
    if edge_counts is None:
        return list(range(rank, n_windows, world))
    if len(edge_counts) != n_windows:
        raise ValueError(f'shard_windows: {len(edge_counts)} edge counts for {n_windows} windows')
    if not 0 <= rank < world:
        raise ValueError(f'shard_windows: rank {rank} of {world}')
    import heapq
    order = sorted(range(n_windows), key=lambda i: (-int(edge_counts[i]), i))
    heap = [(0, r) for r in range(world)]              # (work so far, rank)
    mine: List[int] = []
    for i in order:
        load, r = heapq.heappop(heap)
        if r == rank:
            mine.append(i)
        heapq.heappush(heap, (load + int(edge_counts[i]), r))
    return sorted(mine)
