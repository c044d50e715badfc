"""Multi-GPU layout of the batched step: one process per GPU, lanes sharded contiguously.

Worlds are independent, so the physics never exchanges data between GPUs.
Rank r owns global lanes [r*L, (r+1)*L) and passes ``lane_offset = r*L`` to ``mrp_create``;
the device RNG is keyed by the global lane id, so every lane's trajectory is identical at any
GPU count.  The rollout's only collective is the per-step hand-over of (obs, reward, done) to the
policy rank: each rank packs them into ONE contiguous float32 buffer [L, obs_dim + 2] (done as
0.0/1.0) and ``torch.distributed.gather``s it to rank 0 (RCCL turns this into root receives +
peer sends, one message per peer over its own xGMI link).  With a policy replica on every
rank use ``all_gather`` instead (``StepGather(..., to_all=True)``).

Training with a policy replica and a rollout buffer on every rank needs one more collective, per
minibatch: ``GradExchange`` all-gathers every rank's flat gradient and statistics into one ``[R, stride]``
buffer in rank order, which ``DevicePPO`` combines in that fixed order (``ppo.combine_ref``), so every
replica applies the same bits.  ``DeviceVecNormalize(shard=...)`` uses the same exchange with float64 blocks
(``dtype=torch.float64``), once per ``reset`` / ``step``, for the column moments of its running statistics.
"""
from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class Shard:
    rank: int
    world: int
    lanes_per_rank: int

    @property
    def lane_offset(self) -> int:
        return self.rank * self.lanes_per_rank

    @property
    def global_lanes(self) -> int:
        return self.world * self.lanes_per_rank

    def lanes(self) -> range:
        return range(self.lane_offset, self.lane_offset + self.lanes_per_rank)


def shard_from_env(lanes_per_rank: int) -> Shard:
    import os
    return Shard(int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), lanes_per_rank)


def agree(who, what, value, world, group=None):
    """``ValueError`` on every rank unless all ``world`` ranks hold the same ``value`` (a tuple named by ``what``), so
    that they go on to enqueue the same collectives: one gather of the values when ``world > 1``, else no collective."""
    if world > 1:
        import torch.distributed as dist
        seen = [None] * world
        dist.all_gather_object(seen, value, group=group)
        if any(tuple(v) != tuple(seen[0]) for v in seen):
            raise ValueError(f"{who}: {what} differs across ranks: {seen}")


def broadcast_array(array, src, group, device):
    """Rank ``src``'s numpy ``array`` on every rank, bit for bit, as a new array of the same dtype and shape
    (every rank passes one of that dtype and shape).  It travels on ``device`` under an nccl group and on the
    host otherwise."""
    import numpy as np
    import torch
    import torch.distributed as dist
    buf = torch.from_numpy(np.array(array))      # a contiguous copy: the caller's array is not written
    if dist.get_backend(group) == "nccl":
        buf = buf.to(device)
    dist.broadcast(buf, src, group=group)
    return buf.cpu().numpy()


class StepGather:
    """Packs one step's outputs of this rank and gathers every rank's block to rank 0."""

    def __init__(self, shard: Shard, obs_dim: int, device, group=None, to_all: bool = False, host_stage: bool = False,
                 force_collective: bool = False):
        """``host_stage``: the collective runs on host memory (a CPU backend such as gloo): the packed
        block is copied from the device into a pinned host buffer and gathered there; the receive
        buffer is on the host too.  ``force_collective``: call the collective at world size 1 too
        (a one-GPU box then executes the RCCL gather on device tensors; bench.py --force-collective)."""
        import torch
        self.shard, self.obs_dim, self.group, self.to_all = shard, obs_dim, group, to_all
        self.force_collective = force_collective
        L = shard.lanes_per_rank
        self.packed = torch.zeros((L, obs_dim + 2), dtype=torch.float32, device=device)
        self.host = torch.zeros((L, obs_dim + 2), dtype=torch.float32).pin_memory() if host_stage else None
        root = shard.rank == 0 or to_all
        # the receive blocks are row slices of ONE [G, obs_dim + 2] buffer: the gathered step is
        # contiguous on arrival, no concatenation afterwards
        rdev = "cpu" if host_stage else device
        self.full = torch.zeros((shard.global_lanes, obs_dim + 2), dtype=torch.float32, device=rdev) if root else None
        self.blocks = list(self.full.split(L, dim=0)) if root else None

    def pack(self, obs, reward, done):
        import torch
        # one fused copy into the packed rows [obs | reward | done]
        torch.cat((obs, reward.unsqueeze(1), done.unsqueeze(1).to(torch.float32)), dim=1, out=self.packed)
        return self.packed

    def __call__(self, obs, reward, done):
        """Returns (obs [G, O], reward [G], done [G]) over all G global lanes on rank 0 (every
        rank with to_all), None elsewhere.  Single-process: no collective.  The returned tensors
        are views of this gatherer's receive buffer, valid until its next call."""
        import torch.distributed as dist
        p = self.pack(obs, reward, done)
        if self.host is not None:
            self.host.copy_(p)   # synchronous device -> pinned host copy: the CPU collective reads it next
            p = self.host
        if self.shard.world == 1 and not self.force_collective:
            full = p
        else:
            if self.to_all:
                dist.all_gather(self.blocks, p, group=self.group)
            else:
                dist.gather(p, self.blocks if self.shard.rank == 0 else None, dst=0, group=self.group)
            if self.blocks is None:
                return None
            full = self.full
        O = self.obs_dim
        return full[:, :O], full[:, O], full[:, O + 1] != 0


class GradExchange:
    """All-gathers one flat float32 block per rank (``DevicePPO``'s gradient before clipping and its five
    statistics) into ``parts`` ``[world, part_stride]``, row ``r`` from rank ``r``; ``part_stride`` is
    ``n_floats`` rounded up to a multiple of 64.  The owner writes its block into ``mine`` ``[part_stride]``
    and calls the exchange; every rank then holds the same ``parts``.  ``dtype=torch.float64`` makes the
    blocks float64 (``DeviceVecNormalize``'s column moments); the rows arrive bit for bit either way."""

    def __init__(self, shard: Shard, n_floats: int, device, group=None, host_stage: bool = False, force_collective: bool = False,
                 dtype=None):
        """On a device backend the collective is ``all_gather_into_tensor(parts, mine)`` on device tensors,
        asynchronous on the current stream.  ``host_stage``: the collective runs on pinned host buffers (a
        CPU backend such as gloo), with a synchronous device -> host copy before it and a host -> device
        copy after it.  ``force_collective``: call the collective at world size 1 too; without it world
        size 1 only copies ``mine`` into ``parts[0]``."""
        import torch
        self.shard, self.n_floats, self.group, self.force_collective = shard, int(n_floats), group, force_collective
        if self.n_floats < 1:
            raise ValueError("GradExchange: n_floats must be >= 1")
        self.dtype = dtype = torch.float32 if dtype is None else dtype
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"GradExchange: dtype is {dtype}, expected torch.float32 or torch.float64")
        self.world = shard.world
        self.part_stride = -(-self.n_floats // 64) * 64
        self.mine = torch.zeros(self.part_stride, dtype=dtype, device=device)
        self.parts = torch.zeros((self.world, self.part_stride), dtype=dtype, device=device)
        self.host_mine = torch.zeros(self.part_stride, dtype=dtype).pin_memory() if host_stage else None
        self.host_parts = torch.zeros((self.world, self.part_stride), dtype=dtype).pin_memory() if host_stage else None

    def __call__(self):
        """Returns ``parts`` with every rank's ``mine`` in rank order, valid until the next call."""
        if self.world == 1 and not self.force_collective:
            self.parts[0].copy_(self.mine)
            return self.parts
        import torch.distributed as dist
        if self.host_mine is not None:
            self.host_mine.copy_(self.mine)   # synchronous device -> pinned host copy: the CPU collective reads it next
            dist.all_gather_into_tensor(self.host_parts.view(-1), self.host_mine, group=self.group)
            self.parts.copy_(self.host_parts)
        else:
            dist.all_gather_into_tensor(self.parts.view(-1), self.mine, group=self.group)   # flat: rank r's block is row r
        return self.parts
