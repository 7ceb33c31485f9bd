"""Chain sharding across the GPUs of a node.

Chains are independent Markov chains, so the population splits into contiguous blocks, one per rank, with NO
per-step communication: the device RNG is keyed by the GLOBAL chain index, so a chain's trajectory does not
depend on how many ranks there are. The only collective is the final population collect (all_gather over
RCCL/xGMI on GPUs; gloo in the CPU tests).

`Shard` is one rank's view of such a split and the owner of what a sharded run gathers at its end: per chain, per group of
consecutive chains (tempering ensembles, annealing demes, recorder slots), summed over the ranks, or broadcast from the rank
that owns a chain. Without communication every one of its operations hands its array back.
"""
import os

import numpy as np
import torch
import torch.distributed as dist

# PPDE_COLLECTIVES_AT_WORLD_1=1: run the collectives below even in a process group of ONE rank (where they are the
# identity). It lets a one-GPU box execute the RCCL path end to end -- library load, communicator set-up, host -> device
# staging, all_gather / broadcast, the way back -- before an 8-GPU node ever sees it (tests/test_host_gpu.py).
def force_at_world_1():
    """Read at every call (not at import), '' and '0' mean off -- as the library's atoi-style knobs."""
    return os.environ.get("PPDE_COLLECTIVES_AT_WORLD_1", "0") not in ("", "0")


def world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def active():
    """True when the collectives below actually communicate: more than one rank, or forced at world size 1."""
    _, ws = world()
    return ws > 1 or (force_at_world_1() and dist.is_available() and dist.is_initialized())


def shard_range(n, rank, world_size):
    """Contiguous block [lo, hi) of rank `rank`; the first n % world_size ranks hold one extra chain."""
    base, extra = divmod(n, world_size)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def all_gather_rows(t, n_global, dim=0):
    """Concatenate per-rank shards (unequal sizes allowed) along `dim` on every rank."""
    rank, ws = world()
    if not active():
        return t
    sizes = [shard_range(n_global, r, ws) for r in range(ws)]
    mx = max(hi - lo for lo, hi in sizes)
    home = t.device
    if dist.get_backend() == "nccl" and t.device.type != "cuda":   # RCCL moves device memory only
        t = t.cuda()
    t = t.movedim(dim, 0).contiguous()
    pad = torch.zeros((mx,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    pad[: t.shape[0]] = t
    bufs = [torch.empty_like(pad) for _ in range(ws)]
    dist.all_gather(bufs, pad)
    out = torch.cat([b[: hi - lo] for b, (lo, hi) in zip(bufs, sizes)], 0)
    return out.movedim(0, dim).to(home)


def broadcast_from(t, src):
    if active():
        home = t.device
        if dist.get_backend() == "nccl" and t.device.type != "cuda":
            t = t.cuda()
        dist.broadcast(t, src)
        t = t.to(home)
    return t


def sum_over_ranks(t):
    """Element-wise sum of a tensor over the ranks, on every rank (the recorder's site counts)."""
    if active():
        home = t.device
        if dist.get_backend() == "nccl" and t.device.type != "cuda":
            t = t.cuda()
        t = t.clone()
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        t = t.to(home)
    return t


def agree_from_rank0(values):
    """Rank 0's integers on every rank (random chain index, default seed): ranks that were seeded differently must
    still record the same chain and draw the same Philox stream."""
    if not active():
        return [int(v) for v in values]
    t = torch.tensor([int(v) for v in values], dtype=torch.int64)
    return [int(v) for v in broadcast_from(t, 0).tolist()]


def boundary_cut(starts, size):
    """(rank, start) of the first shard start that is no multiple of `size` -- a group of `size` consecutive chains would lie on
    two ranks --, or None when the groups split as the chains do."""
    for r, start in enumerate(starts):
        if start % size:
            return r, start
    return None


class Shard:
    """Rank `rank` of `ws` in a population of n_global chains: its block [lo, hi) of n chains, and the collect of a sharded run.
    comm False (one rank, or a run that does not shard inside an initialised process group): nothing below communicates and
    every array comes back as it went in."""

    def __init__(self, n_global, rank=0, ws=1, comm=False):
        self.n_global, self.rank, self.ws, self.comm = int(n_global), int(rank), int(ws), bool(comm)
        self.lo, self.hi = shard_range(self.n_global, self.rank, self.ws)
        self.n = self.hi - self.lo

    @property
    def starts(self):
        """First chain of every rank's block."""
        return [shard_range(self.n_global, r, self.ws)[0] for r in range(self.ws)]

    def owner(self, chain):
        """The rank whose block holds global chain `chain`."""
        return next(r for r in range(self.ws) if chain < shard_range(self.n_global, r, self.ws)[1])

    def to_global(self, local):
        """Local chain indices as int64 global ones."""
        return local.astype(np.int64) + self.lo

    def gather(self, a, dim=0, size=1):
        """Every rank's block of `a` along its chain axis `dim`, in global order. size > 1: the axis holds one entry per group
        of `size` consecutive chains (no shard start may cut a group: boundary_cut)."""
        a = np.asarray(a)
        return all_gather_rows(torch.from_numpy(a), self.n_global // size, dim=dim).numpy() if self.comm else a

    def sum(self, a):
        """Element-wise sum of `a` over the ranks (None stays None). uint64 counts travel as int64: the collectives have no
        unsigned 64-bit sum."""
        if a is None or not self.comm:
            return a
        if a.dtype == np.uint64:
            return sum_over_ranks(torch.from_numpy(a.astype(np.int64))).numpy().astype(np.uint64)
        return sum_over_ranks(torch.from_numpy(a)).numpy()

    def broadcast(self, a, src):
        """Rank src's `a` on every rank."""
        return broadcast_from(torch.from_numpy(a), src).numpy() if self.comm else a
