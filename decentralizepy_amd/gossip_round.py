"""What the whole-topology round engines (gossip.py, gossip_jwins.py, gossip_jwins_batch.py,
gossip_subsampling.py, gossip_epidemic.py, gossip_choco.py, gossip_quant.py, gossip_stc.py,
gossip_topkacc.py, gossip_fft.py) share:
``ShardedRound``, the sharding of the nodes over the ranks, and ``PackedRowRound``, the packed row
per node that one all-gather exchanges."""
import math

import numpy as np
import torch


def up4(v):
    """v rounded up to a multiple of 4 (words: rows and slots stay 16-byte aligned)."""
    return -(-int(v) // 4) * 4


def shard(n_nodes, world, rank):
    """Contiguous node block of `rank` and the padded per-rank count for the all-gather."""
    per = math.ceil(n_nodes / world)
    lo = min(rank * per, n_nodes)
    hi = min(lo + per, n_nodes)
    return lo, hi, per


class ShardedRound:
    """Nodes [lo, hi) of a topology of ``n_nodes`` on rank ``rank`` of ``world``; every rank's
    block is padded to ``per`` rows for the all-gather."""

    def __init__(self, adj, x_init, rank, world, group, device):
        """adj: adjacency sets of all nodes; x_init: (hi - lo, N), this rank's nodes' models."""
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside a world of {world}")
        self.adj, self.n_nodes = adj, len(adj)
        self.rank, self.world, self.group = rank, world, group
        # the exchange runs through the collectives with more than one rank, or whenever the
        # caller hands over a process group (one rank too: the RCCL path then runs as a loopback,
        # tests/test_gpu_rccl.py); one rank without a group exchanges in place.  So not coll means
        # world == 1, lo == 0 and per == n_nodes: a node's number is its row in either layout
        self.coll = world > 1 or group is not None
        self.lo, self.hi, self.per = shard(self.n_nodes, world, rank)
        if x_init.shape[0] != self.hi - self.lo:
            raise ValueError(f"x_init holds {x_init.shape[0]} rows, rank {rank} owns "
                             f"{self.hi - self.lo} nodes")
        self.N = x_init.shape[1]
        self.device = device or x_init.device
        self.round = 0

    @property
    def m(self):
        """The owned-node count."""
        return self.hi - self.lo

    def all_gather(self, recv, send):
        import torch.distributed as dist  # looked up per call: the tests patch the module
        dist.all_gather_into_tensor(recv, send, group=self.group)


class PackedRowRound(ShardedRound):
    """One packed int32 row per node, ``[count (int64), status, 0 | the engine's slots]``: ``send``
    holds this rank's ``per`` rows, ``recv`` every rank's after the all-gather (None without
    collectives), ``guard`` every row's status word, contiguous, as the guarded folds read them."""

    HEADER = 4  # int32 words in front of a row's slots: the int64 count, the status word, 0

    def _alloc_rows(self, row_words):
        self.row_words = W = int(row_words)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.send = torch.zeros(self.per, W, **i32)
        self.recv = torch.zeros(self.per * self.world, W, **i32) if self.coll else None
        self.guard = torch.zeros(self.per * self.world, **i32)
        self._guard_host = torch.zeros(self.per * self.world, dtype=torch.int32,
                                       pin_memory=self.device.type == "cuda")

    @property
    def rows(self):
        """The rows the folds read, indexed by node number: every node's after the all-gather,
        this rank's in place."""
        return self.recv if self.coll else self.send

    def _row(self, q):
        return self.rows[q]

    @staticmethod
    def _count_of(row):
        """The int64 count in a row's header.  Blocks."""
        return int(row[:2].view(torch.int64).item())

    def exchange(self):
        """ONE all-gather of the packed rows; then the status words of every row, contiguous."""
        if self.coll:
            self.all_gather(self.recv, self.send)
        self.guard.copy_(self.rows[:, 2])

    def _guard_to_host(self):
        """Enqueues the status words' copy to pinned host memory; the engine says when to wait."""
        self._guard_host.copy_(self.guard, non_blocking=self.device.type == "cuda")

    def _bad_nodes(self):
        """Node numbers whose status word is nonzero on the host (the padded rows excluded)."""
        return np.flatnonzero(self._guard_host.numpy()[:self.n_nodes]).tolist()
