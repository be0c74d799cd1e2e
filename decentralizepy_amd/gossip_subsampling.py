"""One synchronous SubSampling gossip round of a whole topology on the GPU.

In the reference every node is a process whose ``sharing/SubSampling.py`` draws a Bernoulli mask
``torch.rand(n, generator=g) <= alpha`` from ``g.manual_seed(self.seed + communication_round)``
(:129-161), sends ``{"seed", "alpha", "params": concated[mask]}`` and counts the shared
parameters; every receiver rebuilds the mask from the seed (:235-308) and folds the payloads with
Metro-Hastings weights over its own model (``sharing/Sharing.py:156-190``).

This engine keeps every node's flat model resident in HBM, shards the nodes over the ranks like
``gossip.GossipRound`` and runs a round of all owned nodes with one launch per phase:
``dpz_mt_mask_batch`` (a grid of chunks x nodes: one mask alone leaves most of the machine idle),
``dpz_mask_gather_nodes`` into fixed slots, one ``all_gather_into_tensor`` of a packed row per
node, and ``dpz_mask_decode_average_nodes`` guarded by the gathers' status words.  The packed row
carries the mask words and the rank table along with the values: receivers do NOT rebuild remote
masks (the reference's wire carries only the seed), trading about n / 8 + n / 16 bytes per node
over xGMI for the latency-bound mask kernel of every remote node on every rank.

The encode / fold callables are injectable so the sharding and exchange logic can be tested with
the CPU gloo backend; the defaults are the HIP codec (no CPU fallback).
"""
import math

import torch

from .gossip import mh_weights
from .gossip_round import PackedRowRound, up4

HEADER = PackedRowRound.HEADER


def slot_capacity(n, alpha):
    """Values a node's slot holds: ``min(n, ceil(alpha n + 8 sqrt(alpha n (1 - alpha))))`` rounded
    up to a multiple of 4.  The mask's count is Binomial(n, p) with p the 24-bit threshold's
    probability (within 2^-24 of alpha): eight standard deviations put an overflow around 1e-15 per
    mask.  A mask that does exceed the slot is reported by the round, never truncated silently."""
    a = float(alpha)
    cap = min(int(n), math.ceil(a * n + 8.0 * math.sqrt(max(0.0, a * n * (1.0 - a)))))
    return up4(max(cap, 1))


class SubSamplingRound(PackedRowRound):
    """Nodes [lo, hi) of a topology on this rank; ``step()`` runs one SubSampling round of every
    node.  Node i is uid i; ``seeds[i]`` is its plugin's ``self.seed`` (the reference draws it from
    the random device; given here so that a run is reproducible), the mask of round t comes from
    ``seeds[i] + t``."""

    def __init__(self, adj, x_init, alpha, seeds, rank=0, world=1, group=None, device=None,
                 layerwise=False, slot_cap=None, encode=None, fold=None, **unknown):
        """adj: adjacency sets (``gossip.read_edges``); x_init: (hi - lo, N) fp32 tensor, this
        rank's nodes' flat models; seeds: one integer per node of the WHOLE topology.
        layerwise: no counter update (the reference's TODO, SubSampling.py:129-147).
        ``encode(x, seed, alpha, counter or None) -> values`` and ``fold(local, [(seed, alpha,
        values)], weights, w_self, out)`` are injectable (CPU tests)."""
        if unknown:
            raise ValueError(f"unknown arguments {sorted(unknown)}: the peer and reduce-scatter "
                             "exchanges, full shares and payload compression are not implemented")
        if (encode is None) != (fold is None):
            raise ValueError("encode and fold are injected together")
        if len(seeds) != len(adj):
            raise ValueError("seeds must hold one integer per node of the topology")
        if not 0.0 < float(alpha) <= 1.0:
            raise ValueError("alpha must lie in (0, 1]")
        super().__init__(adj, x_init, rank, world, group, device)
        m, N = self.m, self.N
        self.alpha = float(alpha)
        self.seeds = [int(s) for s in seeds]
        self.layerwise = bool(layerwise)
        self._hip = encode is None
        self._encode, self._fold = encode, fold
        self.cap = up4(slot_cap) if slot_cap is not None else slot_capacity(N, self.alpha)
        self.x = x_init.contiguous().clone()
        self.out = torch.empty_like(self.x)
        self.counter = torch.zeros(m, N, dtype=torch.int32, device=self.device)
        if self._hip:
            from . import codec
            self._mw, self._re = up4(codec.mask_words(N)), up4(codec.mt_rank_entries(N))
            self._ws = codec.Workspace(self.device)
        else:
            self._mw = self._re = 0  # the injected fold rebuilds the masks from the seeds
        # a node's packed row: [count (int64), status, 0 | cap values | mask words | rank table]
        self._alloc_rows(HEADER + self.cap + self._mw + self._re)
        self._count = torch.zeros(max(1, self.per), dtype=torch.int64, device=self.device)
        self.weights = [mh_weights(adj, i) for i in range(self.lo, self.hi)]
        self._tabs = {}

    # ---- views of the packed rows ---------------------------------------------------------------
    def _vals(self, rows):
        return rows[..., HEADER:HEADER + self.cap].view(torch.float32)

    def _masks(self, rows):
        o = HEADER + self.cap
        return rows[..., o:o + self._mw]

    def _ranks(self, rows):
        o = HEADER + self.cap + self._mw
        return rows[..., o:o + self._re]

    def payload(self, q):
        """``(seed, alpha, params)`` of node q's payload of the last round, in the wire dict's
        terms (any node after an all-gather, an owned one otherwise).  Reads the count: blocks."""
        row = self._row(q)
        return (self.seeds[q] + self.round - 1, self.alpha,
                self._vals(row)[:min(self._count_of(row), self.cap)])

    # ---- the legs of a round --------------------------------------------------------------------
    def masks(self):
        """The owned nodes' masks of this round into their rows, one launch per phase."""
        m = self.m
        if not self._hip or not m:
            return
        from . import codec
        codec.mt_mask_batch([self.seeds[q] + self.round for q in range(self.lo, self.hi)],
                            [self.alpha] * m, self.N, self.device,
                            mask=self._masks(self.send[:m]), rank_tab=self._ranks(self.send[:m]),
                            count=self._count, workspace=self._ws)

    def gather(self):
        """Every owned node's ``x[mask]`` into its slot, the counters, the rows' headers."""
        m = self.m
        if not m:
            return
        if not self._hip:
            for j in range(m):
                q = self.lo + j
                vals = torch.as_tensor(self._encode(
                    self.x[j], self.seeds[q] + self.round, self.alpha,
                    None if self.layerwise else self.counter[j]), dtype=torch.float32)
                k = min(vals.numel(), self.cap)
                self._vals(self.send[j])[:k] = vals[:k]
                self._count[j] = vals.numel()
                self.send[j, 2] = int(vals.numel() > self.cap)
        else:
            from . import codec
            key = ("gather", self.x.data_ptr())
            if key not in self._tabs:  # the models swap with the fold output: two tables
                rows = self.send[:m]
                self._tabs[key] = codec.gather_node_table(
                    self.x, self._masks(rows), self._ranks(rows), self._vals(rows), self._count,
                    rows[:, 2], None if self.layerwise else self.counter)
            codec.mask_gather_nodes(self._tabs[key], self.N, self.cap)
        self.send[:m, :2].copy_(self._count[:m].view(torch.int32).view(m, 2))

    def _dests(self):
        """Per owned node: (local, out, w_self, [(mask, rank_tab, vals, w)]) over the rows."""
        rows = self.rows
        dests = []
        for j, (nbrs, w, w_self) in enumerate(self.weights):
            pays = []
            for q, wq in zip(nbrs, w):
                r = rows[q]
                pays.append((self._masks(r), self._ranks(r), self._vals(r), wq))
            dests.append((self.x[j], self.out[j], w_self, pays))
        return dests

    def fold(self):
        """Every owned node's Metro-Hastings fold into ``out``, behind the status words.  Returns
        the status words as the host sees them (one read, after the folds are enqueued)."""
        self._guard_to_host()
        ev = None
        if self.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
        if not self._hip:
            if not bool(self._guard_host.any()):
                for j, (nbrs, w, w_self) in enumerate(self.weights):
                    rows = [(q, self._row(q)) for q in nbrs]
                    pays = [(self.seeds[q] + self.round, self.alpha,
                             self._vals(row)[:self._count_of(row)]) for q, row in rows]
                    self._fold(self.x[j], pays, w, w_self, self.out[j])
            return self._guard_host
        from . import codec
        key = ("fold", self.x.data_ptr(), self.out.data_ptr())
        if key not in self._tabs:
            dests = self._dests()
            near = [d for d in dests if len(d[3]) <= codec.MASK_FOLD_MAX]
            far = [j for j, d in enumerate(dests) if len(d[3]) > codec.MASK_FOLD_MAX]
            tab = codec.fold_node_table(near, self.device) if near else None
            self._tabs[key] = (tab, far, dests)
        tab, far, dests = self._tabs[key]
        if tab is not None:
            codec.mask_decode_average_nodes(tab[0], tab[1], self.N, guard=self.guard)
        if ev is not None:
            ev.synchronize()  # the gathers and the exchange only: the folds keep running
        if far and not bool(self._guard_host.any()):
            # more than 16 payloads: the chained fold (DPZ_FOLD_ACCUMULATE), which takes no guard
            # and so follows the host's look at the status words
            for j in far:
                local, out, w_self, pays = dests[j]
                codec.mask_decode_average(local, [p[:3] for p in pays], [p[3] for p in pays],
                                          w_self, out=out)
        return self._guard_host

    def step(self, mark=None):
        """One round.  No host synchronisation between the launches; the status words are read
        once.  A slot that was too small for its mask raises RuntimeError: the folds wrote
        nothing and the models are those of before the round (the round's counter updates and
        payloads stand: construct the engine with a larger ``slot_cap``).  ``mark(leg)`` is
        called after each leg is enqueued (tools/bench_subsampling_round.py records an event)."""
        mark = mark or (lambda leg: None)
        self.masks()
        mark("mask")
        self.gather()
        mark("gather")
        self.exchange()
        mark("exchange")
        self.fold()
        mark("fold")
        bad = self._bad_nodes()
        if bad:
            raise RuntimeError(
                f"SubSampling round {self.round}: the masks of nodes {bad} select more "
                f"than the slot's {self.cap} values; nothing was folded")
        self.x, self.out = self.out, self.x
        self.round += 1
