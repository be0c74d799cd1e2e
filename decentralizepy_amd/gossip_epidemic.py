"""One synchronous full-model gossip round of a whole topology on the GPU.

Two families of the reference's configurations send whole models:

* Epidemic Learning (``node/EpidemicLearning/EL_Local.py`` with ``sharing/PlainAverageSharing.py``,
  ``tutorial/EpidemicLearning/config_EL.ini``): every round node u sends its model to ``degree``
  neighbours drawn from its own ``Random`` (:50-51, :85-86), and a node averages what arrived
  with its own model, every term weighted ``1 / (received + 1)`` (PlainAverageSharing.py:82-114);
  a node that received nothing keeps its model (EL_Local.py:162-165).
* the D-PSGD full share (``sharing/Sharing.py:156-190``, the ``config_*_sharing.ini`` files): every
  neighbour sends, Metro-Hastings weights.

Both are the same device work: each receiver folds whole rows.  ``DenseRound`` keeps every owned
node's flat model resident in HBM (rows a multiple of 4 floats apart, so they stay 16-byte
aligned), shards the nodes over the ranks like ``gossip.GossipRound``, and runs a round as ONE
``all_gather_into_tensor`` of the rank's rows (with a process group) and ONE
``dpz_dense_average_nodes`` launch for all of the rank's nodes into a second buffer; then the
buffers swap.  Nothing synchronises with the host in between.

The fold callable is injectable so that sampling, sharding and exchange can be tested with the
CPU gloo backend; the default is the HIP codec (no CPU fallback).
"""
from random import Random

import torch

from .gossip import mh_weights
from .gossip_round import ShardedRound, up4


class DenseRound(ShardedRound):
    """Nodes [lo, hi) of a topology on this rank; ``step()`` runs one round of every owned node.
    A subclass says who folds what: ``lists(t)`` returns, per owned node, ``(senders, weights,
    w_self)`` in fold order."""

    static = False  # the lists are the same every round: the fold tables are built once

    def __init__(self, adj, x_init, rank=0, world=1, group=None, device=None, fold=None,
                 mode=0, **unknown):
        """adj: adjacency sets (``gossip.read_edges``); x_init: (hi - lo, N) fp32 tensor, this
        rank's nodes' flat models.  ``fold(local, rows, weights, w_self, out)`` is injectable (CPU
        tests).  mode: the kernel path (codec.dense_average_nodes), 0 = auto."""
        if unknown:
            raise ValueError(f"unknown arguments {sorted(unknown)}: the peer exchange, the "
                             "over-HBM (reduce-scatter) exchange and compressed wire payloads "
                             "are not implemented for full-model rounds")
        super().__init__(adj, x_init, rank, world, group, device)
        m, N = self.m, self.N
        self.stride = S = up4(N)
        self.mode = int(mode)
        self._fold = fold
        f32 = dict(dtype=torch.float32, device=self.device)
        # two buffers of `per` rows (the all-gather's block), the models and the fold's output
        self._cur, self._nxt = torch.zeros(self.per, S, **f32), torch.zeros(self.per, S, **f32)
        self._cur[:m, :N].copy_(x_init)
        self.recv = torch.zeros(self.per * world, S, **f32) if self.coll else None
        self._tabs = {}

    @property
    def x(self):
        """The owned nodes' models, (hi - lo, N)."""
        return self._cur[:self.m, :self.N]

    def lists(self, t):
        raise NotImplementedError

    # ---- the legs of a round --------------------------------------------------------------------
    def _table(self, lists):
        from . import codec
        key = (self._cur.data_ptr(), self._nxt.data_ptr())
        if self.static and key in self._tabs:
            return self._tabs[key]
        srcs = self.recv if self.coll else self._cur  # a node's number is its row in either
        recvs = [(self._nxt[j], self.lo + j, w_self, list(zip(senders, weights)))
                 for j, (senders, weights, w_self) in enumerate(lists)]
        tab = codec.DenseTable(srcs, recvs, self.device)
        if self.static:
            self._tabs[key] = tab
        return tab

    def exchange(self):
        """ONE all-gather of the rank's rows (padded to ``per`` rows of ``stride`` floats)."""
        if self.coll:
            self.all_gather(self.recv, self._cur)

    def fold(self, lists, table=None):
        if not self.m:
            return
        if self._fold is None:
            from . import codec
            codec.dense_average_nodes(table, self.N, self.mode)
            return
        src = self.recv if self.coll else self._cur
        for j, (senders, weights, w_self) in enumerate(lists):
            out = self._nxt[j, :self.N]
            if not senders:
                out.copy_(self._cur[j, :self.N])
                continue
            self._fold(self._cur[j, :self.N], [src[q, :self.N] for q in senders],
                       weights, w_self, out)

    def step(self, mark=None):
        """One round: the table of this round's lists (before anything is enqueued), the
        all-gather, one fold launch, the swap.  ``mark(leg)`` is called after each leg is
        enqueued (tools/bench_epidemic_round.py records an event)."""
        mark = mark or (lambda leg: None)
        lists = self.lists(self.round)
        table = self._table(lists) if self._fold is None and self.m else None
        self.exchange()
        mark("exchange")
        self.fold(lists, table)
        mark("fold")
        self._cur, self._nxt = self._nxt, self._cur
        self.round += 1


class EpidemicRound(DenseRound):
    """EL-Local.  Node u owns ``Random()`` seeded ``random_seed + u`` and sends every round to
    ``set(rng.sample(tuple(adj[u]), degree))``; every rank derives every node's send set (the
    streams are a function of the seed alone).  Receiver i folds the senders j with i in send_j,
    in the iteration order of ``adj[i]``; each sender and the local term weigh
    ``1 / (received + 1)``, a Python double rounded to fp32 at the multiply.

    ``senders(t)`` (one send set per node of the topology) replaces the sampler: EL-Oracle's
    per-round regular graphs come in this way.

    ``received_this_round[i]``: what the reference's ``sharing.received_this_round`` holds after
    the round.  It is set by the averaging only, so a node that received nothing keeps the value
    of its last averaging (0 before the first), as EL_Local logs it."""

    def __init__(self, adj, x_init, degree, random_seed, senders=None, **kw):
        super().__init__(adj, x_init, **kw)
        self.degree = int(degree)
        if senders is None and not all(0 < self.degree <= len(a) for a in adj):
            raise ValueError("degree must lie in [1, the smallest neighbourhood]")
        self.random_seed = int(random_seed)
        self._senders = senders
        self._rng = []
        for u in range(self.n_nodes):
            rng = Random()
            rng.seed(self.random_seed + u)
            self._rng.append(rng)
        self.send_sets = None  # of the last round
        self.received_this_round = [0] * self.n_nodes

    def sample(self, t):
        """Every node's send set of round t.  The sampler's streams advance: once per round."""
        if self._senders is not None:
            return [set(s) for s in self._senders(t)]
        # tuple(set) keeps the set's iteration order: the stream random.sample drew from the
        # set itself before Python 3.11 stopped accepting one
        return [set(self._rng[u].sample(tuple(self.adj[u]), self.degree))
                for u in range(self.n_nodes)]

    def lists(self, t):
        self.send_sets = sets = self.sample(t)
        if len(sets) != self.n_nodes:
            raise ValueError("senders(t) must return one send set per node of the topology")
        out = []
        for i in range(self.n_nodes):
            got = [j for j in self.adj[i] if i in sets[j]]
            if got:
                self.received_this_round[i] = len(got)
            if self.lo <= i < self.hi:
                w = 1 / (len(got) + 1)
                out.append((got, [w] * len(got), w))
        return out


class FullShareRound(DenseRound):
    """The D-PSGD full share: a static topology, every neighbour sends; weights and fold order of
    ``gossip.mh_weights`` (``Sharing._averaging``)."""

    static = True

    def __init__(self, adj, x_init, **kw):
        super().__init__(adj, x_init, **kw)
        self._lists = [mh_weights(adj, i) for i in range(self.lo, self.hi)]

    def lists(self, t):
        return self._lists
