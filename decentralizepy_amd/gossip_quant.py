"""One synchronous QUANTISED full-model gossip round of a whole topology on the GPU.

``sharing/Sharing.py`` / ``sharing/PlainAverageSharing.py`` with ``compress = True`` and
``compression_class = Quantization`` is the one compressed full-model configuration the reference
can express: every sender's model travels as ``compression/Quantization.py``'s stream (a w-bit
field per value and an fp32 scale), a receiver decodes each stream and folds it with its OWN fp32
model (``Sharing.py:80-91, :156-190``, ``PlainAverageSharing.py:82-114``).  The quantiser is
lossy and does not round-trip (it normalises by ``max|x| / k`` and rescales by ``mean|x| / k``),
so an uncompressed engine computes something else.

These engines keep every owned node's fp32 model resident in HBM (two buffers), shard the nodes
over the ranks like ``gossip.GossipRound`` and run a round as ``dpz_quant_encode_nodes`` (two
launches whatever the node count) into one packed row per node, ONE ``all_gather_into_tensor`` of
the packed rows (the fp32 models do not travel) and ONE ``dpz_qdense_average_nodes`` launch that
unpacks and folds into the second buffer; then the buffers swap.  Nothing synchronises with the
host inside ``step()``: the fold reads each row's width and scale from its header on the device,
and behind the rows' status words it turns into a copy, so the swap is unconditional and a round
that could not be quantised changes no model; ``check()`` reads the status words.

A node's packed row is ``[count = N (int64), status, 0 | the 8 info words of the quantiser | body
dwords]`` (``codec.quant_row_words``), padded to a multiple of 4 words.  The slot holds
``slot_bits`` bits per value; the width the quantiser finds is ``bit_length(qmax) + 1`` with
``qmax = rint(max / fl(max / k))``, which is exactly k whenever the norm is a normal number and
k <= 2^22, so the default slot is ``bit_length(k) + 1`` there and ``codec.quant_encode``'s bound
``min(32, bit_length(k) + 2)`` above.  A wider field (a subnormal norm) is reported by
``check()``, never truncated.

The encode / fold callables are injectable together so the sharding and the exchange can be
tested with the CPU gloo backend; the defaults are the HIP codec (no CPU fallback).
"""
from random import Random

import numpy as np
import torch

from .gossip import mh_weights
from .gossip_epidemic import EpidemicRound
from .gossip_round import PackedRowRound, up4

INFO = PackedRowRound.HEADER   # int32 words in front of a row's info record
BODY = INFO + 8                # ... and in front of its body
REASONS = {1: "an all-zero model", 2: "a non-finite model",
           3: "max|x| / float_precision underflows",
           4: "a field wider than the slot (a subnormal norm): raise slot_bits"}


def default_slot_bits(k):
    """Bits per value of the default slot for float_precision k."""
    k = int(k)
    return k.bit_length() + 1 if k <= 2 ** 22 else min(32, k.bit_length() + 2)


class QuantRound(PackedRowRound):
    """Nodes [lo, hi) of a topology on this rank; ``step()`` runs one round of every owned node.
    A subclass says who folds what: ``lists(t)`` returns, per owned node, ``(senders, weights,
    w_self)`` in fold order.  ``x`` is a writable view of the owned nodes' fp32 models: the caller
    applies its local training to it between rounds."""

    static = False  # the lists are the same every round: the fold tables are built once

    def __init__(self, adj, x_init, float_precision=32767, slot_bits=None, rank=0, world=1,
                 group=None, device=None, mode=0, encode=None, fold=None, **unknown):
        """adj: adjacency sets (``gossip.read_edges``); x_init: (hi - lo, N) fp32 tensor, this
        rank's nodes' flat models.  ``encode(x, k) -> (np.float32 scale, uint8 to_send)`` (one
        node: the reference's wire value before the pickle) and ``fold(local, [(scale, to_send)],
        weights, w_self, out)`` (one node) are injectable (CPU tests).  mode: the fold's kernel
        path (codec.qdense_average_nodes), 0 = auto."""
        if unknown:
            raise ValueError(f"unknown arguments {sorted(unknown)}: the peer exchange, the "
                             "over-HBM (reduce-scatter) exchange and codecs other than "
                             "Quantization are not implemented for quantised full-model rounds")
        if (encode is None) != (fold is None):
            raise ValueError("encode and fold are injected together")
        k = float_precision
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"float_precision must be an int, got {type(k).__name__}")
        if not 1 <= int(k) <= 2 ** 30:
            raise ValueError("float_precision must be in [1, 2^30]")
        super().__init__(adj, x_init, rank, world, group, device)
        m, N = self.m, self.N
        self.k = int(k)
        self.slot_bits = default_slot_bits(self.k) if slot_bits is None else int(slot_bits)
        if not 2 <= self.slot_bits <= 32:
            raise ValueError("slot_bits must lie in [2, 32]")
        self.mode = int(mode)
        self._hip = encode is None
        self._encode, self._fold = encode, fold
        self.stride = S = up4(N)  # every model row 16-byte aligned
        f32 = dict(dtype=torch.float32, device=self.device)
        self._cur, self._nxt = torch.zeros(max(1, m), S, **f32), torch.zeros(max(1, m), S, **f32)
        self._cur[:m, :N].copy_(x_init)
        self.cap = (N * self.slot_bits + 31) // 32  # body dwords of a row
        self._alloc_rows(up4(BODY + self.cap))
        self._enc_tabs, self._tabs, self._ws = {}, {}, None

    @property
    def x(self):
        """The owned nodes' models, (hi - lo, N)."""
        return self._cur[:self.m, :self.N]

    def lists(self, t):
        raise NotImplementedError

    # ---- views of the packed rows ---------------------------------------------------------------
    def payload(self, q):
        """``(np.float32 scale, uint8 to_send)`` of node q's row of the last encode (an owned
        node; any node after an all-gather), ``to_send = [padding, w, body...]``: the reference's
        unpickled wire value.  Copies the row to the host: blocks."""
        return self._pay(self._row(q).cpu().numpy())

    def _pay(self, row):
        w, pad = int(row[INFO + 1]), int(row[INFO + 2])
        scale = row[INFO + 3:INFO + 4].view(np.float32)[0]
        body = row[BODY:].view(np.uint8)[:(self.N * w + 7) // 8]
        return np.float32(scale), np.concatenate([np.array([pad, w], np.uint8), body])

    # ---- the legs of a round --------------------------------------------------------------------
    def encode(self):
        """Every owned node's quantised stream into its packed row, with the row's header."""
        m, N = self.m, self.N
        if not m:
            return
        if self._hip:
            from . import codec
            key = self._cur.data_ptr()
            if key not in self._enc_tabs:
                self._enc_tabs[key] = codec.quant_node_table(self._cur[:m], self.send[:m])
            self._ws = codec.quant_encode_nodes(self._enc_tabs[key], N, self.k, self.slot_bits,
                                                self._ws)
            return
        for j in range(m):
            scale, to_send = self._encode(self._cur[j, :N], self.k)
            to_send = np.asarray(to_send, dtype=np.uint8)
            pad, w = int(to_send[0]), int(to_send[1])
            status = 4 if (N * w + 31) // 32 > self.cap else 0
            row = np.zeros(self.row_words, dtype=np.int32)
            row[:2] = np.array([N], dtype=np.int64).view(np.int32)
            row[2] = row[INFO] = status
            row[INFO + 1], row[INFO + 2] = w, pad
            row[INFO + 3:INFO + 4] = np.array([scale], dtype=np.float32).view(np.int32)
            if not status:
                row[BODY:].view(np.uint8)[:to_send.size - 2] = to_send[2:]
            self.send[j].copy_(torch.from_numpy(row))

    def _table(self, lists):
        from . import codec
        key = (self._cur.data_ptr(), self._nxt.data_ptr())
        if self.static and key in self._tabs:
            return self._tabs[key]
        recvs = [(self._nxt[j], self._cur[j], w_self, list(zip(senders, weights)))
                 for j, (senders, weights, w_self) in enumerate(lists)]
        tab = codec.QDenseTable(self.rows, recvs, self.device)  # a node's number is its row
        if self.static:
            self._tabs[key] = tab
        return tab

    def fold(self, lists, table=None):
        """Every owned node's unpack-and-average into the second buffer, behind the status
        words: a copy of the models when any is nonzero."""
        m, N = self.m, self.N
        if not m:
            return
        if self._hip:
            from . import codec
            codec.qdense_average_nodes(table, N, self.cap, self.mode, guard=self.guard)
            return
        if bool(self.guard.any()):
            self._nxt[:m].copy_(self._cur[:m])
            return
        rows = self.rows.numpy()
        for j, (senders, weights, w_self) in enumerate(lists):
            out = self._nxt[j, :N]
            if not senders:
                out.copy_(self._cur[j, :N])
                continue
            self._fold(self._cur[j, :N], [self._pay(rows[q]) for q in senders], weights, w_self,
                       out)

    def step(self, mark=None):
        """One round: the table of this round's lists (before anything is enqueued), the encode
        launch set, one all-gather of the packed rows, one fold launch, the swap.  Nothing
        synchronises with the host; a round that could not be quantised leaves every model as it
        was and is reported by ``check()``.  ``mark(leg)`` is called after each leg is enqueued
        (tools/bench_quant_round.py records an event)."""
        mark = mark or (lambda leg: None)
        lists = self.lists(self.round)
        table = self._table(lists) if self._hip and self.m else None
        self.encode()
        mark("encode")
        self.exchange()
        mark("exchange")
        self.fold(lists, table)
        mark("fold")
        self._cur, self._nxt = self._nxt, self._cur
        self.round += 1

    def check(self):
        """Copies the last round's status words to pinned host memory (blocks) and raises
        RuntimeError naming the nodes that could not be quantised and why.  That round changed no
        model on any rank: ``x`` is what it was before it."""
        self._guard_to_host()
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        nodes = self._bad_nodes()
        if nodes:
            status = self._guard_host.numpy()
            why = "; ".join(f"node {q}: {REASONS.get(int(status[q]), f'status {int(status[q])}')}"
                            for q in nodes)
            raise RuntimeError(f"quantised round {self.round - 1}: nodes {nodes} could not be "
                               f"quantised ({why}); no model was changed")


class QuantFullShareRound(QuantRound):
    """The D-PSGD full share with Quantization: a static topology, every neighbour sends; weights
    and fold order of ``gossip.mh_weights`` (``Sharing._averaging``)."""

    static = True

    def __init__(self, adj, x_init, float_precision=32767, **kw):
        super().__init__(adj, x_init, float_precision, **kw)
        self._lists = [mh_weights(adj, i) for i in range(self.lo, self.hi)]

    def lists(self, t):
        return self._lists


class QuantEpidemicRound(QuantRound):
    """EL-Local with Quantization: the sampler, ``send_sets``, ``received_this_round`` and the
    lists of ``gossip_epidemic.EpidemicRound`` (its methods, on this engine's state)."""

    def __init__(self, adj, x_init, degree, random_seed, float_precision=32767, senders=None,
                 **kw):
        super().__init__(adj, x_init, float_precision, **kw)
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

    sample = EpidemicRound.sample
    lists = EpidemicRound.lists
