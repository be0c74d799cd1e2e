"""One synchronous round of a whole topology of top-k sharing with accumulated changes on the GPU.

The reference's ``sharing/PartialModel.py`` with ``accumulation = True`` ("TopK with
accumulation", the baseline of the JWINS experiments) keeps per node a vector
``accumulated_changes`` and a counter ``shared_parameters_counter`` across rounds.  A round of a
node, ``init`` the model its last round ended with:

* ``accumulate_averaging_changes = False`` (mode "acc"): ``acc += x - init`` everywhere, the k =
  round(alpha N) largest ``|acc|`` are selected (:320-325);
* ``accumulate_averaging_changes = True`` (mode "avg"): the k largest ``|(x - init) + acc|`` are
  selected, ``acc`` is not written (:326-329);
* both: the payload is the selection's indices ascending with ``x[idx]``, ``counter[idx] += 1``,
  ``acc[idx] = 0`` (:188-255); the neighbours' payloads replace over the node's own model and fold
  with Metro-Hastings weights in ``list(adj[i])`` order (``Sharing._averaging``), exactly
  ``gossip.GossipRound``'s fold;
* mode "avg": ``acc += x_new - init`` (:345-349); both: ``init = x_new``.

This engine keeps x, init (``x0``), acc, the counter and the fold's output of every owned node
resident in HBM and shards the nodes over the ranks like the other engines.  A round is ONE
``dpz_topkacc_encode_nodes`` launch set over the owned nodes, ONE ``all_gather_into_tensor`` of a
packed row per node, the batched one-launch fold with the payload pointers pointing into the
packed rows, in mode "avg" ONE ``dpz_topkacc_post_nodes`` launch, and the swap of ``x0`` with the
fold's output.  In mode "avg" the encode's key vector goes into the fold's output row, which is
free until the fold: no extra allocation.  Nothing synchronises with the host inside ``step()``.

Ties at the k-th key go to the lowest indices (``torch.topk``'s order is implementation-defined).
Finite models only.

The encode / fold / post callables are injectable together so the sharding and exchange logic can
be tested with the CPU gloo backend; the defaults are the HIP codec (no CPU fallback).
"""
import ctypes

import torch

from .gossip import mh_weights
from .gossip_round import PackedRowRound, up4

HEADER = PackedRowRound.HEADER


class TopKAccRound(PackedRowRound):
    """Nodes [lo, hi) of a topology on this rank; ``step()`` runs one round.  ``x`` is a stable
    tensor of the owned nodes' models: the caller applies its local training to it in place
    between rounds."""

    def __init__(self, adj, x_init, alpha, accumulate_averaging_changes=False, metadata_cap=1.0,
                 rank=0, world=1, group=None, device=None, encode=None, fold=None, post=None,
                 **unknown):
        """adj: adjacency sets of all nodes; x_init: (hi - lo, N) fp32, this rank's nodes' models.
        ``encode(x, x0, acc, counter, k, avg) -> (idx, vals)`` (one node, in place on acc and
        counter), ``fold(local, payloads, weights, w_self, out)`` (``GossipRound``'s) and
        ``post(acc, x_new, x_old)`` (in place on acc) are injectable (CPU tests)."""
        if unknown:
            raise ValueError(
                f"unknown arguments {sorted(unknown)}: TopKAccRound offers neither the peer nor the "
                "reduce-scatter exchange nor compressed payloads; use gossip.GossipRound for plain "
                "top-k with those exchanges")
        injected = [f is not None for f in (encode, fold, post)]
        if any(injected) != all(injected):
            raise ValueError("encode, fold and post are injected together")
        super().__init__(adj, x_init, rank, world, group, device)
        m, N = self.m, self.N
        self.alpha, self.avg = float(alpha), bool(accumulate_averaging_changes)
        if self.alpha >= float(metadata_cap):
            raise ValueError(f"alpha {self.alpha} >= metadata_cap {metadata_cap}: the reference "
                             "shares the full model; use gossip_epidemic.FullShareRound")
        self.k = round(self.alpha * N)
        if self.k < 1:
            raise ValueError(f"k = round(alpha N) = {self.k}: an empty payload is not a round; "
                             "use gossip_subsampling.SubSamplingRound for tiny random shares")
        self._hip = not any(injected)
        self._encode, self._fold, self._post = encode, fold, post
        self.cap = up4(self.k)
        stride = up4(N)  # every row 16-byte aligned
        self._state = torch.zeros(4, max(1, m), stride, dtype=torch.float32, device=self.device)
        self.x = self._state[0, :m, :N]
        self.x0 = self._state[1, :m, :N]
        self.acc = self._state[2, :m, :N]
        self.out = self._state[3, :m, :N]
        self.x.copy_(x_init)
        self.x0.copy_(x_init)
        self.counter = torch.zeros(max(1, m), stride, dtype=torch.int32,
                                   device=self.device)[:m, :N]
        # a packed row: [count = k (int64), status = 0, 0 | cap idx | cap vals]
        self._alloc_rows(HEADER + 2 * self.cap)
        self.weights = [mh_weights(adj, i) for i in range(self.lo, self.hi)]
        self._tabs = {}
        self._fold_tab = self._ws = self._dws = None

    # ---- views of the packed rows ---------------------------------------------------------------
    def _pay(self, row):
        return (row[HEADER:HEADER + self.k],
                row[HEADER + self.cap:HEADER + self.cap + self.k].view(torch.float32))

    def payload(self, q):
        """``(idx, vals)`` of node q's payload of its last encode (an owned node; any node after
        an all-gather)."""
        return self._pay(self._row(q))

    def _write_row(self, row, idx, vals):
        idx = torch.as_tensor(idx, dtype=torch.int32)
        vals = torch.as_tensor(vals, dtype=torch.float32)
        if idx.numel() != self.k:
            raise ValueError(f"a payload of {idx.numel()} entries, k = {self.k}")
        si, sv = self._pay(row)
        si.copy_(idx)
        sv.copy_(vals)
        row[:2] = torch.tensor([self.k], dtype=torch.int64).view(torch.int32)
        row[2:HEADER] = 0

    # ---- tables, built once ---------------------------------------------------------------------
    @staticmethod
    def _ptrs(rows):
        base, step = rows.data_ptr(), rows.stride(0) * rows.element_size()
        return (ctypes.c_void_p * max(1, rows.shape[0]))(
            *[base + j * step for j in range(rows.shape[0])])

    def _tables(self):
        """The node table and the fold's row pointers for the current (x0, out) pair: the two
        buffers swap every round, so there are two sets, each built once."""
        tab = self._tabs.get(self.x0.data_ptr())
        if tab is None:
            from . import codec
            m = self.m
            tab = self._tabs[self.x0.data_ptr()] = dict(
                node=codec.topkacc_node_table(self.x, self.x0, self.acc, self.send[:m],
                                              key=self.out, counter=self.counter),
                local=self._ptrs(self.x), out=self._ptrs(self.out))
        return tab

    def _fold_tables(self):
        """Host tables of the batched fold, built once: the payload pointers point into the packed
        rows, which do not move between rounds."""
        if self._fold_tab is None:
            counts, idx, val, w, ws_ = [], [], [], [], []
            step = self.rows.stride(0) * 4
            for nbrs, wj, w_self in self.weights:
                counts.append(len(nbrs))
                for q in nbrs:
                    row = self.rows.data_ptr() + q * step
                    idx.append(row + 4 * HEADER)
                    val.append(row + 4 * (HEADER + self.cap))
                w.extend(wj)
                ws_.append(w_self)
            m, tot = max(1, self.m), max(1, len(idx))
            self._fold_tab = dict(
                np=(ctypes.c_int * m)(*counts), idx=(ctypes.c_void_p * tot)(*idx),
                val=(ctypes.c_void_p * tot)(*val), k=(ctypes.c_int64 * tot)(*[self.k] * len(idx)),
                w=(ctypes.c_float * tot)(*w), w_self=(ctypes.c_float * m)(*ws_),
                maxp=max(counts, default=1))
        return self._fold_tab

    # ---- the legs of a round --------------------------------------------------------------------
    def encode(self):
        """Every owned node's selection into its row; acc and the counter updated."""
        if self._hip:
            from . import codec
            if self.m:
                mode = codec.DPZ_ACC_ADD if self.avg else codec.DPZ_ACC_ACCUMULATE
                self._ws = codec.topkacc_encode_nodes(self._tables()["node"], self.N, self.k,
                                                      mode, self._ws)
            return
        for j in range(self.m):
            self._write_row(self.send[j], *self._encode(self.x[j], self.x0[j], self.acc[j],
                                                        self.counter[j], self.k, self.avg))

    def fold(self):
        """Every owned node's Metro-Hastings fold into ``out`` (and, on the device, over ``x``)."""
        if not self._hip:
            for j, (nbrs, w, w_self) in enumerate(self.weights):
                self._fold(self.x[j], [self.payload(q) for q in nbrs], w, w_self, self.out[j])
            return
        if not self.m:
            return
        from . import _lib, codec
        from ._lib import DPZ_FOLD_ALSO_LOCAL, DPZ_FOLD_SELF
        tab, ft = self._tables(), self._fold_tables()
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        flags = DPZ_FOLD_SELF | DPZ_FOLD_ALSO_LOCAL
        rc = _lib.lib().dpz_decode_average_batch_guarded(
            self.m, tab["local"], tab["out"], self.N, ft["np"], ft["idx"], ft["val"], ft["k"],
            ft["w"], ft["w_self"], flags, self.guard.data_ptr(), self.guard.numel(), stream)
        if rc == _lib.DPZ_ERR_UNSUPPORTED:  # N < 1024 or a node without neighbours: node after node
            if self._dws is None:
                self._dws = codec.Workspace(self.device)
            dws = self._dws.get_decode(self.N, ft["maxp"])
            rc = _lib.lib().dpz_decode_average_batch(
                self.m, tab["local"], tab["out"], self.N, ft["np"], ft["idx"], ft["val"], ft["k"],
                ft["w"], ft["w_self"], flags, (ctypes.c_void_p * 1)(dws.data_ptr()), dws.numel(),
                1, (ctypes.c_void_p * 1)(stream.value))
            _lib.check(rc, "dpz_decode_average_batch")
            return
        _lib.check(rc, "dpz_decode_average_batch_guarded")

    def post(self):
        """Mode "avg": ``acc += x_new - x0`` of every owned node."""
        if self._hip:
            from . import codec
            if self.m:
                codec.topkacc_post_nodes(self._tables()["node"], self.N)
            return
        for j in range(self.m):
            self._post(self.acc[j], self.out[j], self.x0[j])

    def step(self, mark=None):
        """One round: the encode launch set, one all-gather (with a process group), the batched
        fold, in mode "avg" one post-step launch, and the swap that makes the averaged model the
        next round's ``x0``.  Nothing synchronises with the host.  ``mark(leg)`` is called after
        each leg is enqueued (tools/bench_topkacc_round.py records an event)."""
        mark = mark or (lambda leg: None)
        self.encode()
        mark("encode")
        self.exchange()
        mark("exchange")
        self.fold()
        mark("fold")
        if self.avg:
            self.post()
            mark("post")
        self.x0, self.out = self.out, self.x0
        if not self._hip:
            self.x.copy_(self.x0)  # the device fold wrote the result over the model itself
        self.round += 1
