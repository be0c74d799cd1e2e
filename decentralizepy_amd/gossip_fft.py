"""One synchronous FFT-sharing gossip round of a whole topology with ONE launch set per leg for all
of a rank's nodes.

Semantics: the reference ``sharing/JWINS/FFT.py`` class with ``change_based_selection = True``,
one object per node, driven as ``node/DPSGDNode.py:90-115`` drives a node.  With ``M = N / 2 + 1``
and ``k = round(alpha M)``, every node shares the k coefficients of ``F(x)`` at the k largest
``|change|`` (indices ascending, ``shared_parameters_counter += 1`` there), where ``change`` is

* ``F(x - x0)`` without accumulation;
* ``acc`` after ``acc += F(x - x0)`` with ``accumulation`` (PartialModel.py:321-325);
* ``F(x - x0) + acc`` with ``accumulate_averaging_changes`` too (PartialModel.py:326-329);

the accumulator is zeroed at the shared indices (Model.py:53-64).  The neighbours' payloads fold
over the local ``F(x)`` with Metro-Hastings weights in neighbour-set order (FFT.py:252-299), the
inverse transform gives the new model (FFT.py:301), ``acc += F(x_new - x0)`` with
``accumulate_averaging_changes`` (PartialModel.py:346-349) and ``x0 = x_new``.

A ``step()`` is, whatever the node count and with no host synchronisation:

1. ONE ``dpz_rfft_nodes`` launch set of 2 m jobs: ``F(x)`` and ``F(x - x0)`` of every node;
2. ONE ``dpz_cplx_encode_nodes`` launch set (one memset, nine launches) into this rank's
   ``[pair block | val block]``;
3. ONE all-gather of that int32 buffer.  It carries 4 k words per node: the indices travel in
   the float-pair form ``(2 i, 2 i + 1)`` the fold reads (2 k words) beside the k complex values
   (2 k words), so no rank converts indices after the exchange;
4. the batched fold over the float view of ``fx`` into ``ch`` (n = 2 M):
   ``dpz_decode_average_batch_guarded`` with a zero guard word (any number of neighbours: one
   launch per table of nodes), else (2 M < 1024, a node without neighbours)
   ``dpz_decode_average_batch`` on the same stream;
5. ONE ``dpz_irfft_nodes`` launch set into ``x``;
6. with ``accumulate_averaging_changes``: ONE accumulating ``dpz_rfft_nodes`` launch set of m
   jobs (``x``, ``x0`` -> ``acc``);
7. ONE copy of all rows of ``x`` into ``x0``.

Sizes without a native plan (``codec.fft_native(N)`` false: a prime factor of N / 2 above 4096,
e.g. LeNet's 89,834 = 2 * 44,917) run the transforms of steps 1, 5 and 6 node after node through
``codec.rfft`` / ``codec.irfft`` (hipFFT) and the elementwise calls, as the per-node plugin does;
the batched selection and fold still apply.  A batched hipFFT plan is not offered.  With
``chirp=True`` such a size runs the three transform legs through ``dpz_rfft_chirp_nodes`` /
``dpz_irfft_chirp_nodes`` on the same tables instead (the chirp-z algorithm: one launch set per
leg again); ``batched`` says whether the transforms run as launch sets, ``native`` stays
``codec.fft_native(N)``.  At a size with a native plan ``chirp`` changes nothing.

Ties at the k-th key go to the lowest indices; finite models only.  The device FFT rounds
differently from the reference's pocketfft, so parity with the reference is a tolerance parity
(DESIGN.md 6); against the per-node plugin of this package the round is bit for bit.

``ops`` (an object with ``tests/fft_round_ops.OracleFftOps``'s methods) replaces the HIP codec node
by node on CPU tensors, so the round logic is tested with the gloo backend; the default is the HIP
codec (no CPU fallback).
"""
import ctypes

import torch

from .gossip import mh_weights
from .gossip_jwins import ALIGN, _al
from .gossip_round import ShardedRound

LEGS = ("encode", "exchange", "fold", "post")
ACC_NONE, ACC_ACCUMULATE, ACC_ADD = 0, 1, 2  # DPZ_ACC_*


class FftRound(ShardedRound):
    """Nodes [lo, hi) of a topology on this rank; ``step()`` runs one FFT round of every node.

    Per-node state, rows of (hi - lo, ·) tensors whose rows start on 256-byte boundaries: ``x``
    (the model; the caller trains it in place between rounds), ``x0`` (init_model == prev), ``fx``
    (F(x) of the round, M complex), ``ch`` (F(x - x0), then the fold's total), ``key`` (M fp32),
    ``acc`` (accumulated_changes, M complex; None without accumulation) and ``counter``
    (shared_parameters_counter, M int32)."""

    def __init__(self, adj, x_init, alpha, rank=0, world=1, group=None, metadata_cap=1.0,
                 accumulation=False, accumulate_averaging_changes=False,
                 change_based_selection=True, device=None, ops=None, chirp=False, **unknown):
        if unknown:
            raise ValueError(
                f"unknown arguments {sorted(unknown)}: FftRound offers neither compressed "
                "payloads nor another exchange than the all-gather")
        if not isinstance(chirp, bool):
            raise ValueError(f"chirp={chirp!r}: True or False")
        if not change_based_selection:
            raise ValueError("change_based_selection=False (selection by |F(x)|) is not "
                             "offered: use the per-node plugin sharing.JWINS.FFT")
        super().__init__(adj, x_init, rank, world, group, device)
        N = self.N
        if N < 4 or N % 2:
            raise ValueError(
                f"a model of {N} parameters: the reference's irfft returns 2 (M - 1) values, so "
                "an odd size fails in its reshape; the batched round takes even N >= 4")
        self.M = M = N // 2 + 1
        if alpha >= metadata_cap:
            raise ValueError(
                f"alpha {alpha} >= metadata_cap {metadata_cap}: a full FFT payload makes the "
                "reference's receiver raise KeyError (FFT.py:225-234), so no topology runs it")
        self.k = k = round(alpha * M)
        if k < 1:
            raise ValueError(f"alpha {alpha}: k = round(alpha M) = {k} of M = {M} coefficients: "
                             "an empty payload is not a share")
        self.alpha, self.metadata_cap = alpha, metadata_cap
        self.accumulation = bool(accumulation)
        self.aac = self.accumulation and bool(accumulate_averaging_changes)
        self.acc_mode = ACC_ADD if self.aac else (ACC_ACCUMULATE if self.accumulation
                                                  else ACC_NONE)
        self._hip = ops is None
        self.ops = ops
        m = self.m

        def rows(length, dtype=torch.float32):
            per256 = 256 // torch.empty(0, dtype=dtype).element_size()
            buf = torch.zeros(max(1, m), -(-length // per256) * per256, dtype=dtype,
                              device=self.device)
            return buf, buf[:m, :length]

        self._xbuf, self.x = rows(N)
        self._x0buf, self.x0 = rows(N)
        self.x.copy_(x_init)
        self.x0.copy_(x_init)
        _, self.fx = rows(M, torch.complex64)
        _, self.ch = rows(M, torch.complex64)
        _, self.key = rows(M)
        self.acc = rows(M, torch.complex64)[1] if self.accumulation else None
        _, self.counter = rows(M, torch.int32)
        # one buffer per rank: [pair block | val block], a slot of 2 k words per node in each
        self._slot = _al(2 * k)
        self._half = max(self.per * self._slot, ALIGN)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.send = torch.zeros(2 * self._half, **i32)
        self.recv = torch.zeros(world * 2 * self._half, **i32) if self.coll else None
        self.weights = [mh_weights(adj, i) for i in range(self.lo, self.hi)]
        self.chirp = chirp
        self.native = self.batched = True
        if self._hip and m:
            self._init_hip()

    def _init_hip(self):
        from . import codec
        dev, m, M, N, k = self.device, self.m, self.M, self.N, self.k
        self.native = codec.fft_native(N)
        self.batched = self.native or self.chirp
        xs, x0s = list(self.x), list(self.x0)
        if self.batched:
            self._pre = codec.FftNodesTable(xs + xs, [None] * m + x0s,
                                            list(self.fx) + list(self.ch), False, dev)
            self._inv = codec.IfftNodesTable(self.ch, self.x, dev)
            self._post = codec.FftNodesTable(self.x, self.x0, self.acc, True, dev) \
                if self.aac else None
            if self.native:
                self._fws = codec.fft_nodes_workspace(2 * m, N, dev)
            else:  # the same tables through the chirp-z entry points
                self._fws = codec.fft_chirp_nodes_workspace(2 * m, N, dev)
        else:
            self._fft_ws = codec.Workspace(dev)
            self._diff = torch.empty(N, dtype=torch.float32, device=dev)
            self._d = torch.empty(M, dtype=torch.complex64, device=dev)
        pair = [self.send[j * self._slot:j * self._slot + 2 * k] for j in range(m)]
        val = [self.send[self._half + j * self._slot:self._half + j * self._slot + 2 * k]
               for j in range(m)]
        self._enc = codec.CplxEncodeTable(self.ch, self.acc, self.fx, self.key, self.counter,
                                          pair, val, dev)
        self._ews = torch.empty(
            max(256, int(codec._lib.lib().dpz_cplx_encode_workspace_bytes(m, M))),
            dtype=torch.uint8, device=dev)
        self._guard = torch.zeros(1, dtype=torch.int32, device=dev)
        maxp = max((len(nb) for nb, _, _ in self.weights), default=1)
        self._dws = codec.Workspace(dev).get_decode(2 * M, max(1, maxp))
        counts, w, ws_ = [], [], []
        for nbrs, wj, w_self in self.weights:
            counts.append(len(nbrs))
            w.extend(wj)
            ws_.append(w_self)
        self._tot = tot = max(1, len(w))
        base = (self.recv if self.coll else self.send).data_ptr()
        idx, val_p = [], []
        for nbrs, _, _ in self.weights:
            for q in nbrs:
                pi, pv = self._place(q)
                idx.append(base + 4 * pi)
                val_p.append(base + 4 * pv)
        self._fold_tab = dict(
            np=(ctypes.c_int * m)(*counts), w=(ctypes.c_float * tot)(*w),
            w_self=(ctypes.c_float * m)(*ws_),
            local=(ctypes.c_void_p * m)(*codec._row_ptrs(self.fx, m)),
            out=(ctypes.c_void_p * m)(*codec._row_ptrs(self.ch, m)),
            idx=(ctypes.c_void_p * tot)(*idx), val=(ctypes.c_void_p * tot)(*val_p),
            k=(ctypes.c_int64 * tot)(*([2 * k] * len(idx))))

    # ---- layout of the payloads --------------------------------------------------------------
    def _place(self, q):
        """Word offsets of node q's pair slot and val slot in the buffer the folds read (every
        rank's blocks after an all-gather, this rank's in place)."""
        base = (q // self.per) * 2 * self._half if self.coll else 0
        j = q % self.per if self.coll else q
        return base + j * self._slot, base + self._half + j * self._slot

    def _pairs_vals(self, q):
        pi, pv = self._place(q)
        buf = self.recv if self.coll else self.send
        return buf[pi:pi + 2 * self.k], buf[pv:pv + 2 * self.k].view(torch.float32)

    def payload(self, q):
        """``(idx int32[k], vals complex64[k])`` of node q's payload of the last round (an owned
        node; any node after an all-gather)."""
        pairs, vals = self._pairs_vals(q)
        return pairs[0::2] // 2, torch.view_as_complex(vals.view(-1, 2))

    def _rfft_nodes(self, table):
        from . import codec
        call = codec.rfft_nodes if self.native else codec.rfft_chirp_nodes
        call(table, self.N, self._fws)

    def _irfft_nodes(self, table):
        from . import codec
        call = codec.irfft_nodes if self.native else codec.irfft_chirp_nodes
        call(table, self.N, self._fws)

    # ---- the legs of a round -----------------------------------------------------------------
    def encode(self):
        """F(x), F(x - x0) and the payload of every owned node; acc and the counter updated."""
        m, k = self.m, self.k
        if not m:
            return
        if self._hip:
            from . import codec
            if self.batched:
                self._rfft_nodes(self._pre)
            else:
                for j in range(m):
                    codec.elementwise(codec.DPZ_EW_SUB, self.x[j], self.x0[j], out=self._diff)
                    codec.rfft(self.x[j], out=self.fx[j], workspace=self._fft_ws)
                    codec.rfft(self._diff, out=self.ch[j], workspace=self._fft_ws)
            codec.cplx_encode_nodes(self._enc, self.M, k, self.acc_mode, self._ews)
            return
        for j in range(m):
            self.ops.transform_pair(self.x[j], self.x0[j], self.fx[j], self.ch[j])
            pairs, vals = (self.send[j * self._slot:j * self._slot + 2 * k],
                           self.send[self._half + j * self._slot:
                                     self._half + j * self._slot + 2 * k].view(torch.float32))
            self.ops.encode(self.ch[j], None if self.acc is None else self.acc[j], self.acc_mode,
                            self.fx[j], self.key[j], self.counter[j], k, pairs, vals)

    def exchange(self):
        """ONE all-gather of this rank's ``[pair block | val block]``."""
        if self.coll:
            self.all_gather(self.recv, self.send)

    def fold(self):
        """Every owned node's Metro-Hastings fold over the float view of its F(x) into ``ch``."""
        m, M = self.m, self.M
        if not m:
            return
        if not self._hip:
            jobs = []
            for j, (nbrs, w, w_self) in enumerate(self.weights):
                jobs.append((torch.view_as_real(self.fx[j]).view(-1),
                             [self._pairs_vals(q) for q in nbrs], w, w_self,
                             torch.view_as_real(self.ch[j]).view(-1)))
            self.ops.fold_all(jobs, 2 * M)
            return
        from . import _lib
        ft, tot = self._fold_tab, self._tot
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L = _lib.lib()
        rc = L.dpz_decode_average_batch_guarded(
            m, ft["local"], ft["out"], 2 * M, ft["np"], ft["idx"], ft["val"], ft["k"], ft["w"],
            ft["w_self"], _lib.DPZ_FOLD_SELF, self._guard.data_ptr(), 1, stream)
        if rc == _lib.DPZ_ERR_UNSUPPORTED:  # 2 M < 1024 or a node without neighbours: node after node
            rc = L.dpz_decode_average_batch(
                m, ft["local"], ft["out"], 2 * M, ft["np"], ft["idx"], ft["val"], ft["k"], ft["w"],
                ft["w_self"], _lib.DPZ_FOLD_SELF, (ctypes.c_void_p * 1)(self._dws.data_ptr()),
                self._dws.numel(), 1, (ctypes.c_void_p * 1)(stream.value))
            _lib.check(rc, "dpz_decode_average_batch")
            return
        _lib.check(rc, "dpz_decode_average_batch_guarded")

    def post(self):
        """model <- irfft(total); acc += F(x_new - x0) with accumulate_averaging_changes;
        x0 <- x_new, of every owned node."""
        if not self.m:
            return
        if self._hip:
            from . import codec
            if self.batched:
                self._irfft_nodes(self._inv)
                if self.aac:
                    self._rfft_nodes(self._post)
            else:
                for j in range(self.m):
                    codec.irfft(self.ch[j], self.N, out=self.x[j], workspace=self._fft_ws)
                    if self.aac:
                        codec.elementwise(codec.DPZ_EW_SUB, self.x[j], self.x0[j], out=self._diff)
                        codec.rfft(self._diff, out=self._d, workspace=self._fft_ws)
                        a = torch.view_as_real(self.acc[j]).view(-1)
                        codec.elementwise(codec.DPZ_EW_ADD, a,
                                          torch.view_as_real(self._d).view(-1), out=a)
        else:
            for j in range(self.m):
                self.ops.inverse(self.ch[j], self.N, self.x[j])
                if self.aac:
                    self.ops.accumulate(self.acc[j], self.x[j], self.x0[j])
        self._x0buf.copy_(self._xbuf)  # every row at once, the rows' padding included

    def step(self, mark=None):
        """One round.  Nothing synchronises with the host.  ``mark(leg)`` is called after each of
        ``LEGS`` is enqueued (tools/bench_fft_round.py records an event)."""
        mark = mark or (lambda leg: None)
        self.encode()
        mark("encode")
        self.exchange()
        mark("exchange")
        self.fold()
        mark("fold")
        self.post()
        mark("post")
        self.round += 1
