"""One synchronous JWINS gossip round of a whole topology with ONE launch set per leg for all of a
rank's nodes.

The semantics, the state and the payload layout are ``gossip_jwins.JwinsRound``'s (see there for
the reference's lines): every node draws ``alpha = random.Random(uid).choice(alpha_list)``, shares
the top ``round(alpha M)`` wavelet coefficients of ``|W(x - x0) + acc|`` with their ``W(x)`` values
(counter += 1, accumulator rewound) or, for ``alpha >= metadata_cap``, all of ``W(x)`` with the
accumulator zeroed; the neighbours' payloads fold over the local ``W(x)`` with Metro-Hastings
weights in neighbour-set order, the inverse transform gives the new model, ``acc += W(x_new -
x0)`` and ``x0 = x_new``.  This is the reference's ``accumulation = True``,
``accumulate_averaging_changes = True``, ``change_based_selection = True``: the tutorial's and
every shipped JWINS configuration.

Where ``JwinsRound`` runs each owned node's kernels as separate calls on three streams and reads
the sampled selections' status words back once per round, a round here is, whatever the node
count:

* the round's encode table (every node's k and output slots), built and handed to the copy engine
  before anything else is enqueued;
* ONE ``dpz_dwt_sym2_nodes`` launch (W(x) and W(x - x0) of every node);
* ONE ``dpz_jwins_encode_nodes`` launch set (one memset, nine launches: the exact selection with
  a k per node; a full share zeroes its accumulator and copies its W(x) in the first pass);
* ONE all-gather of one int32 buffer per rank, ``[idx block | val block]``, the block sizes being
  the round's maxima over the ranks, which every rank derives from the replayed draws;
* the fold into the ``wc`` rows: ``dpz_decode_average_batch_guarded`` with a zero guard word when
  the round qualifies (any number of neighbours, partial and full shares mixed: one launch per
  table of nodes), else ``dpz_decode_average_batch`` on the same stream (M < 1024, a node
  without neighbours);
* ONE ``dpz_idwt_sym2_nodes`` launch into ``x``, ONE accumulating ``dpz_dwt_sym2_nodes`` launch,
  ONE copy of all rows of ``x`` into ``x0``.

Nothing synchronises with the host inside ``step()``.  sym2 at levels 1-4 only; other wavelets and
deeper levels stay with ``JwinsRound``.  Ties at the k-th key go to the lowest indices; finite
models only.

``ops`` (an object with ``tests/jwins_ops.OracleJwinsOps``'s methods) replaces the HIP codec node
by node on CPU tensors, so the round logic is tested with the gloo backend; the default is the HIP
codec (no CPU fallback).
"""
import ctypes
import random

import torch

from .gossip import mh_weights
from .gossip_jwins import ALIGN, JwinsRound, _al
from .gossip_round import ShardedRound

LEGS = ("encode", "exchange", "fold", "post")


def sym2_coeff_len(n, level):
    """Length of pywt's concatenated sym2 ``wavedec`` array of n values (mode "symmetric"), or
    None where the library's kernels refuse (n, level)."""
    lens, cur = [], int(n)
    if cur < 1:
        return None
    for _ in range(level):
        if cur < 4:
            return None
        cur = (cur + 3) // 2
        lens.append(cur)
    return sum(lens) + lens[-1]


class JwinsBatchRound(ShardedRound):
    """Nodes [lo, hi) of a topology on this rank; ``step()`` runs one JWINS round of every node.

    Node i is uid i.  Per-node state, rows of (hi - lo, ·) tensors whose rows start on 256-byte
    boundaries: ``x`` (the model; the caller trains it in place between rounds), ``x0``
    (init_model == prev), ``acc`` (accumulated_changes, M), ``wx`` (W(x) of the round), ``wc``
    (W(x - x0), then the selection's key, then the fold's total) and ``counter``
    (shared_parameters_counter, M int32)."""

    def __init__(self, adj, x_init, alpha_list="[0.1, 0.2, 0.3, 0.4, 1.0]", rank=0, world=1,
                 group=None, wavelet="sym2", level=4, metadata_cap=0.5, device=None, ops=None,
                 **unknown):
        if unknown:
            raise ValueError(
                f"unknown arguments {sorted(unknown)}: JwinsBatchRound offers neither compressed "
                "payloads nor another exchange than the all-gather")
        if wavelet != "sym2" or level not in (1, 2, 3, 4):
            raise ValueError(f"wavelet {wavelet!r} at level {level}: the batched round runs sym2 "
                             "at levels 1-4; use gossip_jwins.JwinsRound for the others")
        super().__init__(adj, x_init, rank, world, group, device)
        self.alpha_list = eval(alpha_list) if isinstance(alpha_list, str) else list(alpha_list)
        self.metadata_cap, self.level, self.wavelet = metadata_cap, level, wavelet
        M = sym2_coeff_len(self.N, level)
        if M is None:
            raise ValueError(f"a model of {self.N} parameters is too short for level {level}")
        self.M = M
        partial = [a for a in self.alpha_list if a < metadata_cap]
        for a in partial:
            if round(a * M) < 1:
                raise ValueError(f"alpha {a}: k = round(alpha M) = {round(a * M)} of M = {M} "
                                 "coefficients: an empty payload is not a share")
        self._hip = ops is None
        self.ops = ops
        # JWINS.__init__: random.seed(uid) in every node process; every rank replays every node's
        # draws, so every payload's size and place are known everywhere
        self.rngs = [random.Random(uid) for uid in range(self.n_nodes)]
        m = self.m

        def rows(length, dtype=torch.float32):
            buf = torch.zeros(max(1, m), _al(length), dtype=dtype, device=self.device)
            return buf, buf[:m, :length]

        self._xbuf, self.x = rows(self.N)
        self._x0buf, self.x0 = rows(self.N)
        self.x.copy_(x_init)
        self.x0.copy_(x_init)
        _, self.acc = rows(M)
        _, self.wx = rows(M)
        _, self.wc = rows(M)
        _, self.counter = rows(M, torch.int32)
        # one buffer per rank: [idx block | val block], sized for a round's largest blocks
        kmax = max([round(a * M) for a in partial], default=0)
        full = any(a >= metadata_cap for a in self.alpha_list)
        self._cap = self.per * (_al(kmax) + _al(max(kmax, M if full else 0)))
        self._cap = max(self._cap, 2 * ALIGN)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.send = torch.zeros(self._cap, **i32)
        self.recv = torch.zeros(world * self._cap, **i32) if self.coll else None
        self.weights = [mh_weights(adj, i) for i in range(self.lo, self.hi)]
        self.alphas = None
        self._lay = self._s_idx = self._s_val = None
        if self._hip and m:
            from . import codec
            dev = self.device
            self._pair = codec.DwtNodesTable(self.x, self.x0, self.wx, self.wc, dev)
            self._enc = codec.JwinsEncodeTable(self.wc, self.acc, self.wx, self.counter, dev)
            self._inv = codec.IdwtNodesTable(self.wc, self.x, dev)
            self._post = codec.DwtNodesTable(self.x, self.x0, None, self.acc, dev)
            self._ws = torch.empty(
                max(256, int(codec._lib.lib().dpz_jwins_encode_workspace_bytes(m, M))),
                dtype=torch.uint8, device=dev)
            self._guard = torch.zeros(1, **i32)
            maxp = max((len(nb) for nb, _, _ in self.weights), default=1)
            self._dws = codec.Workspace(dev).get_decode(M, max(1, maxp))
            counts, w, ws_ = [], [], []
            for nbrs, wj, w_self in self.weights:
                counts.append(len(nbrs))
                w.extend(wj)
                ws_.append(w_self)
            tot = max(1, len(w))
            self._tot = tot
            self._fold_tab = dict(
                np=(ctypes.c_int * m)(*counts), w=(ctypes.c_float * tot)(*w),
                w_self=(ctypes.c_float * m)(*ws_),
                local=(ctypes.c_void_p * m)(*self._ptrs(self.wx)),
                out=(ctypes.c_void_p * m)(*self._ptrs(self.wc)))

    @staticmethod
    def _ptrs(rows):
        base, step = rows.data_ptr(), rows.stride(0) * rows.element_size()
        return [base + j * step for j in range(rows.shape[0])]

    # ---- layout of one round's payloads ------------------------------------------------------
    def _place(self, q):
        """Node q's (partial, k, word offset of its idx slot, of its val slot) in the buffer the
        folds read (every rank's blocks after an all-gather, this rank's in place)."""
        partial, k, oi, ov = self._lay[q]
        base = (q // self.per) * (self._s_idx + self._s_val) if self.coll else 0
        return partial, k, base + oi, base + self._s_idx + ov

    def payload(self, q):
        """``(idx or None, vals)`` of node q's payload of the last round (an owned node; any
        node after an all-gather).  A full share has no indices."""
        partial, k, pi, pv = self._place(q)
        buf = self.recv if self.coll else self.send
        if partial:
            return buf[pi:pi + k], buf[pv:pv + k].view(torch.float32)
        if not self.coll:
            return None, self.wx[q - self.lo]  # the full W(x), no copy on one rank
        return None, buf[pv:pv + self.M].view(torch.float32)

    # ---- the legs of a round -----------------------------------------------------------------
    def encode(self):
        """W(x), W(x - x0) and the payload of every owned node; acc and the counter updated."""
        m, M = self.m, self.M
        if not m:
            return
        if self._hip:
            from . import codec
            base = self.send.data_ptr()
            for j in range(m):
                partial, k, oi, ov = self._lay[self.lo + j]
                pv = base + 4 * (self._s_idx + ov)
                if partial:
                    self._enc.set(j, k, base + 4 * oi, pv)
                else:  # Wavelet.py:185-192: all of W(x); copied only where it is gathered
                    self._enc.set(j, 0, 0, pv if self.coll else 0)
            self._enc.upload()
            codec.dwt_sym2_nodes(self._pair, self.N, self.level)
            codec.jwins_encode_nodes(self._enc, M, self._ws)
            return
        vals = self.send[self._s_idx:self._s_idx + self._s_val].view(torch.float32)
        for j in range(m):
            partial, k, oi, ov = self._lay[self.lo + j]
            self.ops.transform_pair(self.x[j], self.x0[j], self.wx[j], self.wc[j])
            if partial:
                self.ops.encode(self.wc[j], k, self.acc[j], self.wx[j], self.counter[j],
                                self.send[oi:oi + k], vals[ov:ov + k])
            else:
                self.acc[j].zero_()
                if self.coll:
                    vals[ov:ov + M].copy_(self.wx[j])

    def exchange(self):
        """ONE all-gather of this rank's ``[idx block | val block]``."""
        if self.coll:
            W = self._s_idx + self._s_val
            self.all_gather(self.recv[:self.world * W], self.send[:W])

    def fold(self):
        """Every owned node's Metro-Hastings fold over its W(x) into its ``wc`` row."""
        m, M = self.m, self.M
        if not m:
            return
        if not self._hip:
            jobs = []
            for j, (nbrs, w, w_self) in enumerate(self.weights):
                jobs.append((self.wx[j], [self.payload(q) for q in nbrs], w, w_self, self.wc[j]))
            self.ops.fold_all(jobs, M)
            return
        from . import _lib
        base = (self.recv if self.coll else self.send).data_ptr()
        wx0, wstep = self.wx.data_ptr(), self.wx.stride(0) * 4
        idx, val, kk = [], [], []
        for nbrs, _, _ in self.weights:
            for q in nbrs:
                partial, k, pi, pv = self._place(q)
                if partial:
                    idx.append(base + 4 * pi)
                    val.append(base + 4 * pv)
                    kk.append(k)
                else:
                    idx.append(None)
                    val.append(base + 4 * pv if self.coll else wx0 + (q - self.lo) * wstep)
                    kk.append(M)
        ft, tot = self._fold_tab, self._tot
        idx_a, val_a = (ctypes.c_void_p * tot)(*idx), (ctypes.c_void_p * tot)(*val)
        k_a = (ctypes.c_int64 * tot)(*kk)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L = _lib.lib()
        rc = L.dpz_decode_average_batch_guarded(
            m, ft["local"], ft["out"], M, ft["np"], idx_a, val_a, k_a, ft["w"], ft["w_self"],
            _lib.DPZ_FOLD_SELF, self._guard.data_ptr(), 1, stream)
        if rc == _lib.DPZ_ERR_UNSUPPORTED:  # M < 1024 or a node without neighbours: node after node
            rc = L.dpz_decode_average_batch(
                m, ft["local"], ft["out"], M, ft["np"], idx_a, val_a, k_a, ft["w"], ft["w_self"],
                _lib.DPZ_FOLD_SELF, (ctypes.c_void_p * 1)(self._dws.data_ptr()),
                self._dws.numel(), 1, (ctypes.c_void_p * 1)(stream.value))
            _lib.check(rc, "dpz_decode_average_batch")
            return
        _lib.check(rc, "dpz_decode_average_batch_guarded")

    def post(self):
        """model <- waverec(total); acc += W(x_new - x0); x0 <- x_new, of every owned node."""
        if not self.m:
            return
        if self._hip:
            from . import codec
            codec.idwt_sym2_nodes(self._inv, self.N, self.level)
            codec.dwt_sym2_nodes(self._post, self.N, self.level, accumulate=True)
        else:
            for j in range(self.m):
                self.ops.inverse(self.wc[j], self.N, self.x[j])
                self.ops.accumulate(self.acc[j], self.x[j], self.x0[j])
        self._x0buf.copy_(self._xbuf)  # every row at once, the rows' padding included

    def step(self, mark=None):
        """One round.  Nothing synchronises with the host.  ``mark(leg)`` is called after each of
        ``LEGS`` is enqueued (tools/bench_jwins_round.py records an event)."""
        mark = mark or (lambda leg: None)
        self.alphas = [rng.choice(self.alpha_list) for rng in self.rngs]
        self._lay, self._s_idx, self._s_val = JwinsRound._layout(self, self.alphas)
        self.encode()
        mark("encode")
        self.exchange()
        mark("exchange")
        self.fold()
        mark("fold")
        self.post()
        mark("post")
        self.round += 1
