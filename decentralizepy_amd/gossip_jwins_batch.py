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

Nothing synchronises with the host inside ``step()``.  ``JwinsBatchRound`` runs sym2 at levels
1-4 on the fused kernels; ``JwinsWaveletBatchRound`` runs every other wavelet of the filter table
and sym2 at levels 5-8 with the same legs on ``dpz_dwt_generic_nodes`` /
``dpz_idwt_generic_nodes`` (``level`` launches per transform instead of one).  Ties at the k-th
key go to the lowest indices; finite models only.

With ``compression="EliasQuantization"`` (the reference's ``Wavelet`` / ``JWINS`` with
``compression_class = EliasQuantization``; ``float_precision`` is the quantiser's k) the values of
every share, the full ones included (``Wavelet.serialized_model`` -> ``compress_data``), travel
quantised: after the selection ONE ``dpz_squant_encode_nodes`` call over the owned nodes' value
lists, each with its own count (k_j, or M for a full share), the all-gather of ``[idx block |
quantised rows]``, and ONE ``dpz_squant_decode_nodes`` call of every gathered row this rank folds
into an fp32 value block, which the unchanged fold reads behind the decode's status words.  The
sender's own W(x) stays unquantised.

``wire_bytes()`` / ``wire_payload(q)`` (``gossip_round.WireCoded``) give what the round's payloads
are on the wire with ``compression_class = EliasFpzip`` at ``float_precision``; ``step()`` does not
call them.

``ops`` (an object with ``tests/jwins_ops.OracleJwinsOps``'s methods) replaces the HIP codec node
by node on CPU tensors, so the round logic is tested with the gloo backend; the default is the HIP
codec (no CPU fallback).
"""
import ctypes
import random

import torch

from .gossip import mh_weights
from .gossip_jwins import ALIGN, JwinsRound, _al
from .gossip_round import ShardedRound, WireCoded, shard, up4

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


class JwinsBatchRound(WireCoded, ShardedRound):
    """Nodes [lo, hi) of a topology on this rank; ``step()`` runs one JWINS round of every node.

    Node i is uid i.  Per-node state, rows of (hi - lo, ·) tensors whose rows start on 256-byte
    boundaries: ``x`` (the model; the caller trains it in place between rounds), ``x0``
    (init_model == prev), ``acc`` (accumulated_changes, M), ``wx`` (W(x) of the round), ``wc``
    (W(x - x0), then the selection's key, then the fold's total) and ``counter``
    (shared_parameters_counter, M int32)."""

    def __init__(self, adj, x_init, alpha_list="[0.1, 0.2, 0.3, 0.4, 1.0]", rank=0, world=1,
                 group=None, wavelet="sym2", level=4, metadata_cap=0.5, device=None, ops=None,
                 float_precision=0, selection="exact", compression=None, **unknown):
        """``compression``: None, or "EliasQuantization": every share's values are exchanged
        through the reference's quantiser with k = ``float_precision``, an int in [1, 2^30] (HIP
        only).  ``selection``: "exact", the nine-launch radix selection, or "window", the one-read
        selection around the last threshold of the node's alpha (``dpz_jwins_encode_nodes_window``,
        one prior per node and entry of ``alpha_list``): the same round bit for bit
        (``selection_status()`` tells which way a node went).  ``ops`` selects exactly either
        way."""
        if selection not in ("exact", "window"):
            raise ValueError(f"selection {selection!r}: 'exact' or 'window'")
        self.selection = selection
        if unknown:
            raise ValueError(
                f"unknown arguments {sorted(unknown)}: JwinsBatchRound offers neither compressed "
                "payloads nor another exchange than the all-gather")
        self._check_config(wavelet, level)
        super().__init__(adj, x_init, rank, world, group, device)
        self.alpha_list = eval(alpha_list) if isinstance(alpha_list, str) else list(alpha_list)
        self.metadata_cap, self.level, self.wavelet = metadata_cap, level, wavelet
        self.M = M = self._coeff_len()
        partial = [a for a in self.alpha_list if a < metadata_cap]
        for a in partial:
            if round(a * M) < 1:
                raise ValueError(f"alpha {a}: k = round(alpha M) = {round(a * M)} of M = {M} "
                                 "coefficients: an empty payload is not a share")
        self._hip = ops is None
        self.ops = ops
        self._init_wire(float_precision, [round(a * M) for a in partial], compression=compression)
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
        if self._squant:
            # on the wire [idx block | quantised rows]; the selection's values stay in ``_vraw``
            # (a node's at its idx offset), the receivers' decoded values go to ``_dvals``
            self._sq_cache = {}
            vcap = _al(max(kmax, M if full else 0))
            qcap = max(self._sq_words(kmax) if kmax else 0, self._sq_words(M) if full else 0)
            self._cap = max(ALIGN, self.per * _al(kmax)) + max(ALIGN, self.per * qcap)
            f32 = dict(dtype=torch.float32, device=self.device)
            self._vraw = torch.zeros(max(ALIGN, self.per * _al(kmax)), **f32)
            self._dvals = torch.zeros(max(ALIGN, world * self.per * vcap), **f32)
        self.send = torch.zeros(self._cap, **i32)
        self.recv = torch.zeros(world * self._cap, **i32) if self.coll else None
        self.weights = [mh_weights(adj, i) for i in range(self.lo, self.hi)]
        self.alphas = None
        self._lay = self._s_idx = self._s_val = None
        self._kmax, self._sel_ws = kmax, None
        self._exact_status = torch.zeros(m, dtype=torch.int32, device=self.device)
        if self._hip and m and selection == "window" and kmax:
            from . import codec
            if len(self.alpha_list) > codec._lib.lib().dpz_jwins_window_slots():
                raise ValueError(f"selection='window' keeps one prior per entry of alpha_list: "
                                 f"at most {codec._lib.lib().dpz_jwins_window_slots()} entries")
        if self._hip and m:
            from . import codec
            dev = self.device
            self._make_transform_tables(codec, dev)
            self._enc = codec.JwinsEncodeTable(self.wc, self.acc, self.wx, self.counter, dev)
            self._ws = torch.empty(
                max(256, int(codec._lib.lib().dpz_jwins_encode_workspace_bytes(m, M))),
                dtype=torch.uint8, device=dev)
            self._guard = torch.zeros(1, **i32)
            if self._squant:
                self._sq_enc = codec.SquantTable(m, dev)
                self._sq_nodes = sorted({q for i in range(self.lo, self.hi) for q in adj[i]})
                self._sq_dec = codec.SquantTable(len(self._sq_nodes), dev)
                # the decode's status words are the fold's guard
                self._guard = self.guard = torch.zeros(max(1, len(self._sq_nodes)), **i32)
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

    # ---- what depends on the wavelet (JwinsWaveletBatchRound overrides these) -----------------
    @staticmethod
    def _check_config(wavelet, level):
        if wavelet != "sym2" or level not in (1, 2, 3, 4):
            raise ValueError(f"wavelet {wavelet!r} at level {level}: the batched round runs sym2 "
                             "at levels 1-4; use JwinsWaveletBatchRound for the others "
                             "(gossip_jwins.JwinsRound for haar)")

    def _coeff_len(self):
        M = sym2_coeff_len(self.N, self.level)
        if M is None:
            raise ValueError(f"a model of {self.N} parameters is too short for level {self.level}")
        return M

    def _make_transform_tables(self, codec, dev):
        self._pair = codec.DwtNodesTable(self.x, self.x0, self.wx, self.wc, dev)
        self._inv = codec.IdwtNodesTable(self.wc, self.x, dev)
        self._post = codec.DwtNodesTable(self.x, self.x0, None, self.acc, dev)

    def _transform_pair(self, codec):
        codec.dwt_sym2_nodes(self._pair, self.N, self.level)

    def _transform_post(self, codec):
        codec.idwt_sym2_nodes(self._inv, self.N, self.level)
        codec.dwt_sym2_nodes(self._post, self.N, self.level, accumulate=True)

    @staticmethod
    def _ptrs(rows):
        base, step = rows.data_ptr(), rows.stride(0) * rows.element_size()
        return [base + j * step for j in range(rows.shape[0])]

    # ---- layout of one round's payloads ------------------------------------------------------
    def _place(self, q):
        """Node q's (partial, k, word offset of its idx slot, of its val slot) in the buffer the
        folds read (every rank's blocks after an all-gather, this rank's in place).  With
        ``compression`` the val offset is into ``_dvals``, the decoded values."""
        partial, k, oi, ov = self._lay[q]
        r = q // self.per if self.coll else 0
        if self._squant:
            return partial, k, r * (self._s_idx + self._s_q) + oi, r * self._s_val + ov
        base = r * (self._s_idx + self._s_val)
        return partial, k, base + oi, base + self._s_idx + ov

    # ---- the EliasQuantization exchange (gossip_round.WireCoded) ------------------------------
    def _sq_words(self, count):
        """int32 words of the quantised row of ``count`` values, rows 16-byte aligned."""
        w = self._sq_cache.get(count)
        if w is None:
            from . import codec
            w = self._sq_cache[count] = up4(codec.squant_row_words(count, self.float_precision))
        return w

    def _sq_layout(self):
        """Per node the word offset of its quantised row inside its rank's block of rows, and
        the padded block size (identical on every rank)."""
        oq, s_q = [0] * self.n_nodes, 0
        for r in range(self.world):
            lo, hi, _ = shard(self.n_nodes, self.world, r)
            o = 0
            for q in range(lo, hi):
                oq[q] = o
                o += self._sq_words(self._lay[q][1] or self.M)
            s_q = max(s_q, o)
        return oq, max(ALIGN, s_q)

    def _squant_rows(self):
        rows = []
        for q in range(self.lo, self.hi):
            count = self._lay[q][1] or self.M
            o = self._s_idx + self._oq[q]
            rows.append((count, self.send[o:o + self._sq_words(count)]))
        return rows

    def _squant_exchange_decode(self):
        """ONE decode of every gathered row this rank folds into its place in ``_dvals``."""
        buf = self.recv if self.coll else self.send
        W = self._s_idx + self._s_q
        for j, q in enumerate(self._sq_nodes):
            _, k, _, pv = self._place(q)
            count = k or self.M
            r = q // self.per if self.coll else 0
            self._sq_dec.set(j, buf.data_ptr() + 4 * (r * W + self._s_idx + self._oq[q]), count,
                             self._dvals.data_ptr() + 4 * pv, self._sq_words(count))
        self._sq_dec.upload()
        self._squant_decode(self._sq_dec, self.guard)

    def payload(self, q):
        """``(idx or None, vals)`` of node q's payload of the last round (an owned node; any
        node after an all-gather).  A full share has no indices."""
        partial, k, pi, pv = self._place(q)
        buf = self.recv if self.coll else self.send
        if self._squant:  # what the receivers decoded
            return buf[pi:pi + k] if partial else None, self._dvals[pv:pv + (k or self.M)]
        if partial:
            return buf[pi:pi + k], buf[pv:pv + k].view(torch.float32)
        if not self.coll:
            return None, self.wx[q - self.lo]  # the full W(x), no copy on one rank
        return None, buf[pv:pv + self.M].view(torch.float32)

    # ---- the wire layer's hooks (gossip_round.WireCoded) --------------------------------------
    def _wire_views(self):
        vals = self.send[self._s_idx:self._s_idx + self._s_val].view(torch.float32)
        views = []
        for j in range(self.m):
            partial, k, oi, ov = self._lay[self.lo + j]
            if self._squant:  # the selection's own values, at the index offsets
                vals, ov = self._vraw, oi
            views.append((self.send[oi:oi + k], vals[ov:ov + k]) if partial
                         else (None, self.wx[j]))
        return self.M, views

    def _wire_message(self, q, indices, params):
        if indices is None:  # Wavelet.py:185-192: a full share carries its coefficients only
            return {"params": params}
        return {"alpha": self.alphas[q], "params": params, "indices": indices,
                "send_partial": True}  # key order of reference Wavelet.py:223-229

    # ---- the legs of a round -----------------------------------------------------------------
    def encode(self):
        """W(x), W(x - x0) and the payload of every owned node; acc and the counter updated."""
        m, M = self.m, self.M
        self._wire_reset()
        if not m:
            return
        if self._hip:
            from . import codec
            base = self.send.data_ptr()
            for j in range(m):
                partial, k, oi, ov = self._lay[self.lo + j]
                pv = base + 4 * (self._s_idx + ov)
                if self._squant:
                    # the values stay here: the quantiser reads them (a full share's from wx)
                    pv = self._vraw.data_ptr() + 4 * oi if partial else 0
                    o = self._s_idx + self._oq[self.lo + j]
                    self._sq_enc.set(j, pv or self.wx[j], k or M, base + 4 * o,
                                     self._sq_words(k or M))
                if partial and self.selection == "window":
                    # the prior slot: the drawn alpha's place in alpha_list
                    self._enc.set(j, k, base + 4 * oi, pv,
                                  self.alpha_list.index(self.alphas[self.lo + j]))
                elif partial:
                    self._enc.set(j, k, base + 4 * oi, pv)
                else:  # Wavelet.py:185-192: all of W(x); copied only where it is gathered
                    self._enc.set(j, 0, 0, pv if self.coll else 0)
            self._enc.upload()
            if self._squant:
                self._sq_enc.upload()
            self._transform_pair(codec)
            if self.selection == "window" and self._kmax:
                self._sel_ws = codec.jwins_encode_nodes_window(self._enc, M, self._kmax,
                                                               self._sel_ws)
            else:
                codec.jwins_encode_nodes(self._enc, M, self._ws)
            if self._squant:
                self._squant_encode(self._sq_enc)
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

    def selection_status(self):
        """The last encode's status per owned node, an int32 tensor on the engine's device: 0 =
        exact (no prior for the drawn alpha yet, or a full share), 1 = window hit, 2 = window
        miss, then exact.  Reading it is the caller's synchronisation."""
        if self._sel_ws is None:
            return self._exact_status
        from . import codec
        return codec.window_status(self._sel_ws, self.m)

    def exchange(self):
        """ONE all-gather of this rank's ``[idx block | val block]``."""
        if self.coll:
            W = self._s_idx + (self._s_q if self._squant else self._s_val)
            self.all_gather(self.recv[:self.world * W], self.send[:W])
        if self._squant and self.m:
            self._squant_exchange_decode()

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
        vbase = self._dvals.data_ptr() if self._squant else base
        wx0, wstep = self.wx.data_ptr(), self.wx.stride(0) * 4
        idx, val, kk = [], [], []
        for nbrs, _, _ in self.weights:
            for q in nbrs:
                partial, k, pi, pv = self._place(q)
                if partial:
                    idx.append(base + 4 * pi)
                    val.append(vbase + 4 * pv)
                    kk.append(k)
                else:
                    idx.append(None)
                    val.append(vbase + 4 * pv if self.coll or self._squant
                               else wx0 + (q - self.lo) * wstep)
                    kk.append(M)
        ft, tot = self._fold_tab, self._tot
        idx_a, val_a = (ctypes.c_void_p * tot)(*idx), (ctypes.c_void_p * tot)(*val)
        k_a = (ctypes.c_int64 * tot)(*kk)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L = _lib.lib()
        rc = L.dpz_decode_average_batch_guarded(
            m, ft["local"], ft["out"], M, ft["np"], idx_a, val_a, k_a, ft["w"], ft["w_self"],
            _lib.DPZ_FOLD_SELF, self._guard.data_ptr(), self._guard.numel(), stream)
        if rc == _lib.DPZ_ERR_UNSUPPORTED and self._squant:
            raise _lib.CodecError("compression='EliasQuantization' folds behind the decode's "
                                  "status words: M >= 1024, two owned nodes or more, every node "
                                  "with a neighbour")
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
            self._transform_post(codec)
        else:
            for j in range(self.m):
                self.ops.inverse(self.wc[j], self.N, self.x[j])
                self.ops.accumulate(self.acc[j], self.x[j], self.x0[j])
        self._x0buf.copy_(self._xbuf)  # every row at once, the rows' padding included

    def draw(self):
        """Every node's alpha of the coming round and the layout of the round's payloads."""
        self.alphas = [rng.choice(self.alpha_list) for rng in self.rngs]
        self._lay, self._s_idx, self._s_val = JwinsRound._layout(self, self.alphas)
        if self._squant:
            self._oq, self._s_q = self._sq_layout()

    def step(self, mark=None):
        """One round.  Nothing synchronises with the host.  ``mark(leg)`` is called after each of
        ``LEGS`` is enqueued (tools/bench_jwins_round.py records an event)."""
        mark = mark or (lambda leg: None)
        self.draw()
        self.encode()
        mark("encode")
        self.exchange()
        mark("exchange")
        self.fold()
        mark("fold")
        self.post()
        mark("post")
        self.round += 1


def wavelet_coeff_len(n, level, flen):
    """Length of pywt's concatenated ``wavedec`` array of n values for a filter of ``flen`` taps
    (mode "symmetric"), len_l = (len_{l-1} + flen - 1) // 2, or None where a level's input is
    shorter than the filter (the generic kernels' rule, computed without the library)."""
    lens, cur = [], int(n)
    for _ in range(level):
        if cur < flen:
            return None
        cur = (cur + flen - 1) // 2
        lens.append(cur)
    return sum(lens) + lens[-1]


class JwinsWaveletBatchRound(JwinsBatchRound):
    """``JwinsBatchRound`` for every (wavelet, level) the generic-filter kernels serve: every name
    of the filter table (db1-32, sym2-20, coif1-10, bior / rbio, dmey; ``db1`` for the Haar
    filters) at levels 1-8 except sym2 at levels 1-4.  Same constructor, state rows, ``payload()``,
    legs and ``step()``; the three transforms are ``level`` launches each, whatever the node
    count, on ``dpz_dwt_generic_nodes`` / ``dpz_idwt_generic_nodes`` with one workspace allocated
    here."""

    @staticmethod
    def _check_config(wavelet, level):
        from . import codec
        if wavelet == "haar":
            raise ValueError("wavelet 'haar' runs the fused haar kernels node after node: use "
                             "gossip_jwins.JwinsRound (or 'db1', the same filters, here)")
        codec._check_wavelet(wavelet)
        if level not in range(1, 9):
            raise NotImplementedError(f"{wavelet} level-{level} wavedec unsupported: the device "
                                      "kernels run levels 1-8")
        if codec._fused(wavelet, level):
            raise ValueError(f"wavelet {wavelet!r} at level {level} runs the fused kernels: use "
                             "gossip_jwins_batch.JwinsBatchRound")

    def _coeff_len(self):
        from . import codec
        M = wavelet_coeff_len(self.N, self.level, codec.filter_len(self.wavelet))
        if M is None:
            # Wavelet's documented case: a level whose input is shorter than the filter
            raise NotImplementedError(
                f"{self.wavelet} level-{self.level} wavedec unsupported for n={self.N}")
        return M

    def _make_transform_tables(self, codec, dev):
        super()._make_transform_tables(codec, dev)
        self._wws = codec.wavelet_nodes_workspace(self.m, self.N, self.level, self.wavelet, dev)

    def _transform_pair(self, codec):
        codec.dwt_generic_nodes(self._pair, self.N, self.level, self.wavelet,
                                workspace=self._wws)

    def _transform_post(self, codec):
        codec.idwt_generic_nodes(self._inv, self.N, self.level, self.wavelet,
                                 workspace=self._wws)
        codec.dwt_generic_nodes(self._post, self.N, self.level, self.wavelet, accumulate=True,
                                workspace=self._wws)
