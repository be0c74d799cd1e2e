"""What the whole-topology round engines (gossip.py, gossip_jwins.py, gossip_jwins_batch.py,
gossip_subsampling.py, gossip_epidemic.py, gossip_choco.py, gossip_quant.py, gossip_stc.py,
gossip_topkacc.py, gossip_fft.py) share:
``ShardedRound``, the sharding of the nodes over the ranks, ``PackedRowRound``, the packed row
per node that one all-gather exchanges, and ``WireCoded``, the EliasFpzip wire streams of a round's
payloads in one batched call and the exchange that carries them, and the EliasQuantization
exchange (``compression="EliasQuantization"``): the payloads' values through the reference's
quantiser, one batched call each way."""
import math
import pickle

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


class WireCoded:
    """The wire layer of an engine whose payloads are ``(idx or None, vals)`` lists with counts the
    host knows: what the per-node plugins would send with ``compression_class = EliasFpzip`` (the
    reference's ``compression/EliasFpzip.py``), coded for all owned nodes by ONE
    ``codec.wire_encode_nodes`` call.  The engine calls ``_init_wire`` from its constructor and
    ``_wire_reset`` from ``encode()``, sets ``_hip`` and provides two hooks:

    * ``_wire_views()``: ``(n, [(idx or None, vals), ...])``, device views of the owned nodes'
      payloads of the last encode in node order, indices below n;
    * ``_wire_message(q, indices, params)``: the dict the plugin puts on the wire for node q
      (``indices`` None for a full share)."""

    COMPRESSIONS = (None, "EliasQuantization")

    def _init_wire(self, float_precision, partial_ks, coded_exchange=False, compression=None):
        if compression not in self.COMPRESSIONS:
            raise ValueError(f"compression {compression!r}: None or 'EliasQuantization' (the "
                             "EliasFpzip streams are wire_payload() / coded_exchange)")
        self._squant = compression is not None
        if self._squant:
            # float_precision is the quantiser's k, as Sharing.__init__ hands it to the compressor
            k = float_precision
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
                raise TypeError(f"float_precision must be an int, got {type(k).__name__}")
            if not 1 <= int(k) <= 2 ** 30:
                raise ValueError("float_precision must be in [1, 2^30]")
            if coded_exchange:
                raise ValueError("coded_exchange carries the EliasFpzip streams: not with "
                                 "compression='EliasQuantization'")
            if not self._hip:
                raise NotImplementedError("compression='EliasQuantization' quantises with the HIP "
                                          "codec only; the CPU stand-in has no quantiser")
        self.compression = compression
        self.float_precision = int(float_precision)
        if self.float_precision < 0:
            raise ValueError("float_precision must be >= 0 (0 or >= 32: lossless)")
        self._coded = bool(coded_exchange)
        if self._coded and not self._hip:
            raise NotImplementedError("coded_exchange codes the rows with the HIP codec only; the "
                                      "CPU stand-in has no coder")
        if self._coded and any(k < 2 for k in partial_ks):
            raise ValueError(f"coded_exchange with a share of k = {min(partial_ks)} indices: the "
                             "Elias index stream needs two")
        # a one-index share is a valid round (the engines have always run it) but has no Elias
        # stream: the configuration is refused where the wire layer is asked for
        self._wire_low = min((k for k in partial_ks if k < 2), default=None)
        self._wire_tab = self._wire_ws = self._wire_sizes = self._wire_streams = None
        self._wire_encoded = False

    def _wire_reset(self):
        """A new encode: what was coded for the last one is void."""
        self._wire_encoded = True
        self._wire_sizes = self._wire_streams = None

    def _wire_call(self, slots):
        """One batched call over the owned nodes; with ``slots`` into per-node slots of one new
        buffer.  Returns (sizes, status, buffer or None, [(idx offset or None, val offset)])."""
        if self._wire_low is not None:
            raise ValueError(f"a partial share of k = {self._wire_low} indices: the Elias index "
                             "stream needs two (the reference's Elias.compress raises IndexError)")
        if not self._hip:
            raise NotImplementedError("the wire streams are coded by the HIP codec only; the CPU "
                                      "stand-in has no coder")
        if not self._wire_encoded:
            raise RuntimeError("no round has been encoded yet")
        from . import codec
        n, views = self._wire_views()
        m = len(views)
        if self._wire_tab is None:
            self._wire_tab = codec.WireNodesTable(m, self.device)
        lib = codec._lib.lib()
        caps, total = [], 0
        for idx, vals in views if slots else ():
            ci = codec.elias_bound_bytes(vals.numel(), n) if idx is not None else 0
            cv = int(lib.dpz_fpz_max_bytes(vals.numel()))
            caps.append((total, ci, total + ci, cv))
            total += ci + cv
        buf = torch.empty(max(4, total), dtype=torch.uint8, device=self.device) if slots else None
        for j, (idx, vals) in enumerate(views):
            if slots:
                oi, ci, ov, cv = caps[j]
                base = buf.data_ptr()
                self._wire_tab.set(j, idx, vals, vals.numel(), base + oi if ci else 0, base + ov,
                                   ci, cv)
            else:
                self._wire_tab.set(j, idx, vals, vals.numel())
        self._wire_tab.upload()
        sizes = torch.empty(max(1, m), 2, dtype=torch.int64, device=self.device)
        status = torch.empty(max(1, m), dtype=torch.int32, device=self.device)
        if m:
            self._wire_ws = codec.wire_nodes_workspace(
                m, max(v.numel() for _, v in views), self.device, self._wire_ws)
            codec.wire_encode_nodes(self._wire_tab, sizes, status,
                                    0 if self._squant else self.float_precision, self._wire_ws)
        if self._squant:  # the values travel quantised: the reference's ``to_send``
            sizes[:m, 1] = self._squant_value_bytes()
        self._wire_sizes = sizes[:m]
        return sizes[:m], status[:m], buf, [(oi if ci else None, ov) for oi, ci, ov, _ in caps]

    # ---- the coded exchange: rows of equal k, PackedRowRound's layout ---------------------------
    def _init_coded(self, k, n, idx_word, val_word):
        """After ``_alloc_rows``: the coded rows and the two static tables of an engine whose raw
        row holds k ascending indices below n from int32 word ``idx_word`` and k values from
        ``val_word``.  A coded row is ``[count int64, status, 0 | index bytes int64, value bytes
        int64 | index slot | value slot]`` with slots of up4(``dpz_elias_bound_bytes(k, n)``) and
        ``dpz_fpz_bound_bytes(k, float_precision)`` bytes.  ``csend`` holds this rank's, ``crecv``
        every rank's after the all-gather (``csend`` itself without collectives); the decode
        writes raw-layout rows into ``recv``, which the folds then read (``rows``)."""
        from . import codec
        H, i32 = PackedRowRound.HEADER, dict(dtype=torch.int32, device=self.device)
        ci, cv = up4(codec.elias_bound_bytes(k, n)), codec.fpz_bound_bytes(k, self.float_precision)
        oi, ov = 4 * (H + 4), 4 * (H + 4) + ci
        self._cslots = (oi, ov)
        self.csend = torch.zeros(self.per, up4(H + 4 + (ci + cv) // 4), **i32)
        self.crecv = torch.zeros(self.per * self.world, self.csend.shape[1],
                                 **i32) if self.coll else self.csend
        self.csend[:, :2] = torch.tensor([k], dtype=torch.int64).view(torch.int32).to(self.device)
        if self.recv is None:
            self.recv = torch.zeros(self.per * self.world, self.row_words, **i32)
        m = self.m
        self._enc_tab = codec.WireNodesTable(m, self.device)
        for j in range(m):
            raw, c = self.send[j].data_ptr(), self.csend[j].data_ptr()
            self._enc_tab.set(j, raw + 4 * idx_word, raw + 4 * val_word, k, c + oi, c + ov, ci, cv)
        self._enc_tab.upload()
        self._enc_sizes = torch.zeros(max(1, m), 2, dtype=torch.int64, device=self.device)
        self._enc_status = torch.zeros(max(1, m), **i32)
        self._enc_ws = codec.wire_nodes_workspace(max(1, m), k, self.device)
        # the static set of nodes this rank's neighbourhoods fold
        nodes = sorted({q for i in range(self.lo, self.hi) for q in self.adj[i]})
        self._dec_tab = codec.WireDecodeTable(len(nodes), self.device)
        for j, q in enumerate(nodes):
            raw, c = self.recv[q].data_ptr(), self.crecv[q].data_ptr()
            self._dec_tab.set(j, c + oi, c + ov, k, raw + 4 * idx_word, raw + 4 * val_word,
                              c + 4 * H, ci, cv)
        self._dec_tab.upload()
        self._dec_status = torch.zeros(max(1, len(nodes)), **i32)
        self._dec_all = nodes == list(range(self.per * self.world))
        self._dec_nodes = torch.tensor(nodes, dtype=torch.int64, device=self.device)
        self._dec_ws = codec.wire_decode_workspace(max(1, len(nodes)), ci, k, self.device)

    def _coded_encode(self):
        """After the selection: ONE ``wire_encode_nodes`` call from the raw rows into the coded
        rows' slots; the stream lengths go into the rows' header words and the coder's status is
        ORed into the rows' status words."""
        from . import codec
        m, H = self.m, PackedRowRound.HEADER
        if not m:
            return
        codec.wire_encode_nodes(self._enc_tab, self._enc_sizes, self._enc_status,
                                self.float_precision, self._enc_ws)
        self.csend[:m, H:H + 4].copy_(self._enc_sizes[:m].view(torch.int32))
        torch.bitwise_or(self.send[:m, 2], self._enc_status[:m], out=self.csend[:m, 2])

    # ---- the EliasQuantization exchange ----------------------------------------------------------
    # What the engines share: the two tables' calls, and the wire view of a quantised row.  An
    # engine provides ``_squant_rows()``: per owned node (count, its coded row [8 info words |
    # body] as an int32 view) of the last encode.
    def _squant_encode(self, table):
        """ONE ``squant_encode_nodes`` call over the owned nodes' value lists."""
        from . import codec
        if table.m:
            self._sq_ws, _ = codec.squant_encode_nodes(table, self.float_precision,
                                                       getattr(self, "_sq_ws", None))

    def _squant_decode(self, table, status):
        """ONE ``squant_decode_nodes`` call over the gathered rows this rank folds."""
        from . import codec
        if table.m:
            codec.squant_decode_nodes(table, status)

    def _squant_value_bytes(self):
        """Device int64 (m): 2 + ceil(count w / 8), the length of the reference's ``to_send``."""
        rows = self._squant_rows()
        if not rows:
            return torch.zeros(0, dtype=torch.int64, device=self.device)
        w = torch.stack([row[1] for _, row in rows]).to(torch.int64)
        counts = torch.tensor([c for c, _ in rows], dtype=torch.int64).to(self.device)
        return 2 + (counts * w + 7) // 8

    def _squant_params(self, q):
        """Owned node q's quantised values as the plugin's wire value: ``pickle((np.float32(scale),
        uint8[padding, w, body...]))`` (compression/Quantization.py).  Blocks."""
        count, row = self._squant_rows()[q - self.lo]
        info = row[:8].cpu().numpy()
        if info[0]:
            raise RuntimeError(f"quantised values of node {q} refused (status {int(info[0])})")
        w, pad = int(info[1]), int(info[2])
        nbytes = (count * w + 7) // 8
        body = row[8:8 + (nbytes + 3) // 4].cpu().numpy().view(np.uint8)[:nbytes]
        to_send = np.concatenate([np.array([pad, w], dtype=np.uint8), body])
        return pickle.dumps((info[3:4].view(np.float32)[0], to_send))

    # ---- the EliasQuantization exchange of rows of equal k, PackedRowRound's layout -------------
    def _init_squant_rows(self, k, idx_words, val_word):
        """After ``_alloc_rows``: a coded row is ``[header | idx_words raw int32 index words | 8
        info words | body]``, the raw row's first ``HEADER + idx_words`` words followed by the
        quantised row of its k values at ``val_word``.  ``csend`` holds this rank's, ``crecv``
        every rank's after the all-gather; the decode writes the values into the raw-layout rows
        of ``recv``, which the folds read with the indices of ``crecv``."""
        from . import codec
        H, i32 = PackedRowRound.HEADER, dict(dtype=torch.int32, device=self.device)
        self._sq_head = H + idx_words
        self._sq_slot = slot = up4(codec.squant_row_words(k, self.float_precision))
        self.csend = torch.zeros(self.per, self._sq_head + slot, **i32)
        self.crecv = torch.zeros(self.per * self.world, self.csend.shape[1],
                                 **i32) if self.coll else self.csend
        if self.recv is None:
            self.recv = torch.zeros(self.per * self.world, self.row_words, **i32)
        self._enc_tab = codec.SquantTable(self.m, self.device)
        for j in range(self.m):
            self._enc_tab.set(j, self.send[j].data_ptr() + 4 * val_word, k,
                              self.csend[j].data_ptr() + 4 * self._sq_head, slot)
        self._enc_tab.upload()
        nodes = sorted({q for i in range(self.lo, self.hi) for q in self.adj[i]})
        self._dec_tab = codec.SquantTable(len(nodes), self.device)
        for j, q in enumerate(nodes):
            self._dec_tab.set(j, self.crecv[q].data_ptr() + 4 * self._sq_head, k,
                              self.recv[q].data_ptr() + 4 * val_word, slot)
        self._dec_tab.upload()
        self._dec_status = torch.zeros(max(1, len(nodes)), **i32)
        self._dec_all = nodes == list(range(self.per * self.world))
        self._dec_nodes = torch.tensor(nodes, dtype=torch.int64, device=self.device)
        self._sq_k = k

    def _squant_rows(self):
        return [(self._sq_k, self.csend[j, self._sq_head:]) for j in range(self.m)]

    def _squant_rows_encode(self):
        """After the selection: the header and index words copied, the values quantised."""
        m = self.m
        if m:
            self.csend[:m, :self._sq_head].copy_(self.send[:m, :self._sq_head])
            self._squant_encode(self._enc_tab)

    @property
    def rows(self):
        """The rows the folds read: the decoded ones with a coded exchange."""
        return self.recv if self._coded or self._squant else super().rows

    @property
    def idx_rows(self):
        """The rows whose index words the folds read: with the EliasQuantization exchange the
        gathered rows themselves (the indices travel raw)."""
        return self.crecv if self._squant else self.rows

    def exchange(self):
        """With ``coded_exchange``: ONE all-gather of the coded rows (in place with one rank and no
        group), then ONE ``wire_decode_nodes`` call into the raw-layout receive buffer; the decode
        status is ORed into the guard words of the guarded fold."""
        if not self._coded and not self._squant:
            return super().exchange()
        from . import codec
        if self.coll:
            self.all_gather(self.crecv, self.csend)
        if self._squant:
            # one decode of every gathered row this rank folds; a refused row (the sender's
            # quantiser status, a bad width, a count past the slot) goes into the guard words
            self._squant_decode(self._dec_tab, self._dec_status)
            if self._dec_all:
                return torch.bitwise_or(self.crecv[:, 2], self._dec_status, out=self.guard)
            self.guard.copy_(self.crecv[:, 2])
            if self._dec_tab.m:
                self.guard[self._dec_nodes] |= self._dec_status
            return None
        if not self._dec_tab.m:
            return self.guard.copy_(self.crecv[:, 2])
        codec.wire_decode_nodes(self._dec_tab, self._dec_status, self.float_precision,
                                self._dec_ws)
        if self._dec_all:
            torch.bitwise_or(self.crecv[:, 2], self._dec_status, out=self.guard)
        else:
            self.guard.copy_(self.crecv[:, 2])
            self.guard[self._dec_nodes] |= self._dec_status

    def _coded_stream(self, q):
        """Owned node q's coded row on the host, sliced into (indices, params).  Blocks."""
        H = PackedRowRound.HEADER
        row = self.csend[q - self.lo].cpu().numpy().view(np.uint8)
        nb_i, nb_v = row[4 * H:4 * H + 16].view(np.int64).tolist()
        if row[8:12].view(np.int32)[0]:
            raise RuntimeError(f"wire streams of node {q} refused (status "
                               f"{int(row[8:12].view(np.int32)[0])})")
        oi, ov = self._cslots
        return row[oi:oi + nb_i].copy(), row[ov:ov + nb_v].copy()

    def wire_bytes(self):
        """Device int64 ``(m, 2)``: the bytes of the index stream (0 for a full share) and of the
        value stream of every owned node's payload of the last ``encode()`` / ``step()``, as
        ``EliasFpzip`` codes them at this engine's ``float_precision``.  One batched size-only
        call of two launches; nothing synchronises with the host.  The pickle framing that the
        reference's ``TCP.encrypt`` adds is not counted: it is made on the host and is the same
        for every message of a configuration.
        With ``compression="EliasQuantization"`` the second column is ``2 + ceil(count w / 8)``,
        the length of the uint8 array ``to_send`` of the reference's quantiser at the width w the
        node's values gave; the pickle framing of ``(scale, to_send)`` is excluded as well."""
        if self._coded:  # the coded rows' header words: nothing is launched
            if not self._wire_encoded:
                raise RuntimeError("no round has been encoded yet")
            H = PackedRowRound.HEADER
            return self.csend[:self.m, H:H + 4].view(torch.int64)
        if self._wire_sizes is None:
            self._wire_call(False)
        return self._wire_sizes

    def wire_payload(self, q):
        """The dict the per-node plugin would put on the wire for owned node q after the last
        ``encode()`` / ``step()``: ``params`` (and ``indices`` of a partial share) as uint8 numpy
        streams that ``compression.EliasFpzip`` decodes, ``alpha`` and ``send_partial`` as the
        plugin sets them.  The first call after an encode codes every owned node in one batched
        call, into slots of ``dpz_elias_bound_bytes`` / ``dpz_fpz_max_bytes`` bytes, and brings
        the streams to the host (one synchronisation); later calls read that cache."""
        if not self.lo <= q < self.hi:
            raise ValueError(f"node {q} is not one of this rank's nodes [{self.lo}, {self.hi})")
        if self._coded:  # a slice of the coded row that was exchanged
            if not self._wire_encoded:
                raise RuntimeError("no round has been encoded yet")
            return self._wire_message(q, *self._coded_stream(q))
        if self._wire_streams is None:
            sizes, status, buf, offs = self._wire_call(True)
            host = torch.empty(buf.numel(), dtype=torch.uint8, pin_memory=True)
            host.copy_(buf, non_blocking=True)
            sizes, status = sizes.cpu().numpy(), status.cpu().numpy()  # waits for all three
            if status.any():
                raise RuntimeError(f"wire streams of nodes {np.flatnonzero(status).tolist()} "
                                   f"refused (status {status[status != 0].tolist()})")
            host = host.numpy()
            self._wire_streams = [
                (None if oi is None else host[oi:oi + nb_i].copy(), host[ov:ov + nb_v].copy())
                for (oi, ov), (nb_i, nb_v) in zip(offs, sizes.tolist())]
        indices, params = self._wire_streams[q - self.lo]
        if self._squant:  # compression.EliasQuantization decodes it: Elias indices, pickled values
            params = self._squant_params(q)
        return self._wire_message(q, indices, params)


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
