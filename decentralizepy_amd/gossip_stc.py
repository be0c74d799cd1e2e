"""One synchronous STC round of a whole federation on the GPU.

In the reference every client is a process (``node/STC/STCClient.py``) whose ``sharing/STC.py``
keeps two N-float states across rounds, ``prev_model`` and ``residuals``, and one more process is
the server (``node/STC/STCServer.py``) with a model and a residual of its own.  A round: every
working client sends the exact top-k, k = round(alpha N), of ``c = (x - prev) + residuals`` and
keeps ``c`` minus what it sent (:259-270, :308-316); the server averages the payloads in the order
of its working set, ``total += (1 / n) T_j`` from zeros, forms ``c_s = residuals_s + total``
(:333-362), broadcasts the top-k of ``c_s``, keeps the rest as its residual and adds the broadcast
to its model (:318-331); every working client adds the broadcast to its model (:281-306).

This engine keeps x, prev and r of every owned client resident in HBM, shards the clients over the
ranks like ``gossip.GossipRound`` and REPLICATES the server: every rank holds ``server_x`` and
``server_r`` and runs the server's leg on the gathered rows, so one collective per round suffices
(the kernels are deterministic: the replicas agree in every bit).  A round is
``dpz_stc_encode_nodes`` over the owned workers (one launch set whatever their count), ONE
``all_gather_into_tensor`` of a packed row per client, ONE ``dpz_stc_server_fold`` launch over the
workers' rows in the given order, the encode launch set once more with the server's residual in
server form into a broadcast row, and ONE ``dpz_stc_apply_nodes`` launch over the owned workers'
models and the server's.  Nothing synchronises with the host inside ``step()``.

Finite models only (a non-finite change is sent and then cleared, where the reference's ``c - c``
leaves NaN behind).  An element of a model that the broadcast does not name keeps its bits; the
reference's dense ``flat + T`` turns a -0.0 there into +0.0.

The encode / server_fold / apply callables are injectable together so the sharding and exchange
logic can be tested with the CPU gloo backend; the defaults are the HIP codec (no CPU fallback).
"""
import torch

from .gossip_round import PackedRowRound, up4

HEADER = PackedRowRound.HEADER


class StcRound(PackedRowRound):
    """Clients [lo, hi) of a federation on this rank and a replica of the server; ``step()`` runs
    one STC round.  ``x`` is a writable view of the owned clients' models: the caller applies its
    local training to it between rounds."""

    def __init__(self, n_clients, x_init, server_init, alpha, rank=0, world=1, group=None,
                 device=None, encode=None, server_fold=None, apply=None, **unknown):
        """x_init: (hi - lo, N) fp32 tensor, this rank's clients' flat models; server_init: the
        server's flat model (N).  ``encode(x, prev, r, k) -> (idx, vals)`` (one node, in place on
        prev and r; x None: the server form), ``server_fold(r_s, [(idx, vals)], w)`` (in place)
        and ``apply(x, idx, vals)`` (one model, in place) are injectable (CPU tests)."""
        if unknown:
            raise ValueError(f"unknown arguments {sorted(unknown)}: payload compression, the peer "
                             "exchange and a non-replicated server are not implemented")
        injected = [f is not None for f in (encode, server_fold, apply)]
        if any(injected) != all(injected):
            raise ValueError("encode, server_fold and apply are injected together")
        # a star: no client-to-client edges
        super().__init__([set() for _ in range(int(n_clients))], x_init, rank, world, group,
                         device)
        m, N = self.m, self.N
        self.alpha = float(alpha)
        if not self.alpha <= 1.0:
            raise ValueError("alpha must lie in (0, 1]")
        self.k = round(self.alpha * N)
        if self.k < 1:
            raise ValueError(f"k = round(alpha N) = {self.k}: an empty payload is not a round")
        if server_init.numel() != N:
            raise ValueError(f"server_init holds {server_init.numel()} values, the models {N}")
        self._hip = not any(injected)
        self._encode, self._server_fold, self._apply = encode, server_fold, apply
        self.cap = up4(self.k)
        f32 = dict(dtype=torch.float32, device=self.device)
        stride = up4(N)  # every row 16-byte aligned
        self._state = torch.zeros(3, max(1, m), stride, **f32)
        self.x = self._state[0, :m, :N]
        self.prev = self._state[1, :m, :N]
        self.r = self._state[2, :m, :N]
        self.x.copy_(x_init)
        self.prev.copy_(x_init)
        self._server = torch.zeros(2, stride, **f32)
        self.server_x = self._server[0, :N]
        self.server_r = self._server[1, :N]
        self.server_x.copy_(server_init.reshape(-1))
        # a packed row: [count = k (int64), status = 0, 0 | cap idx | cap vals]
        self._alloc_rows(HEADER + 2 * self.cap)
        self.bcast = torch.zeros(self.row_words, dtype=torch.int32, device=self.device)
        self._plans = {}
        self._server_tab = self._ws = self._ws1 = None

    # ---- views of the packed rows ---------------------------------------------------------------
    def _pay(self, row):
        return (row[HEADER:HEADER + self.k],
                row[HEADER + self.cap:HEADER + self.cap + self.k].view(torch.float32))

    def payload(self, q):
        """``(idx, vals)`` of client q's payload of its last encode (an owned client; any client
        after an all-gather)."""
        return self._pay(self._row(q))

    def broadcast(self):
        """``(idx, vals)`` of the server's last broadcast."""
        return self._pay(self.bcast)

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

    # ---- the plan of a working set --------------------------------------------------------------
    def _plan(self, workers):
        """The tables of a working set, built once per ``tuple(workers)``."""
        workers = tuple(int(q) for q in (range(self.n_nodes) if workers is None else workers))
        plan = self._plans.get(workers)
        if plan is not None:
            return plan
        if not workers:
            raise ValueError("an STC round needs at least one worker")
        if len(set(workers)) != len(workers):
            raise ValueError(f"duplicate workers in {list(workers)}")
        if min(workers) < 0 or max(workers) >= self.n_nodes:
            raise ValueError(f"a worker outside [0, {self.n_nodes}) in {list(workers)}")
        plan = dict(workers=workers, weight=1.0 / len(workers),
                    owned=[q - self.lo for q in workers if self.lo <= q < self.hi])
        if self._hip:
            from . import codec
            own = plan["owned"]
            plan["enc"] = codec.stc_node_table(
                [self.x[j] for j in own], [self.prev[j] for j in own],
                [self.r[j] for j in own], [self.send[j] for j in own]) if own else None
            plan["fold"] = codec.StcFoldTable([(self._row(q), plan["weight"]) for q in workers],
                                              self.device)
            plan["apply"] = codec.stc_apply_table([self.x[j] for j in own] + [self.server_x])
        self._plans[workers] = plan
        return plan

    # ---- the legs of a round --------------------------------------------------------------------
    def encode(self, plan):
        """Every owned worker's top-k of ``(x - prev) + r`` into its row; prev and r updated."""
        if self._hip:
            from . import codec
            if plan["enc"] is not None:
                self._ws = codec.stc_encode_nodes(plan["enc"], self.N, self.k, self._ws)
            return
        for j in plan["owned"]:
            self._write_row(self.send[j], *self._encode(self.x[j], self.prev[j], self.r[j],
                                                        self.k))

    def exchange(self):
        """ONE all-gather of the packed rows (the rows carry no status: every row holds k)."""
        if self.coll:
            self.all_gather(self.recv, self.send)

    def server_fold(self, plan):
        """``server_r += sum (1 / n) T_j`` over the workers' rows in the plan's order."""
        if self._hip:
            from . import codec
            codec.stc_server_fold(plan["fold"], self.N, self.k, self.server_r)
            return
        self._server_fold(self.server_r, [self._pay(self._row(q)) for q in plan["workers"]],
                          plan["weight"])

    def server_encode(self):
        """The top-k of the server's change vector into the broadcast row; the rest stays."""
        if self._hip:
            from . import codec
            if self._server_tab is None:
                self._server_tab = codec.stc_node_table(None, None, [self.server_r], [self.bcast])
            self._ws1 = codec.stc_encode_nodes(self._server_tab, self.N, self.k, self._ws1)
            return
        self._write_row(self.bcast, *self._encode(None, None, self.server_r, self.k))

    def apply(self, plan):
        """The broadcast added to the owned workers' models and the server's, in place."""
        if self._hip:
            from . import codec
            codec.stc_apply_nodes(plan["apply"], self.N, self.k, self.bcast)
            return
        idx, vals = self.broadcast()
        for j in plan["owned"]:
            self._apply(self.x[j], idx, vals)
        self._apply(self.server_x, idx, vals)

    def step(self, workers=None, mark=None):
        """One round of the working set ``workers`` (distinct client numbers; their order is the
        server's fold order; default: every client, ascending): the encode launch set, one
        all-gather (with a process group), one server fold launch, the server's encode launch
        set, one apply launch.  Clients outside ``workers`` are neither read nor written.  Nothing
        synchronises with the host.  ``mark(leg)`` is called after each leg is enqueued
        (tools/bench_stc_round.py records an event)."""
        mark = mark or (lambda leg: None)
        plan = self._plan(workers)
        self.encode(plan)
        mark("encode")
        self.exchange()
        mark("exchange")
        self.server_fold(plan)
        mark("fold")
        self.server_encode()
        mark("broadcast")
        self.apply(plan)
        mark("apply")
        self.round += 1
