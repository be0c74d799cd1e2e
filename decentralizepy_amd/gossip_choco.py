"""One synchronous Choco-SGD gossip round of a whole topology on the GPU.

In the reference every node is a process whose ``sharing/Choco.py`` keeps two N-float states
across rounds, ``model_hat`` (x_hat) and ``s``.  A round (:359-453) sparsifies ``x - x_hat`` at
the k-th largest magnitude, k = round(alpha N), keeping every tie (:186-207), sends the nonzero
entries, and on receipt does ``x_hat += q``; ``s += w_i T_i`` over the neighbours in the order of
``peer_deques`` with Metro-Hastings weights, ``s += (1 - sum w) q``; ``x += step_size (s - x_hat)``.

This engine keeps x, x_hat and s of every owned node resident in HBM, shards the nodes over the
ranks like ``gossip.GossipRound`` and runs a round of all owned nodes as ``dpz_choco_encode_nodes``
(one launch set whatever the node count) into fixed slots, ONE ``all_gather_into_tensor`` of a
packed row per node, and ONE ``dpz_choco_fold_nodes`` launch guarded by the rows' status words.
Nothing synchronises with the host inside ``step()``; ``check()`` reads the status words.

The slot holds ``min(N, k + max(64, k // 8))`` entries (rounded up to 4): the selection keeps every
tie at the threshold, so it has at least k entries and more when |x - x_hat| repeats there.
Continuous data ties rarely; quantised data (many equal magnitudes) can tie by the thousand and
needs a larger ``slot_cap``.  An overflow is reported by ``check()``, never truncated silently.

The encode / fold callables are injectable together so the sharding and exchange logic can be
tested with the CPU gloo backend; the defaults are the HIP codec (no CPU fallback).
"""
import torch

from .gossip import mh_weights
from .gossip_round import PackedRowRound, up4

HEADER = PackedRowRound.HEADER


def slot_capacity(n, k):
    """Entries a node's slot holds by default: ``min(n, k + max(64, k // 8))`` rounded up to 4."""
    return up4(min(int(n), int(k) + max(64, int(k) // 8)))


class ChocoRound(PackedRowRound):
    """Nodes [lo, hi) of a topology on this rank; ``step()`` runs one Choco round of every node.
    ``x`` is a writable view of the owned nodes' models: the caller applies its local training to
    it between rounds."""

    def __init__(self, adj, x_init, alpha, step_size, rank=0, world=1, group=None, device=None,
                 slot_cap=None, encode=None, fold=None, **unknown):
        """adj: adjacency sets (``gossip.read_edges``); x_init: (hi - lo, N) fp32 tensor, this
        rank's nodes' flat models.  ``encode(x, x_hat, k) -> (idx, vals)`` (one node; the threshold
        selection of x - x_hat) and ``fold(x, x_hat, s, (idx, vals), w_self, [(idx, vals, w)],
        step_size)`` (one node, in place) are injectable (CPU tests)."""
        if unknown:
            raise ValueError(f"unknown arguments {sorted(unknown)}: the peer and reduce-scatter "
                             "exchanges, payload compression and _averaging_server are not "
                             "implemented")
        if (encode is None) != (fold is None):
            raise ValueError("encode and fold are injected together")
        super().__init__(adj, x_init, rank, world, group, device)
        m, N = self.m, self.N
        self.alpha, self.step_size = float(alpha), float(step_size)
        self.k = round(self.alpha * N)
        if self.k < 1:
            raise ValueError(f"k = round(alpha N) = {self.k}: the k = 0 branch (no "
                             "sparsification) stays with the per-node plugin")
        if self.k > N:
            raise ValueError("alpha must lie in (0, 1]")
        self._hip = encode is None
        self._encode, self._fold = encode, fold
        self.cap = up4(slot_cap) if slot_cap is not None else slot_capacity(N, self.k)
        f32 = dict(dtype=torch.float32, device=self.device)
        stride = up4(N)  # every row 16-byte aligned
        self._state = torch.zeros(3, max(1, m), stride, **f32)
        self.x = self._state[0, :m, :N]
        self.x_hat = self._state[1, :m, :N]
        self.s = self._state[2, :m, :N]
        self.x.copy_(x_init)
        # a node's packed row: [count (int64), status, 0 | cap idx | cap vals]
        self._alloc_rows(HEADER + 2 * self.cap)
        self.weights = [mh_weights(adj, i) for i in range(self.lo, self.hi)]
        self._enc_tab = self._fold_tab = self._ws = None

    # ---- views of the packed rows ---------------------------------------------------------------
    def _slots(self, row):
        return (row[HEADER:HEADER + self.cap],
                row[HEADER + self.cap:HEADER + 2 * self.cap].view(torch.float32))

    def payload(self, q):
        """``(idx, vals)`` of node q's payload of the last encode (an owned node; any node after
        an all-gather).  Reads the count: blocks."""
        return self._pay(self._row(q))

    def _pay(self, row):
        count = min(self._count_of(row), self.cap)
        idx, vals = self._slots(row)
        return idx[:count], vals[:count]

    # ---- the legs of a round --------------------------------------------------------------------
    def encode(self):
        """Every owned node's sparsified ``x - x_hat`` into its slot, with the row's header."""
        m = self.m
        if not m:
            return
        if self._hip:
            from . import codec
            if self._enc_tab is None:
                self._enc_tab = codec.choco_node_table(self.x, self.x_hat, self.send[:m])
            self._ws = codec.choco_encode_nodes(self._enc_tab, self.N, self.k, self.cap, self._ws)
            return
        for j in range(m):
            idx, vals = self._encode(self.x[j], self.x_hat[j], self.k)
            idx = torch.as_tensor(idx, dtype=torch.int32)
            vals = torch.as_tensor(vals, dtype=torch.float32)
            c = min(idx.numel(), self.cap)
            si, sv = self._slots(self.send[j])
            si[:c], sv[:c] = idx[:c], vals[:c]
            self.send[j, :2] = torch.tensor([idx.numel()], dtype=torch.int64).view(torch.int32)
            self.send[j, 2] = int(idx.numel() > self.cap)

    def _recvs(self):
        """Per owned node: (x, x_hat, s, own row, cap, w_self, [(row, cap, w)]) in fold order."""
        out = []
        for j, (nbrs, w, w_self) in enumerate(self.weights):
            pays = [(self._row(q), self.cap, wq) for q, wq in zip(nbrs, w)]
            out.append((self.x[j], self.x_hat[j], self.s[j], self._row(self.lo + j), self.cap,
                        w_self, pays))
        return out

    def fold(self):
        """Every owned node's ``_averaging`` in place, behind the status words."""
        m = self.m
        if not m:
            return
        if self._hip:
            from . import codec
            if self._fold_tab is None:  # in place: the addresses never change
                self._fold_tab = codec.ChocoTable(self._recvs(), self.device)
            codec.choco_fold_nodes(self._fold_tab, self.N, self.step_size, guard=self.guard)
            return
        if bool(self.guard.any()):
            return
        for x, x_hat, s, own, _, w_self, pays in self._recvs():  # no status word: counts <= cap
            self._fold(x, x_hat, s, self._pay(own), w_self,
                       [self._pay(r) + (w,) for r, _, w in pays], self.step_size)

    def step(self, mark=None):
        """One round: the encode launch set, one all-gather (with a process group), one fold
        launch.  Nothing synchronises with the host; a slot that was too small leaves x, x_hat and
        s as they were before the round and is reported by ``check()``.  ``mark(leg)`` is called
        after each leg is enqueued (tools/bench_choco_round.py records an event)."""
        mark = mark or (lambda leg: None)
        self.encode()
        mark("encode")
        self.exchange()
        mark("exchange")
        self.fold()
        mark("fold")
        self.round += 1

    def check(self):
        """Copies the last round's status words to pinned host memory (blocks) and raises
        RuntimeError naming the nodes whose selection exceeded the slot.  That round folded
        nothing: x, x_hat and s are those of before it, so the caller can rebuild the engine from
        them with a larger ``slot_cap``."""
        self._guard_to_host()
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        nodes = self._bad_nodes()
        if nodes:
            raise RuntimeError(
                f"Choco round {self.round - 1}: nodes {nodes} select more than the slot's "
                f"{self.cap} entries (ties at the threshold); nothing was folded")
