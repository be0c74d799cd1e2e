"""numpy restatement of the reference's full-model rounds — TEST INFRASTRUCTURE ONLY — and the
recorded reference runs (tests/golden/epidemic.json + epidemic_*.npz, make_golden_epidemic.py).

* the fold: ``PlainAverageSharing._averaging`` (sharing/PlainAverageSharing.py:82-114) and
  ``Sharing._averaging`` (sharing/Sharing.py:156-190) on flat models, every product and sum one
  fp32 rounding, in list order, the local term last;
* the EL-Local sampler (node/EpidemicLearning/EL_Local.py:50-51, :85-86) around ``Random``;
* ``NumpyRound``: a whole-topology engine written node by node, the yardstick of the engines in
  decentralizepy_amd/gossip_epidemic.py where no fixture exists (other graphs, other sizes).
"""
import hashlib
import json
import os
from random import Random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32 = np.float32


def fold(local, rows, weights, w_self):
    """t = fl(v_0 w_0); t = fl(t + fl(v_i w_i)); fl(t + fl(local w_self)).  An empty list: the
    model stays (EL_Local.py:162-165)."""
    local = np.asarray(local, dtype=f32)
    if not len(rows):
        return local.copy()
    total = None
    for v, w in zip(rows, weights):
        term = np.asarray(v, dtype=f32) * f32(w)
        total = term if total is None else total + term
    return total + local * f32(w_self)


def recipe(seed, n, scale=1.0):
    """A node's initial model: a recorded generator recipe (the fixtures store no inputs)."""
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(f32)


def initial_models(meta):
    return np.stack([recipe(meta["x_seed"] + u, meta["n"]) for u in range(meta["nodes"])])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def read_edges(path):
    """As ``decentralizepy_amd.gossip.read_edges`` (the same sets in the same insertion order)."""
    from decentralizepy_amd.gossip import read_edges as rd
    return rd(path)


class Sampler:
    """EL-Local's send sets: node u's ``Random`` seeded ``random_seed + u``, one
    ``sample(neighbours, degree)`` per round."""

    def __init__(self, adj, degree, random_seed):
        self.adj, self.degree = adj, degree
        self.rng = []
        for u in range(len(adj)):
            r = Random()
            r.seed(random_seed + u)
            self.rng.append(r)

    def __call__(self, t=None):
        return [set(self.rng[u].sample(tuple(self.adj[u]), self.degree))
                for u in range(len(self.adj))]


def receive_lists(adj, sets):
    """Per node: the senders it folds, in the iteration order of its neighbour set."""
    return [[j for j in adj[i] if i in sets[j]] for i in range(len(adj))]


def mh_lists(adj):
    """Per node (senders, weights, w_self) of ``Sharing._averaging``: every neighbour sends."""
    out = []
    for i in range(len(adj)):
        nbrs = list(adj[i])
        w = [1 / (max(len(nbrs), len(adj[j])) + 1) for j in nbrs]
        total = 0
        for v in w:
            total += v
        out.append((nbrs, w, 1 - total))
    return out


class NumpyRound:
    """Every node of a topology, one synchronous round per ``step()``, node by node."""

    def __init__(self, adj, x, degree=None, random_seed=None, senders=None):
        self.adj, self.x = adj, np.array(x, dtype=f32)
        self.full = degree is None and senders is None
        if not self.full:
            self.senders = senders or Sampler(adj, degree, random_seed)
        self.received_this_round = [0] * len(adj)
        self.send_sets = None
        self.round = 0

    def step(self):
        if self.full:
            lists = mh_lists(self.adj)
        else:
            self.send_sets = [set(s) for s in self.senders(self.round)]
            lists = []
            for i, got in enumerate(receive_lists(self.adj, self.send_sets)):
                w = 1 / (len(got) + 1)
                lists.append((got, [w] * len(got), w))
                if got:  # set by the averaging only (PlainAverageSharing.py:87)
                    self.received_this_round[i] = len(got)
        self.x = np.stack([fold(self.x[i], [self.x[j] for j in s], w, ws)
                           for i, (s, w, ws) in enumerate(lists)])
        self.round += 1


# ---- the recorded reference runs ----------------------------------------------------------------
def runs():
    with open(os.path.join(GOLDEN, "epidemic.json")) as f:
        return json.load(f)["runs"]


def load(name):
    """(meta, last): a run's record and the full models after its last round."""
    meta = next(r for r in runs() if r["name"] == name)
    last = np.load(os.path.join(GOLDEN, f"epidemic_{name}.npz"))["last"]
    return meta, last


def graph(meta):
    if "edges_file" in meta:
        return read_edges(os.path.join(GOLDEN, meta["edges_file"]))
    adj = [set() for _ in range(meta["nodes"])]
    for a, b in meta["edges"]:
        adj[a].add(b)
        adj[b].add(a)
    return adj


def check_round(meta, last, r, models, lo=0, received=None, send_sets=None):
    """Rows [lo, lo + len(models)) after round r against the record."""
    mr = meta["rounds"][r]
    models = np.ascontiguousarray(models)
    assert models.dtype == f32 and models.shape[1] == meta["n"]
    for j, row in enumerate(models):
        assert sha(row) == mr["model_sha"][lo + j], (meta["name"], r, lo + j)
    if r == len(meta["rounds"]) - 1:
        np.testing.assert_array_equal(models.view(np.uint32),
                                      last[lo:lo + len(models)].view(np.uint32))
    if received is not None:
        assert list(received) == mr["received_this_round"]
    if send_sets is not None:
        assert [sorted(s) for s in send_sets] == mr["send_sets"]
