"""numpy restatement of a Choco round in its dense reference form (reference sharing/Choco.py:
186-207 the threshold sparsification, :359-453 the round), one fp32 rounding per operation, plus
the recipes the recorded runs (tests/golden/make_golden_choco_round.py) are rebuilt from."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# 6 nodes with degrees 4 3 2 3 1 1
EDGES_IRR6 = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (3, 5)]


def adjacency(n, edges):
    """Adjacency sets filled like ``gossip.read_edges`` fills them (same insertion order)."""
    adj = [set() for _ in range(n)]
    for a, b in edges:
        adj[a].add(b)
        adj[b].add(a)
    return adj


def perturbation(seed, r, u, n):
    """The "training" of node u before round r: a fixed seeded step, added in fp32."""
    rng = np.random.default_rng([seed, r, u])
    return (0.01 * rng.standard_normal(n)).astype(np.float32)


def quantise(x):
    """Steps of 0.05 with every 5th element zero: ties at the threshold and exact zeros."""
    q = (np.round(x * np.float32(20)) / np.float32(20)).astype(np.float32)
    q[::5] = 0.0
    return q


def train(x, meta, r, u):
    """Node u's model before round r's exchange, from its model after round r - 1."""
    x = (x + perturbation(meta["seed"], r, u, x.size)).astype(np.float32)
    if meta["quantised"] and r == 0:
        x = quantise(x)
    return x


def select(x, x_hat, k):
    """``nonzero(topk_sparsification(x - x_hat))``: T = the k-th largest |d|, every |d| >= T that
    is not zero, ascending.  Returns (idx int32, vals fp32)."""
    d = x.astype(np.float32) - x_hat.astype(np.float32)
    a = np.abs(d)
    T = np.partition(a, d.size - k)[d.size - k]
    idx = np.flatnonzero((a >= T) & (d != 0)).astype(np.int32)
    return idx, d[idx]


def dense(idx, vals, n):
    t = np.zeros(n, np.float32)
    t[idx] = vals
    return t


def fold(x, x_hat, s, q_self, w_self, pays, step_size):
    """``_averaging`` written densely, in place on the fp32 arrays x, x_hat, s.  pays: (idx, vals,
    w) in fold order; weights and step_size are rounded to fp32 as torch rounds a scalar."""
    n = x.size
    q = dense(q_self[0], q_self[1], n)
    x_hat[:] = x_hat + q
    for idx, vals, w in pays:
        s[:] = s + dense(idx, vals, n) * np.float32(w)
    s[:] = s + q * np.float32(w_self)
    x[:] = x + np.float32(step_size) * (s - x_hat)


def mh(adj, i):
    """gossip.mh_weights restated: neighbours in set order, Python-double weights."""
    nbrs = list(adj[i])
    w = [1 / (max(len(nbrs), len(adj[j])) + 1) for j in nbrs]
    total = 0
    for v in w:
        total += v
    return nbrs, w, 1 - total


def load_runs():
    """[(meta, arrays)] of the recorded reference runs."""
    with open(os.path.join(GOLDEN, "choco_round.json")) as f:
        metas = json.load(f)["runs"]
    return [(m, dict(np.load(os.path.join(GOLDEN, f"choco_round_{m['name']}.npz"),
                             allow_pickle=False))) for m in metas]


def run_adjacency(meta):
    if "edges_file" in meta:
        from decentralizepy_amd.gossip import read_edges
        return read_edges(os.path.join(GOLDEN, meta["edges_file"]))
    return adjacency(meta["nodes"], [tuple(e) for e in meta["edges"]])


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_recorded(meta, arr, r, x, counts, x_hat=None, s=None, lo=0):
    """Rows [lo, lo + len(x)) after round r against the recording, bit for bit."""
    m = len(x)
    np.testing.assert_array_equal(u32(x), u32(arr[f"x_r{r}"][lo:lo + m]), err_msg=f"x r{r}")
    if counts is not None:
        assert list(counts) == arr["counts"][r].tolist(), (r, counts)
    if r == meta["rounds"] - 1 and x_hat is not None:
        np.testing.assert_array_equal(u32(x_hat), u32(arr["x_hat"][lo:lo + m]), err_msg="x_hat")
        np.testing.assert_array_equal(u32(s), u32(arr["s"][lo:lo + m]), err_msg="s")
