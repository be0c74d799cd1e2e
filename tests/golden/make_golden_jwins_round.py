#!/usr/bin/env python3
"""Generate the whole-topology JWINS fixtures (tests/golden/jwins_round.json +
jwins_round_{reg16,irr6}.npz) from the UNMODIFIED reference ``decentralizepy.sharing.JWINS.JWINS``
and ``graphs/Graph.py`` (sacs-epfl/decentralizepy).  Run in the build container only (the
reference is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_jwins_round.py

One reference ``JWINS`` object per node of a topology, with the real neighbour sets, the
tutorial's ``alpha_list``, sym2 at level 4, ``metadata_cap = 0.5``, ``accumulation = True``,
``accumulate_averaging_changes = True`` and ``compress = False`` (fpzip is not in the container;
the wire codec is lossless).  PyWavelets 1.1.1 is reached through make_golden.py's bridge to
python3.9.  Per round every node "trains" (a seeded perturbation, tests/jwins_round_ops.py:train),
then ``get_data_to_send``, then ``_averaging`` over its neighbours' actual messages in
``graph.neighbors(u)`` order, as ``node/DPSGDNode.py:90-115`` drives a node.

The reference seeds and draws from the GLOBAL ``random`` module (``JWINS.py:89,96``), one process
per node.  Here all nodes share a process, so one ``random.getstate()`` per node is kept: saved
after the node's construction (which seeds it) and restored around each ``get_data_to_send``.
The classes themselves stay untouched.

Runs: ``reg16`` (regular_16.edges, N = 1,030, 3 rounds) and ``irr6`` (the 6-node graph with degrees
1 to 4, N = 4,100, 4 rounds).  Recorded: the initial models, per round every node's alpha, its
partial payload (indices, params; a full share is not stored) and its model, after the last round
every ``accumulated_changes`` and ``shared_parameters_counter``.  Plain numpy arrays
(allow_pickle=False).  torch.topk's CPU tie order is implementation-defined: a seed at which any
selection ties at its k-th key, or at which a recorded float array holds -0.0, is skipped, and the
seed used is recorded.
"""
import json
import os
import random
import sys
import tempfile
from collections import deque

import numpy as np

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as mg  # noqa: E402  (installs the pywt bridge, imports the reference classes)

sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from oracle import topk as otopk  # noqa: E402
from tests import jwins_round_ops as ops  # noqa: E402  (recipes and the graph's edges only)

REF = mg.REF
JWINS, Linear, Net = mg.JWINS, mg.Linear, mg.Net
ALPHAS = ops.TUTORIAL_ALPHAS
ALPHA_LIST = "[0.1,0.15,0.2,0.25,0.3,0.4,1.0]"
CAP, LEVEL = 0.5, 4
assert eval(ALPHA_LIST) == ALPHAS


def _load_graph_class():
    """graphs/Graph.py by its path: the package's __init__ also imports SmallWorld, whose
    ``smallworld`` dependency the build container lacks."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "_reference_graph", os.path.join(REF, "decentralizepy", "graphs", "Graph.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Graph


Graph = _load_graph_class()


class Retry(RuntimeError):
    pass


def expected_draws(n_nodes, rounds):
    rngs = [random.Random(u) for u in range(n_nodes)]
    return [[rngs[u].choice(ALPHAS) for u in range(n_nodes)] for _ in range(rounds)]


def run(meta, graph, shape, seed):
    n_nodes = graph.n_procs
    n = shape[0] * shape[1] + shape[2]
    meta.update(nodes=n_nodes, n=n, shape=list(shape), seed=seed, alpha_list=ALPHAS,
                metadata_cap=CAP, wavelet="sym2", level=LEVEL)
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((n_nodes, n)).astype(np.float32)
    mapping = Linear(1, n_nodes)
    nodes, states = [], []
    with tempfile.TemporaryDirectory() as tmp:
        for u in range(n_nodes):
            model = Net(*shape)
            mg.set_flat(model, x0[u])
            nodes.append(JWINS(u, 0, None, mapping, graph, model, None, tmp,
                               alpha_list=ALPHA_LIST, metadata_cap=CAP, wavelet="sym2",
                               level=LEVEL, accumulation=True, accumulate_averaging_changes=True,
                               compress=False))  # JWINS.py:89 seeded the global generator
            states.append(random.getstate())
    m_len = int(nodes[0].wt_shape[0])
    meta["m_len"] = m_len
    draws = expected_draws(n_nodes, meta["rounds"])
    arrays = {"x0": x0}
    for r in range(meta["rounds"]):
        msgs = []
        for u, s in enumerate(nodes):
            mg.set_flat(s.model, ops.train(mg.get_flat(s.model), meta, r, u))
            random.setstate(states[u])
            m = s.get_data_to_send(degree=len(graph.neighbors(u)))
            states[u] = random.getstate()
            assert m["iteration"] == r and m["degree"] == len(graph.neighbors(u))
            assert s.alpha == draws[r][u]  # the uid-seeded draws every rank replays
            if "send_partial" in m:
                k = round(s.alpha * m_len)
                assert s.alpha < CAP and len(m["indices"]) == k >= 1
                if otopk.kth_has_tie(otopk.keys_u32(s.model.model_change.numpy()), k):
                    raise Retry(f"tie: node {u} round {r}")
                arrays[f"r{r}_n{u}_idx"] = np.array(m["indices"], dtype=np.int32, copy=True)
                arrays[f"r{r}_n{u}_vals"] = np.array(m["params"], dtype=np.float32, copy=True)
            else:
                assert s.alpha >= CAP and len(m["params"]) == m_len
            m["params"] = np.array(m["params"], dtype=np.float32, copy=True)
            m["CHANNEL"] = "DPSGD"
            msgs.append(m)
        for u, s in enumerate(nodes):
            s._averaging({v: deque([dict(msgs[v])]) for v in graph.neighbors(u)})
            assert s.communication_round == r + 1
        arrays[f"r{r}_alpha"] = np.array(draws[r], dtype=np.float64)
        arrays[f"r{r}_x"] = np.stack([mg.get_flat(s.model) for s in nodes])
    arrays["acc"] = np.stack([s.model.accumulated_changes.numpy().copy() for s in nodes])
    arrays["counter"] = np.stack([s.model.shared_parameters_counter.numpy().copy()
                                  for s in nodes]).astype(np.int32)
    for name, a in arrays.items():
        if a.dtype == np.float32 and np.signbit(a[a == 0]).any():
            raise Retry(f"-0.0 in {name}")
    # every round of the run holds a full share beside partial ones
    meta["full_shares"] = [[u for u in range(n_nodes) if draws[r][u] >= CAP]
                           for r in range(meta["rounds"])]
    assert all(meta["full_shares"])
    assert len({a for row in draws for a in row if a < CAP}) >= 4
    return arrays


def main():
    mg.torch.set_num_threads(4)
    g16 = Graph()
    g16.read_graph_from_file(os.path.join(OUT, "regular_16.edges"), "edges")
    g6 = Graph(6)
    for a, b in ops.EDGES_IRR6:  # as tests/choco_round_ops.py:adjacency fills its sets
        g6.adj_list[a].add(b)
        g6.adj_list[b].add(a)
    assert sorted(len(g6.neighbors(u)) for u in range(6)) == [1, 1, 2, 3, 3, 4]
    specs = [
        (dict(name="irr6", edges=[list(e) for e in ops.EDGES_IRR6], rounds=4), g6,
         (50, 81, 50), 61),  # N = 4,100: two forward tiles, just past one inverse tile
        (dict(name="reg16", edges_file="regular_16.edges", rounds=3), g16, (30, 33, 40), 62),
    ]
    metas = []
    for meta, graph, shape, seed0 in specs:
        for seed in range(seed0, seed0 + 400, 10):
            try:
                arrays = run(meta, graph, shape, seed)
                break
            except Retry as e:
                print("retry:", meta["name"], seed, e, flush=True)
        else:
            raise SystemExit("no tie-free seed")
        if meta["name"] == "irr6":
            assert meta["full_shares"] == [[0, 2], [2], [0, 1], [1]]
        path = os.path.join(OUT, f"jwins_round_{meta['name']}.npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(meta["name"], meta["n"], meta["m_len"], meta["seed"], size, "bytes", flush=True)
        assert size < 1_000_000
        metas.append(meta)
    with open(os.path.join(OUT, "jwins_round.json"), "w") as f:
        json.dump({"numpy": np.__version__, "torch": mg.torch.__version__,
                   "pywavelets": "1.1.1 (python3.9 bridge)",
                   "reference": "sacs-epfl/decentralizepy v1", "runs": metas}, f, indent=1)


if __name__ == "__main__":
    main()
