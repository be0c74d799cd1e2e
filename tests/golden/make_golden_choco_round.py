#!/usr/bin/env python3
"""Generate the whole-topology Choco fixtures (tests/golden/choco_round.json + choco_round_*.npz)
from the UNMODIFIED reference ``decentralizepy.sharing.Choco`` and ``graphs/Graph.py``
(sacs-epfl/decentralizepy).  Run in the build container only (the reference is not on the GPU
box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_choco_round.py

One reference ``Choco`` object per node of a topology, with the real neighbour sets.  Three rounds:
every node "trains" (a seeded perturbation, tests/choco_round_ops.py:train), then
``get_data_to_send(degree=len(neighbours))``, then ``_averaging`` over its neighbours' actual
messages in ``graph.neighbors(u)`` order, as ``node/DPSGDNode.py:90-115`` drives a node.

Runs: ``regular16`` (regular_16.edges, alpha 0.05, N = 2,051) and ``irr6`` (a 6-node graph with
degrees 1 to 4, alpha 0.1, N = 4,100, round 0 quantised to steps of 0.05 with every 5th element
zero: ties at the threshold and exact zeros; the slot the engine needs for it is recorded).
Recorded: the initial models, per round every node's payload count and model, after the last round
x_hat and s.  Plain numpy arrays (allow_pickle=False).
"""
import json
import os
import sys
import tempfile
from collections import deque

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference/src"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
import torch  # noqa: E402

from decentralizepy.mappings.Linear import Linear  # noqa: E402
from decentralizepy.models.Model import Model  # noqa: E402
from decentralizepy.sharing.Choco import Choco  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import choco_round_ops as ops  # noqa: E402  (recipes and the graph's edges only)


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
ROUNDS = 3


class Net(Model):
    def __init__(self, rows, cols, nb):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(rows, cols))
        self.bias = torch.nn.Parameter(torch.zeros(nb))


def set_flat(model, flat):
    new, pos = {}, 0
    for key, v in model.state_dict().items():
        new[key] = torch.from_numpy(flat[pos:pos + v.numel()].reshape(v.shape).copy())
        pos += v.numel()
    model.load_state_dict(new)


def flat_of(state):
    return torch.cat([v.flatten() for v in state.values()]).numpy().copy()


def run(meta, graph, shape):
    n_nodes = graph.n_procs
    n = shape[0] * shape[1] + shape[2]
    meta.update(nodes=n_nodes, n=n, shape=list(shape), rounds=ROUNDS)
    rng = np.random.default_rng(meta["seed"])
    x0 = rng.standard_normal((n_nodes, n)).astype(np.float32)
    mapping = Linear(1, n_nodes)
    nodes = []
    with tempfile.TemporaryDirectory() as tmp:
        for u in range(n_nodes):
            model = Net(*shape)
            set_flat(model, x0[u])
            nodes.append(Choco(u, 0, None, mapping, graph, model, None, tmp,
                               step_size=meta["step_size"], alpha=meta["alpha"]))
    arrays = {"x0": x0}
    counts = []
    for r in range(ROUNDS):
        msgs = []
        for u, s in enumerate(nodes):
            set_flat(s.model, ops.train(flat_of(s.model.state_dict()), meta, r, u))
            m = s.get_data_to_send(degree=len(graph.neighbors(u)))
            assert m["iteration"] == r
            m["params"] = np.array(m["params"], dtype=np.float32, copy=True)
            m["indices"] = np.array(m["indices"], copy=True)
            m["CHANNEL"] = "DPSGD"
            msgs.append(m)
        counts.append([len(m["indices"]) for m in msgs])
        for u, s in enumerate(nodes):
            s._averaging({v: deque([dict(msgs[v])]) for v in graph.neighbors(u)})
            assert s.communication_round == r + 1
        arrays[f"x_r{r}"] = np.stack([flat_of(s.model.state_dict()) for s in nodes])
    arrays["counts"] = np.array(counts, dtype=np.int64)
    arrays["x_hat"] = np.stack([flat_of(s.model_hat) for s in nodes])
    arrays["s"] = np.stack([flat_of(s.s) for s in nodes])
    k = round(meta["alpha"] * n)
    meta["k"] = k
    meta["max_count"] = int(arrays["counts"].max())
    # the tie run gets exactly the slot its largest payload needs; the other the engine's default
    meta["slot_cap"] = -(-meta["max_count"] // 4) * 4 if meta["quantised"] else None
    return arrays


def main():
    metas = []
    g16 = Graph()
    g16.read_graph_from_file(os.path.join(OUT, "regular_16.edges"), "edges")
    m16 = dict(name="regular16", edges_file="regular_16.edges", alpha=0.05, step_size=0.5,
               seed=31, quantised=False)
    metas.append((m16, run(m16, g16, (40, 50, 51))))  # N = 2,051
    g6 = Graph(6)
    for a, b in ops.EDGES_IRR6:  # as tests/choco_round_ops.py:adjacency fills its sets
        g6.adj_list[a].add(b)
        g6.adj_list[b].add(a)
    assert sorted(len(g6.neighbors(u)) for u in range(6)) == [1, 1, 2, 3, 3, 4]
    m6 = dict(name="irr6", edges=[list(e) for e in ops.EDGES_IRR6], alpha=0.1, step_size=0.3,
              seed=32, quantised=True)
    metas.append((m6, run(m6, g6, (50, 81, 50))))  # N = 4,100
    assert m6["max_count"] > m6["k"]  # the ties are there
    for meta, arrays in metas:
        path = os.path.join(OUT, f"choco_round_{meta['name']}.npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(meta["name"], meta["n"], meta["k"], meta["max_count"], meta["slot_cap"], size,
              "bytes", flush=True)
        assert size < 1_000_000
    with open(os.path.join(OUT, "choco_round.json"), "w") as f:
        json.dump({"numpy": np.__version__, "runs": [m for m, _ in metas]}, f, indent=1)


if __name__ == "__main__":
    main()
