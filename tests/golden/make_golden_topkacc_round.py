#!/usr/bin/env python3
"""Generate the whole-topology fixtures of top-k sharing with accumulated changes
(tests/golden/topkacc_round.json + topkacc_round_*.npz) from the UNMODIFIED reference
``decentralizepy.sharing.PartialModel`` and ``graphs/Graph.py`` (sacs-epfl/decentralizepy).  Run in
the build container only (the reference is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_topkacc_round.py

One reference ``PartialModel`` object per node of a topology, with the real neighbour sets,
``accumulation=True``, ``compress=False`` and ``accumulate_averaging_changes`` False (runs
``acc_*``) or True (runs ``avg_*``).  Per round every node "trains" (a seeded perturbation,
tests/topkacc_round_ops.py:train), then ``get_data_to_send(degree=len(neighbours))``, then
``_averaging`` over its neighbours' actual messages in ``graph.neighbors(u)`` order, as
``node/DPSGDNode.py:90-115`` drives a node.

Runs: ``*_reg16`` (regular_16.edges, alpha 0.05, N = 2,051, 3 rounds) and ``*_irr6`` (a 6-node
graph with degrees 1 to 4, alpha 0.1, N = 4,100, 4 rounds).  Recorded: the initial models, per
round every node's indices, params and model, after the last round every ``accumulated_changes``
and ``shared_parameters_counter``.  Plain numpy arrays (allow_pickle=False).  torch.topk's CPU tie
order is implementation-defined: a seed at which any selection ties at its k-th key, or at which a
recorded float array holds -0.0, is skipped, and the seed used is recorded.
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
from decentralizepy.sharing.PartialModel import PartialModel  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import topkacc_round_ops as ops  # noqa: E402  (recipes and the graph's edges only)


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


def flat_of(model):
    return torch.cat([v.flatten() for v in model.state_dict().values()]).numpy().copy()


def run(meta, graph, shape, seed):
    n_nodes = graph.n_procs
    n = shape[0] * shape[1] + shape[2]
    k = round(meta["alpha"] * n)
    meta.update(nodes=n_nodes, n=n, k=k, shape=list(shape), seed=seed)
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((n_nodes, n)).astype(np.float32)
    mapping = Linear(1, n_nodes)
    nodes = []
    with tempfile.TemporaryDirectory() as tmp:
        for u in range(n_nodes):
            model = Net(*shape)
            set_flat(model, x0[u])
            nodes.append(PartialModel(u, 0, None, mapping, graph, model, None, tmp,
                                      alpha=meta["alpha"], accumulation=True,
                                      accumulate_averaging_changes=meta["avg"], compress=False))
    arrays = {"x0": x0}
    for r in range(meta["rounds"]):
        msgs = []
        for u, s in enumerate(nodes):
            set_flat(s.model, ops.train(flat_of(s.model), meta, r, u))
            m = s.get_data_to_send(degree=len(graph.neighbors(u)))
            assert m["iteration"] == r and m["send_partial"] and len(m["indices"]) == k
            if ops.kth_has_tie(s.model.model_change.numpy(), k):
                raise Retry(f"tie: node {u} round {r}")
            m["params"] = np.array(m["params"], dtype=np.float32, copy=True)
            m["indices"] = np.array(m["indices"], dtype=np.int32, copy=True)
            m["CHANNEL"] = "DPSGD"
            msgs.append(m)
        for u, s in enumerate(nodes):
            s._averaging({v: deque([dict(msgs[v])]) for v in graph.neighbors(u)})
            assert s.communication_round == r + 1
        arrays[f"r{r}_idx"] = np.stack([m["indices"] for m in msgs])
        arrays[f"r{r}_vals"] = np.stack([m["params"] for m in msgs])
        arrays[f"r{r}_x"] = np.stack([flat_of(s.model) for s in nodes])
    arrays["acc"] = np.stack([s.model.accumulated_changes.numpy().copy() for s in nodes])
    arrays["counter"] = np.stack([s.model.shared_parameters_counter.numpy().copy()
                                  for s in nodes]).astype(np.int32)
    for name, a in arrays.items():
        if a.dtype == np.float32 and np.signbit(a[a == 0]).any():
            raise Retry(f"-0.0 in {name}")
    return arrays


def main():
    g16 = Graph()
    g16.read_graph_from_file(os.path.join(OUT, "regular_16.edges"), "edges")
    g6 = Graph(6)
    for a, b in ops.EDGES_IRR6:  # as tests/choco_round_ops.py:adjacency fills its sets
        g6.adj_list[a].add(b)
        g6.adj_list[b].add(a)
    assert sorted(len(g6.neighbors(u)) for u in range(6)) == [1, 1, 2, 3, 3, 4]
    metas = []
    for avg in (False, True):
        mode = "avg" if avg else "acc"
        specs = [
            (dict(name=f"{mode}_irr6", edges=[list(e) for e in ops.EDGES_IRR6], alpha=0.1,
                  avg=avg, rounds=4), g6, (50, 81, 50), 52),  # N = 4,100
            (dict(name=f"{mode}_reg16", edges_file="regular_16.edges", alpha=0.05, avg=avg,
                  rounds=3), g16, (40, 50, 51), 51),  # N = 2,051
        ]
        for meta, graph, shape, seed0 in specs:
            for seed in range(seed0, seed0 + 400, 10):
                try:
                    arrays = run(meta, graph, shape, seed)
                    break
                except Retry as e:
                    print("retry:", meta["name"], seed, e, flush=True)
            else:
                raise SystemExit("no tie-free seed")
            path = os.path.join(OUT, f"topkacc_round_{meta['name']}.npz")
            np.savez_compressed(path, **arrays)
            size = os.path.getsize(path)
            print(meta["name"], meta["n"], meta["k"], meta["seed"], size, "bytes", flush=True)
            assert size < 1_000_000
            metas.append(meta)
    with open(os.path.join(OUT, "topkacc_round.json"), "w") as f:
        json.dump({"numpy": np.__version__, "runs": metas}, f, indent=1)


if __name__ == "__main__":
    main()
