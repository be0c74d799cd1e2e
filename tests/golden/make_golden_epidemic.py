#!/usr/bin/env python3
"""Generate the full-model round fixtures (tests/golden/epidemic.json + epidemic_*.npz) from the
UNMODIFIED reference (sacs-epfl/decentralizepy): ``sharing/PlainAverageSharing.py``,
``sharing/Sharing.py`` and ``graphs/Graph.py``.  Run in the build container only (the reference
is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_epidemic.py

Epidemic Learning (``el_d7``, ``el_d1``, ``el_d15``): one reference ``PlainAverageSharing``
object per uid over ``fullyConnected_16.edges`` (the tutorial's graph, copied next to this file as
data and read by the reference's ``Graph``), ``random_seed = 90`` as in
``tutorial/EpidemicLearning/config_EL.ini``, three rounds at degree 7 (the tutorial's), 1 and 15.
The nodes are driven by the loop of ``node/EpidemicLearning/EL_Local.py`` restated around
``Random`` (:85-86 the seeding, :50-51 the sample, :143-165 who is averaged, in the iteration
order of the neighbour set; a node that received nothing only advances its round).  No training
happens between the rounds.

Full share (``fullshare6``): reference ``Sharing`` nodes over the 6-node graph of
tests/test_cpu_subsampling_round.py for two rounds, driven as ``node/DPSGDNode.py:90-115`` does.

Every node is a multi-tensor model of n = 1,031 parameters from a recorded recipe
(tests/epidemic_ops.py:recipe).  Recorded per round: the send sets, ``received_this_round`` of
every node's sharing object and SHA-256 of every node's flat model; the npz holds the models after
the last round.
"""
import json
import os
import sys
import tempfile
from collections import deque
from random import Random

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference/src"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
import torch  # noqa: E402

from decentralizepy.mappings.Linear import Linear  # noqa: E402
from decentralizepy.models.Model import Model  # noqa: E402
from decentralizepy.sharing.PlainAverageSharing import PlainAverageSharing  # noqa: E402
from decentralizepy.sharing.Sharing import Sharing  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import epidemic_ops as ops  # noqa: E402  (recipe and sha only)
from tests.test_cpu_subsampling_round import EDGES6  # noqa: E402


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
SHAPE = [30, 33, 37, 4]  # n = 1,031
RANDOM_SEED = 90
EDGES_FILE = "fullyConnected_16.edges"


class Net(Model):
    def __init__(self, rows, cols, nb, ne):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(rows, cols))
        self.bias = torch.nn.Parameter(torch.zeros(nb))
        self.scale = torch.nn.Parameter(torch.zeros(ne))


def set_flat(model, flat):
    new, pos = {}, 0
    for key, v in model.state_dict().items():
        new[key] = torch.from_numpy(flat[pos:pos + v.numel()].reshape(v.shape).copy())
        pos += v.numel()
    model.load_state_dict(new)


def get_flat(model):
    return torch.cat([v.flatten() for v in model.state_dict().values()]).numpy().copy()


def make_nodes(cls, graph, meta):
    n_nodes = graph.n_procs
    mapping = Linear(1, n_nodes)
    nodes = []
    with tempfile.TemporaryDirectory() as tmp:
        for u in range(n_nodes):
            model = Net(*SHAPE)
            set_flat(model, ops.recipe(meta["x_seed"] + u, meta["n"]))
            nodes.append(cls(u, 0, None, mapping, graph, model, None, tmp))
    return nodes


def record(meta, nodes, extra):
    flats = np.stack([get_flat(s.model) for s in nodes])
    meta["rounds"].append(dict(extra, model_sha=[ops.sha(row) for row in flats]))
    return flats


def sample(rng, neighbours, degree):
    """``set(self.rng.sample(self.my_neighbors, self.degree))`` (EL_Local.py:51).  The set form is
    what the reference calls; Python 3.11 refuses it, so check once that the tuple form, which
    the engine uses, draws the same."""
    state = rng.getstate()
    drawn = rng.sample(tuple(neighbours), degree)
    if sys.version_info < (3, 11):
        other = Random()
        other.setstate(state)
        assert other.sample(neighbours, degree) == drawn
    return set(drawn)


def run_el(degree, rounds=3):
    graph = Graph()
    graph.read_graph_from_file(os.path.join(OUT, EDGES_FILE), "edges")
    n_nodes = graph.n_procs
    n = SHAPE[0] * SHAPE[1] + SHAPE[2] + SHAPE[3]
    meta = dict(name=f"el_d{degree}", kind="el", nodes=n_nodes, n=n, shape=SHAPE, degree=degree,
                random_seed=RANDOM_SEED, edges_file=EDGES_FILE, x_seed=1000, rounds=[])
    nodes = make_nodes(PlainAverageSharing, graph, meta)
    rngs = []
    for u in range(n_nodes):  # EL_Local.py:85-86
        rng = Random()
        rng.seed(RANDOM_SEED + u)
        rngs.append(rng)
    flats = None
    for it in range(rounds):
        sends = [sample(rngs[u], graph.neighbors(u), degree) for u in range(n_nodes)]
        msgs = []
        for u, s in enumerate(nodes):
            m = s.get_data_to_send()
            assert m["iteration"] == it
            m["params"] = np.array(m["params"], dtype=np.float32, copy=True)
            m["CHANNEL"] = "DPSGD"
            msgs.append(m)
        for u, s in enumerate(nodes):
            averaging_deque = dict()
            for x in graph.neighbors(u):  # EL_Local.py:145-153: "NotWorking" senders drop out
                if u in sends[x]:
                    averaging_deque[x] = deque([dict(msgs[x])])
            if averaging_deque:
                s._averaging(averaging_deque)
            else:
                s.communication_round += 1
            assert s.communication_round == it + 1
        flats = record(meta, nodes, dict(
            send_sets=[sorted(s) for s in sends],
            received_this_round=[int(s.received_this_round) for s in nodes]))
    return meta, flats


def run_fullshare(rounds=2):
    graph = Graph(6)
    for a, b in EDGES6:  # as tests/test_cpu_subsampling_round.py:adjacency fills its sets
        graph.adj_list[a].add(b)
        graph.adj_list[b].add(a)
    n = SHAPE[0] * SHAPE[1] + SHAPE[2] + SHAPE[3]
    meta = dict(name="fullshare6", kind="fullshare", nodes=6, n=n, shape=SHAPE,
                edges=[list(e) for e in EDGES6], x_seed=2000, rounds=[])
    nodes = make_nodes(Sharing, graph, meta)
    flats = None
    for it in range(rounds):
        msgs = []
        for u, s in enumerate(nodes):  # DPSGDNode.py:90
            m = s.get_data_to_send(degree=len(graph.neighbors(u)))
            m["params"] = np.array(m["params"], dtype=np.float32, copy=True)
            m["CHANNEL"] = "DPSGD"
            msgs.append(m)
        for u, s in enumerate(nodes):  # DPSGDNode.py:111-115
            s._averaging({x: deque([dict(msgs[x])]) for x in graph.neighbors(u)})
            assert s.communication_round == it + 1
        flats = record(meta, nodes, {})
    return meta, flats


def main():
    metas = []
    for degree in (7, 1, 15):
        meta, flats = run_el(degree)
        first = [len([1 for s in meta["rounds"][0]["send_sets"] if i in s])
                 for i in range(meta["nodes"])]
        # the fixture must keep covering the uneven lists, the empty list and the full list
        if degree == 7:
            assert (min(first), max(first)) == (2, 11), first
        if degree == 1:
            assert [i for i, c in enumerate(first) if c == 0] == [1, 8, 10, 12], first
            assert meta["rounds"][0]["received_this_round"][1] == 0
        if degree == 15:
            assert all(r["received_this_round"] == [15] * 16 for r in meta["rounds"])
        metas.append((meta, flats))
    metas.append(run_fullshare())
    total = 0
    for meta, flats in metas:
        path = os.path.join(OUT, f"epidemic_{meta['name']}.npz")
        np.savez_compressed(path, last=flats)
        total += os.path.getsize(path)
        print(meta["name"], os.path.getsize(path), "bytes", flush=True)
    with open(os.path.join(OUT, "epidemic.json"), "w") as f:
        json.dump({"numpy": np.__version__, "runs": [m for m, _ in metas]}, f, indent=1)
    total += os.path.getsize(os.path.join(OUT, "epidemic.json"))
    print("total", total, "bytes")
    assert total < 300_000


if __name__ == "__main__":
    main()
