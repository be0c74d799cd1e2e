#!/usr/bin/env python3
"""Generate the quantised full-model round fixtures (tests/golden/quant_round.json +
quant_round_*.npz) from the UNMODIFIED reference (sacs-epfl/decentralizepy):
``sharing/Sharing.py`` and ``sharing/PlainAverageSharing.py`` with ``compress = True`` and
``compression/Quantization.py``, ``graphs/Graph.py``.  Run in the build container only (the
reference is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_quant_round.py

One reference sharing object per node, driven as make_golden_epidemic.py drives them
(``node/DPSGDNode.py:90-115`` for the full share, the loop of
``node/EpidemicLearning/EL_Local.py`` for EL-Local); no training between the rounds.

* ``fullshare6_q255``: ``Sharing`` + ``Quantization(255)`` over the 6-node irregular graph of
  tests/test_cpu_subsampling_round.py, 2 rounds, n = 2,001 (w = 9; n is no multiple of 4 or 32);
* ``el_d7_q32767`` / ``el_d1_q32767``: ``PlainAverageSharing`` + ``Quantization(32767)`` over
  ``fullyConnected_16.edges``, EL-Local at degree 7 and 1 (some nodes receive nothing), seed 90,
  2 rounds, n = 1,031.

Recorded per round: SHA-256 of every node's flat model (and, for EL, the send sets and
``received_this_round``); every node's round-0 wire as scale bits, w, padding and SHA-256 of the
body; the npz holds the models after the last round and the whole ``to_send`` of nodes 0, 1 and
the last.  The json records the numpy version: the scale depends on numpy's summation order.
"""
import json
import os
import pickle
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
from tests import quantization_ops as qops  # noqa: E402  (bits_of only)
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
RANDOM_SEED = 90
EDGES_FILE = "fullyConnected_16.edges"
ROUNDS = 2
STORED = (0, 1, -1)  # nodes whose whole round-0 to_send is stored


class Net(Model):
    """Two-tensor model: weight (rows, cols) and bias (nb,)."""

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


def get_flat(model):
    return torch.cat([v.flatten() for v in model.state_dict().values()]).numpy().copy()


def make_nodes(cls, graph, meta):
    mapping = Linear(1, graph.n_procs)
    nodes = []
    with tempfile.TemporaryDirectory() as tmp:
        for u in range(graph.n_procs):
            model = Net(*meta["shape"])
            set_flat(model, ops.recipe(meta["x_seed"] + u, meta["n"]))
            nodes.append(cls(u, 0, None, mapping, graph, model, None, tmp, compress=True,
                             compression_package="decentralizepy.compression.Quantization",
                             compression_class="Quantization",
                             float_precision=meta["float_precision"]))
    return nodes


def new_meta(name, kind, nodes, shape, k, x_seed, **extra):
    rows, cols, nb = shape
    return dict(name=name, kind=kind, nodes=nodes, n=rows * cols + nb, shape=shape,
                float_precision=k, x_seed=x_seed, rounds=[], wire=[], **extra)


def record_wire(meta, arrays, msgs):
    """Round 0: what every node put on the wire, params unpickled."""
    for u, m in enumerate(msgs):
        scale, to_send = pickle.loads(m["params"])
        assert isinstance(scale, np.float32) and to_send.dtype == np.uint8
        meta["wire"].append(dict(scale_bits=qops.bits_of(scale), w=int(to_send[1]),
                                 padding=int(to_send[0]), body_sha=ops.sha(to_send[2:])))
        if u in [s % len(msgs) for s in STORED]:
            arrays[f"to_send_{u}"] = to_send


def record(meta, nodes, extra):
    flats = np.stack([get_flat(s.model) for s in nodes])
    meta["rounds"].append(dict(extra, model_sha=[ops.sha(row) for row in flats]))
    return flats


def run_fullshare(k=255):
    graph = Graph(6)
    for a, b in EDGES6:  # as tests/test_cpu_subsampling_round.py:adjacency fills its sets
        graph.adj_list[a].add(b)
        graph.adj_list[b].add(a)
    meta = new_meta(f"fullshare6_q{k}", "fullshare", 6, [40, 49, 41], k, 3000,
                    edges=[list(e) for e in EDGES6])
    nodes = make_nodes(Sharing, graph, meta)
    arrays = {}
    for it in range(ROUNDS):
        msgs = []
        for u, s in enumerate(nodes):  # DPSGDNode.py:90
            m = s.get_data_to_send(degree=len(graph.neighbors(u)))
            assert isinstance(m["params"], bytes) and m["iteration"] == it
            m["CHANNEL"] = "DPSGD"
            msgs.append(m)
        if it == 0:
            record_wire(meta, arrays, msgs)
        for u, s in enumerate(nodes):  # DPSGDNode.py:111-115
            s._averaging({x: deque([dict(msgs[x])]) for x in graph.neighbors(u)})
            assert s.communication_round == it + 1
        arrays["last"] = record(meta, nodes, {})
    return meta, arrays


def run_el(degree, k=32767):
    graph = Graph()
    graph.read_graph_from_file(os.path.join(OUT, EDGES_FILE), "edges")
    n_nodes = graph.n_procs
    meta = new_meta(f"el_d{degree}_q{k}", "el", n_nodes, [30, 33, 41], k, 4000 + 100 * degree,
                    degree=degree, random_seed=RANDOM_SEED, edges_file=EDGES_FILE)
    nodes = make_nodes(PlainAverageSharing, graph, meta)
    rngs = []
    for u in range(n_nodes):  # EL_Local.py:85-86
        rng = Random()
        rng.seed(RANDOM_SEED + u)
        rngs.append(rng)
    arrays = {}
    for it in range(ROUNDS):
        # EL_Local.py:51; the tuple form draws what the set form drew (make_golden_epidemic.py)
        sends = [set(rngs[u].sample(tuple(graph.neighbors(u)), degree)) for u in range(n_nodes)]
        msgs = []
        for u, s in enumerate(nodes):
            m = s.get_data_to_send()
            assert isinstance(m["params"], bytes) and m["iteration"] == it
            m["CHANNEL"] = "DPSGD"
            msgs.append(m)
        if it == 0:
            record_wire(meta, arrays, msgs)
        for u, s in enumerate(nodes):
            averaging_deque = dict()
            for x in graph.neighbors(u):  # EL_Local.py:145-153
                if u in sends[x]:
                    averaging_deque[x] = deque([dict(msgs[x])])
            if averaging_deque:
                s._averaging(averaging_deque)
            else:
                s.communication_round += 1
            assert s.communication_round == it + 1
        arrays["last"] = record(meta, nodes, dict(
            send_sets=[sorted(s) for s in sends],
            received_this_round=[int(s.received_this_round) for s in nodes]))
    return meta, arrays


def main():
    runs = [run_fullshare(), run_el(7), run_el(1)]
    a, b, c = (m for m, _ in runs)
    assert a["n"] == 2001 and all(w["w"] == 9 for w in a["wire"])
    assert b["n"] == c["n"] == 1031 and all(w["w"] == 16 for w in b["wire"] + c["wire"])
    first = [sum(1 for s in c["rounds"][0]["send_sets"] if i in s) for i in range(c["nodes"])]
    assert 0 in first  # the degree-1 run keeps covering a node that receives nothing
    total = 0
    for meta, arrays in runs:
        path = os.path.join(OUT, f"quant_round_{meta['name']}.npz")
        np.savez_compressed(path, **arrays)
        total += os.path.getsize(path)
        assert os.path.getsize(path) < 2 ** 20
        print(meta["name"], os.path.getsize(path), "bytes", flush=True)
    with open(os.path.join(OUT, "quant_round.json"), "w") as f:
        json.dump({"numpy": np.__version__, "runs": [m for m, _ in runs]}, f, indent=1)
    total += os.path.getsize(os.path.join(OUT, "quant_round.json"))
    print("total", total, "bytes")
    assert total < 400_000


if __name__ == "__main__":
    main()
