#!/usr/bin/env python3
"""Generate the SubSampling golden fixtures (tests/golden/subsampling.json + subsampling_*.npz)
from the UNMODIFIED reference ``decentralizepy.sharing.SubSampling`` (sacs-epfl/decentralizepy,
src/decentralizepy/sharing/SubSampling.py).  Run in the build container only (the reference is
not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_subsampling.py

Each scenario: one reference node (its ``seed`` set to a fixed value after construction) and
three reference neighbour nodes with their own models, seeds, alphas and degrees.  Two rounds;
each round the node encodes with get_data_to_send, the neighbours encode theirs, and the node
folds the three payloads with _averaging (or _averaging_server).  The models come from a recorded
generator recipe (tests/subsampling_ops.py:recipe).  The n = 20,001 scenarios store every array
raw; the n = 200,003 scenario stores only counts and SHA-256 hashes of the outputs (its inputs
are regenerated from the recipe).  The node's seed is 2^32 - 1, so ``seed + round`` carries across
2^32 in round 1; the neighbours' seeds cover 0, > 2^32 and > 2^63.
"""
import json
import os
import sys
import tempfile
from collections import OrderedDict, deque

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference/src"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
import torch  # noqa: E402

from decentralizepy.mappings.Linear import Linear  # noqa: E402
from decentralizepy.models.Model import Model  # noqa: E402
from decentralizepy.sharing.SubSampling import SubSampling  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import subsampling_ops as ops  # noqa: E402  (recipe + sha only)

SMALL = [100, 199, 64, 37]    # n = 20,001
LARGE = [400, 499, 300, 103]  # n = 200,003
NEIGHBOURS = [  # seed, alpha, degree, model recipe seed
    {"seed": 0, "alpha": 0.5, "degree": 2, "x_seed": 101},
    {"seed": 2 ** 63 + 12345, "alpha": 0.1, "degree": 3, "x_seed": 102},
    {"seed": 2 ** 32 + 5, "alpha": 0.3, "degree": 5, "x_seed": 103},
]
SCENARIOS = [
    dict(name="flat_a01", shape=SMALL, alpha=0.1, layerwise=False, averaging="_averaging"),
    dict(name="flat_a05", shape=SMALL, alpha=0.5, layerwise=False, averaging="_averaging"),
    dict(name="layer_a01", shape=SMALL, alpha=0.1, layerwise=True, averaging="_averaging"),
    dict(name="layer_a05", shape=SMALL, alpha=0.5, layerwise=True, averaging="_averaging"),
    dict(name="server_a01", shape=SMALL, alpha=0.1, layerwise=False,
         averaging="_averaging_server"),
    dict(name="large_a01", shape=LARGE, alpha=0.1, layerwise=False, averaging="_averaging",
         hashed=True),
]
SEED = 2 ** 32 - 1
ROUNDS = 2


class Net(Model):
    def __init__(self, rows, cols, nb, ne):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(rows, cols))
        self.bias = torch.nn.Parameter(torch.zeros(nb))
        self.scale = torch.nn.Parameter(torch.zeros(ne))


class Graph:
    def __init__(self, nbrs):
        self.nbrs = set(nbrs)

    def neighbors(self, uid):
        return self.nbrs


def set_flat(model, flat):
    new, pos = {}, 0
    for key, v in model.state_dict().items():
        new[key] = torch.from_numpy(flat[pos:pos + v.numel()].reshape(v.shape).copy())
        pos += v.numel()
    model.load_state_dict(new)


def get_flat(model):
    return torch.cat([v.flatten() for v in model.state_dict().values()]).numpy().copy()


def make(sc):
    rows, cols, nb, ne = sc["shape"]
    n = rows * cols + nb + ne
    mapping = Linear(1, 4)
    meta = dict(name=sc["name"], shape=sc["shape"], n=n, alpha=sc["alpha"],
                layerwise=sc["layerwise"], averaging=sc["averaging"], seed=SEED, x0_seed=100,
                neighbours=NEIGHBOURS, rounds=[])
    arrays = {"x0": ops.recipe(100, n)}
    with tempfile.TemporaryDirectory() as tmp:
        model = Net(rows, cols, nb, ne)
        set_flat(model, arrays["x0"])
        node = SubSampling(0, 0, None, mapping, Graph([1, 2, 3]), model, None, tmp,
                           alpha=sc["alpha"], layerwise=sc["layerwise"])
        node.seed = SEED
        nbrs = []
        for j, nbm in enumerate(NEIGHBOURS):
            m = Net(rows, cols, nb, ne)
            arrays[f"nbr{j}_x"] = ops.recipe(nbm["x_seed"], n, 0.5)
            set_flat(m, arrays[f"nbr{j}_x"])
            s = SubSampling(j + 1, 0, None, mapping, Graph([0]), m, None, tmp,
                            alpha=nbm["alpha"], layerwise=sc["layerwise"])
            s.seed = nbm["seed"]
            nbrs.append(s)
    for r in range(ROUNDS):
        data = node.get_data_to_send(degree=3)
        assert list(data) == ["seed", "alpha", "params", "degree", "iteration"]
        assert data["seed"] == SEED + r
        params = np.asarray(data["params"], dtype=np.float32).copy()
        counter = model.shared_parameters_counter.numpy().copy()
        peers = OrderedDict()
        mr = {"k": len(params), "nbr_k": [], "nbr_sha": []}
        for j, s in enumerate(nbrs):
            s.communication_round = r
            m = s.get_data_to_send(degree=NEIGHBOURS[j]["degree"])
            assert m["seed"] == NEIGHBOURS[j]["seed"] + r
            p = np.asarray(m["params"], dtype=np.float32).copy()
            arrays[f"r{r}_nbr{j}_params"] = p
            mr["nbr_k"].append(len(p))
            mr["nbr_sha"].append(ops.sha(p))
            m["CHANNEL"] = "DPSGD"
            peers[j + 1] = deque([m])
        getattr(node, sc["averaging"])(peers)
        after = get_flat(model)
        arrays[f"r{r}_params"], arrays[f"r{r}_counter"] = params, counter
        arrays[f"r{r}_model_after"] = after
        mr.update(params_sha=ops.sha(params), counter_sha=ops.sha(counter),
                  model_sha=ops.sha(after))
        meta["rounds"].append(mr)
    return meta, arrays


def main():
    metas = []
    for sc in SCENARIOS:
        meta, arrays = make(sc)
        metas.append(meta)
        if not sc.get("hashed"):
            path = os.path.join(OUT, f"subsampling_{sc['name']}.npz")
            np.savez_compressed(path, **arrays)
            print(sc["name"], os.path.getsize(path), "bytes", [m["k"] for m in meta["rounds"]])
    with open(os.path.join(OUT, "subsampling.json"), "w") as f:
        json.dump({"scenarios": metas}, f, indent=1)


if __name__ == "__main__":
    main()
