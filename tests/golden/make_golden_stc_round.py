#!/usr/bin/env python3
"""Generate the whole-federation STC fixtures (tests/golden/stc_round.json + stc_round_*.npz)
from the UNMODIFIED reference ``decentralizepy.sharing.STC`` (sacs-epfl/decentralizepy).  Run in
the build container only (the reference is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stc_round.py

One reference ``STC`` object per client and one for the server, all with compress=False (the
reference's default compressor EliasFpzipLossy needs fpzip, absent here), driven as
``node/STC/STCClient.py`` and ``node/STC/STCServer.py`` drive them: every client calls
``process_received(None)`` once; then per round each worker, and only a worker, "trains" (a seeded
perturbation, tests/stc_round_ops.py:train) and calls ``get_data_to_send``; the server calls
``_averaging_server`` over the workers' messages in worker order, then ``server_broadcast``; each
worker calls ``process_received`` on a copy of the broadcast.

Runs: ``full8`` (8 clients, N = 2,051, alpha 0.05, 3 rounds, everyone works) and ``part6`` (6
clients, N = 4,100, alpha 0.1, 4 rounds of 3-4 workers, one round's order not ascending, clients
that sit out a round and return).  Recorded: the initial models; per round every worker's payload,
the broadcast payload, all client models and the server model; after the last round every
``residuals`` and ``prev_model``.  Plain numpy arrays (allow_pickle=False).  torch.topk's CPU tie
order is implementation-defined: a seed at which any client or server selection ties at its k-th
key is skipped, and the seed used is recorded.
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
from decentralizepy.sharing.STC import STC  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from oracle import topk as otopk  # noqa: E402
from tests import stc_round_ops as ops  # noqa: E402  (the training recipe only)


class Tie(RuntimeError):
    pass


class Net(Model):
    def __init__(self, rows, cols, nb):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(rows, cols))
        self.bias = torch.nn.Parameter(torch.zeros(nb))


class Star:
    """The server's neighbours are the clients, a client's only neighbour is the server."""

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


def no_tie(change, k, who):
    if otopk.kth_has_tie(otopk.keys_u32(change.numpy()), k):
        raise Tie(who)


def run(meta, shape, seed):
    nc = meta["clients"]
    n = shape[0] * shape[1] + shape[2]
    k = round(meta["alpha"] * n)
    meta.update(n=n, k=k, shape=list(shape), seed=seed, rounds=len(meta["workers"]))
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((nc, n)).astype(np.float32)
    xs0 = rng.standard_normal(n).astype(np.float32)
    mapping = Linear(1, nc + 1)
    kw = dict(alpha=meta["alpha"], compress=False, compression_package=None,
              compression_class=None)
    with tempfile.TemporaryDirectory() as tmp:
        clients = []
        for u in range(nc):
            model = Net(*shape)
            set_flat(model, x0[u])
            clients.append(STC(u, 0, None, mapping, Star([nc]), model, None, tmp, **kw))
        smodel = Net(*shape)
        set_flat(smodel, xs0)
        server = STC(nc, 0, None, mapping, Star(range(nc)), smodel, None, tmp, **kw)
    arrays = {"x0": x0, "xs0": xs0}
    for c in clients:
        c.process_received(None)
    for r, workers in enumerate(meta["workers"]):
        peers = OrderedDict()
        pidx, pvals = [], []
        for u in workers:
            c = clients[u]
            set_flat(c.model, ops.train(get_flat(c.model), meta, r, u))
            data = c.get_data_to_send()
            no_tie(c.model.model_change, k, f"client {u} round {r}")
            pidx.append(np.array(data["indices"], dtype=np.int32, copy=True))
            pvals.append(np.array(data["params"], dtype=np.float32, copy=True))
            msg = dict(data, indices=pidx[-1].copy(), params=pvals[-1].copy())
            msg["degree"], msg["CHANNEL"] = 1, "STC"
            peers[u] = deque([msg])
        server._averaging_server(peers)
        no_tie(server.model.model_change, k, f"server round {r}")
        bdata = server.server_broadcast()
        assert bdata["iteration"] == r + 1
        bidx = np.array(bdata["indices"], dtype=np.int32, copy=True)
        bvals = np.array(bdata["params"], dtype=np.float32, copy=True)
        for u in workers:
            clients[u].process_received({"alpha": bdata["alpha"], "indices": bidx.copy(),
                                         "params": bvals.copy(), "iteration": r + 1})
        assert all(len(i) == k for i in pidx) and len(bidx) == k
        arrays[f"r{r}_p_idx"], arrays[f"r{r}_p_vals"] = np.stack(pidx), np.stack(pvals)
        arrays[f"r{r}_b_idx"], arrays[f"r{r}_b_vals"] = bidx, bvals
        arrays[f"r{r}_x"] = np.stack([get_flat(c.model) for c in clients])
        arrays[f"r{r}_xs"] = get_flat(smodel)
    arrays["res"] = np.stack([c.residuals.numpy().copy() for c in clients])
    arrays["prev"] = np.stack([c.prev_model.numpy().copy() for c in clients])
    arrays["res_s"] = server.residuals.numpy().copy()
    for name, a in arrays.items():  # the fixtures hold no -0: the one stated deviation stays out
        if a.dtype == np.float32:
            assert not np.signbit(a[a == 0]).any(), name
    return arrays


def main():
    specs = [
        (dict(name="full8", clients=8, alpha=0.05, workers=[list(range(8))] * 3), (40, 50, 51), 41),
        (dict(name="part6", clients=6, alpha=0.1,
              workers=[[0, 2, 4, 5], [3, 1, 0], [1, 2, 3, 5], [4, 0, 2]]), (50, 81, 50), 42),
    ]
    metas = []
    for meta, shape, seed0 in specs:
        for seed in range(seed0, seed0 + 400, 10):
            try:
                arrays = run(meta, shape, seed)
                break
            except Tie as e:
                print("retry:", meta["name"], seed, e, flush=True)
        else:
            raise SystemExit("no tie-free seed")
        path = os.path.join(OUT, f"stc_round_{meta['name']}.npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(meta["name"], meta["n"], meta["k"], meta["seed"], size, "bytes", flush=True)
        assert size < 1_000_000
        metas.append(meta)
    with open(os.path.join(OUT, "stc_round.json"), "w") as f:
        json.dump({"numpy": np.__version__, "runs": metas}, f, indent=1)


if __name__ == "__main__":
    main()
