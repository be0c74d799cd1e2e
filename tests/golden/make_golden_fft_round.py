#!/usr/bin/env python3
"""Generate the whole-topology FFT fixtures (tests/golden/fft_round.json +
fft_round_{reg16,irr6,plain6}.npz) from the UNMODIFIED reference
``decentralizepy.sharing.JWINS.FFT.FFT`` and ``graphs/Graph.py`` (sacs-epfl/decentralizepy).  Run
in the build container only (the reference is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fft_round.py

One reference ``FFT`` object per node of a topology, with the real neighbour sets, ``alpha = 0.1``,
``change_based_selection = True`` and ``compress = False``.  Per round every node "trains" (a
seeded perturbation of 0.01 randn, tests/fft_round_ops.py:train), then ``get_data_to_send``, then
``_averaging`` over its neighbours' actual messages in ``graph.neighbors(u)`` order, as
``node/DPSGDNode.py:90-115`` drives a node.

Runs: ``reg16`` (regular_16.edges, N = 1,030, ``accumulation`` only, 3 rounds), ``irr6`` (the
6-node graph with degrees 1 to 4, N = 4,100, ``accumulate_averaging_changes``, 3 rounds) and
``plain6`` (the same graph, N = 1,024, no accumulation, 2 rounds).  Recorded per round, one row per
node: the payload's indices and complex params, the counter, the accumulator after the encode and
after the averaging (the accumulating runs) and the model after the averaging.  Plain numpy arrays
(allow_pickle=False).

The transform is floating-point and the device's FFT rounds differently from pocketfft, so the
consumers compare values with tolerances and indices exactly: a seed is kept only if in every
selection of the run the k-th key is separated from the (k + 1)-th by a relative gap of at least
1e-4 (the smallest gap of the run is recorded), no recorded float holds -0.0 and all are finite.
"""
import json
import os
import sys
import tempfile
from collections import deque

import numpy as np

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden as mg  # noqa: E402  (puts the reference on sys.path)
import make_golden_jwins_round as mjr  # noqa: E402  (graphs/Graph.py loaded by its path)

from decentralizepy.sharing.JWINS.FFT import FFT  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import fft_round_ops as ops  # noqa: E402  (recipes and the graph's edges only)

Graph, Linear, Net = mjr.Graph, mg.Linear, mg.Net
ALPHA = 0.1


class Retry(RuntimeError):
    pass


def run(meta, graph, shape, seed):
    n_nodes = graph.n_procs
    n = shape[0] * shape[1] + shape[2]
    m_len = n // 2 + 1
    k = round(ALPHA * m_len)
    meta.update(nodes=n_nodes, n=n, shape=list(shape), seed=seed, alpha=ALPHA, m_len=m_len, k=k)
    kwargs = dict(alpha=ALPHA, dict_ordered=True, change_based_selection=True, compress=False,
                  accumulation=meta["accumulation"],
                  accumulate_averaging_changes=meta["accumulate_averaging_changes"])
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal((n_nodes, n)).astype(np.float32)
    mapping = Linear(1, n_nodes)
    nodes = []
    with tempfile.TemporaryDirectory() as tmp:
        for u in range(n_nodes):
            model = Net(*shape)
            mg.set_flat(model, x0[u])
            nodes.append(FFT(u, 0, None, mapping, graph, model, None, tmp, **kwargs))
    arrays = {"x0": x0}
    min_gap = 1.0
    for r in range(meta["rounds"]):
        msgs = []
        rec = {name: [] for name in ("idx", "params", "counter", "acc_enc")}
        for u, s in enumerate(nodes):
            mg.set_flat(s.model, ops.train(mg.get_flat(s.model), meta, r, u))
            m = s.get_data_to_send(degree=len(graph.neighbors(u)))
            assert m["iteration"] == r and m["degree"] == len(graph.neighbors(u))
            assert "send_partial" in m and len(m["indices"]) == k >= 1
            gap = ops.kth_gap(s.model.model_change.abs().numpy(), k)
            if gap < ops.MIN_GAP:
                raise Retry(f"k-th gap {gap:.2e}: node {u} round {r}")
            min_gap = min(min_gap, gap)
            idx = np.array(m["indices"], dtype=np.int32, copy=True)
            assert np.all(np.diff(idx) > 0)
            rec["idx"].append(idx)
            rec["params"].append(np.array(m["params"], dtype=np.complex64, copy=True))
            rec["counter"].append(s.model.shared_parameters_counter.numpy().astype(np.int32))
            if meta["accumulation"]:
                rec["acc_enc"].append(s.model.accumulated_changes.numpy().copy())
            m["params"] = np.array(m["params"], dtype=np.complex64, copy=True)
            m["CHANNEL"] = "DPSGD"
            msgs.append(m)
        for u, s in enumerate(nodes):
            s._averaging({v: deque([dict(msgs[v])]) for v in graph.neighbors(u)})
            assert s.communication_round == r + 1
        for name, rows in rec.items():
            if rows:
                arrays[f"r{r}_{name}"] = np.stack(rows)
        arrays[f"r{r}_x"] = np.stack([mg.get_flat(s.model) for s in nodes])
        if meta["accumulation"]:
            arrays[f"r{r}_acc_avg"] = np.stack([s.model.accumulated_changes.numpy().copy()
                                                for s in nodes])
    for name, a in arrays.items():
        if a.dtype in (np.float32, np.complex64):
            f = a.view(np.float32)
            if np.signbit(f[f == 0]).any():
                raise Retry(f"-0.0 in {name}")
            assert np.isfinite(f).all(), name
    meta["min_gap"] = min_gap
    if meta["accumulate_averaging_changes"]:
        # this mode's encode leaves the accumulator as the last averaging left it, except where it
        # rewinds: stored as those entries alone (fft_round_ops.load_runs puts the rows together
        # again; checked here against the reference's rows bit for bit) - a third less on disk
        for r in range(meta["rounds"]):
            full = arrays.pop(f"r{r}_acc_enc")
            base = arrays[f"r{r - 1}_acc_avg"] if r else np.zeros_like(full)
            at = np.flatnonzero(full.view(np.uint64).reshape(-1) != base.view(np.uint64).reshape(-1))
            arrays[f"r{r}_acc_enc_at"] = at.astype(np.int32)
            arrays[f"r{r}_acc_enc_val"] = full.reshape(-1)[at]
            back = ops.patched(base, arrays[f"r{r}_acc_enc_at"], arrays[f"r{r}_acc_enc_val"])
            assert back.tobytes() == full.tobytes()
    return arrays


def main():
    mg.torch.set_num_threads(4)
    g16 = Graph()
    g16.read_graph_from_file(os.path.join(OUT, "regular_16.edges"), "edges")

    def g6():
        g = Graph(6)
        for a, b in ops.EDGES_IRR6:  # as tests/choco_round_ops.py:adjacency fills its sets
            g.adj_list[a].add(b)
            g.adj_list[b].add(a)
        assert sorted(len(g.neighbors(u)) for u in range(6)) == [1, 1, 2, 3, 3, 4]
        return g

    irr = [list(e) for e in ops.EDGES_IRR6]
    specs = [
        # N = 1,030: M - 1 = 515 = 103 * 5, a generic-prime two-buffer pass; k = 52
        (dict(name="reg16", edges_file="regular_16.edges", rounds=3, accumulation=True,
              accumulate_averaging_changes=False), g16, (30, 33, 40), 71),
        # N = 4,100: 2050 = 205 [41, 5] * 10 [5, 2]; k = 205
        (dict(name="irr6", edges=irr, rounds=3, accumulation=True,
              accumulate_averaging_changes=True), g6(), (50, 81, 50), 72),
        # N = 1,024: 512, in-place radix-8 passes; k = 51
        (dict(name="plain6", edges=irr, rounds=2, accumulation=False,
              accumulate_averaging_changes=False), g6(), (30, 33, 34), 73),
    ]
    metas = []
    for meta, graph, shape, seed0 in specs:
        for seed in range(seed0, seed0 + 4000, 10):
            try:
                arrays = run(meta, graph, shape, seed)
                break
            except Retry as e:
                print("retry:", meta["name"], seed, e, flush=True)
        else:
            raise SystemExit("no well-separated seed")
        assert meta["min_gap"] >= ops.MIN_GAP
        path = os.path.join(OUT, f"fft_round_{meta['name']}.npz")
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        print(meta["name"], meta["n"], meta["m_len"], meta["k"], meta["seed"], meta["min_gap"],
              size, "bytes", flush=True)
        assert size < 1_000_000
        metas.append(meta)
    with open(os.path.join(OUT, "fft_round.json"), "w") as f:
        json.dump({"numpy": np.__version__, "torch": mg.torch.__version__,
                   "reference": "sacs-epfl/decentralizepy v1", "runs": metas}, f, indent=1)


if __name__ == "__main__":
    main()
