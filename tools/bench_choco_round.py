#!/usr/bin/env python3
"""Time the legs of a whole-topology Choco-SGD round on one GPU.

Shape: every node of tests/golden/96_regular.edges on one rank (no exchange is part of the
timing), N = 11,000,000, alpha = 0.01 (``--n``, ``--alpha``; the state is 96 x 3 x 4 N bytes per
variant plus the baseline's dense q rows).

Two variants of the same round, alternated round by round in one process, from the same models
and the same seeded "training" step between rounds, so their states stay equal in every bit
(checked after the last round):

  engine     ``gossip_choco.ChocoRound.step``: the ``dpz_choco_encode_nodes`` launch set and ONE
             ``dpz_choco_fold_nodes`` launch for all nodes;
  baseline   the per-node call sequence of the plugin ``sharing/Choco.py``, node after node:
             DPZ_EW_SUB, ``topk_threshold`` (blocks on its count), ``mask_below_threshold``; then
             DPZ_EW_ADD, the zero-based accumulating ``decode_average``, DPZ_EW_CHOCO.

Device events per leg (through the engine's ``mark``; around the baseline's two loops), ``--warmup``
untimed rounds, the median over ``--rounds`` rounds, ``--runs`` times over; the range over the
runs is reported.  Rates are over each leg's algorithmic bytes: the encode reads x and x_hat in
each of its five passes (three histograms, count, compaction), 40 N bytes per node, and writes 8
bytes per entry; the fold reads x, x_hat and s and writes x and s (x_hat is rewritten only
where the node's own payload changed it, 16 bytes around each entry), 20 N bytes per node, plus 8
bytes per payload entry read.  ``copy_tb_per_s`` is a
device-to-device copy of 1 GiB timed in the same process.  Prints one JSON line.

    python tools/bench_choco_round.py [--n 11000000] [--alpha 0.01] [--nodes 96]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from decentralizepy_amd import codec  # noqa: E402
from decentralizepy_amd.gossip import mh_weights, read_edges  # noqa: E402
from decentralizepy_amd.gossip_choco import ChocoRound  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


class Baseline:
    """The same round through the per-node plugin's device calls (sharing/Choco.py)."""

    def __init__(self, adj, x_init, alpha, step_size):
        self.adj, self.step_size = adj, step_size
        self.x = x_init.clone()
        self.x_hat = torch.zeros_like(self.x)
        self.s = torch.zeros_like(self.x)
        self.q = torch.empty_like(self.x)
        self.k = round(alpha * x_init.shape[1])
        self.ws = codec.Workspace(x_init.device)
        self.weights = [mh_weights(adj, i) for i in range(len(adj))]
        self.pay = [None] * len(adj)

    def encode(self):
        for u in range(len(self.adj)):
            codec.elementwise(codec.DPZ_EW_SUB, self.x[u], self.x_hat[u], out=self.q[u])
            self.pay[u] = codec.topk_threshold(self.q[u], self.k, workspace=self.ws)
            codec.mask_below_threshold(self.q[u], self.ws)

    def fold(self):
        for u, (nbrs, w, w_self) in enumerate(self.weights):
            codec.elementwise(codec.DPZ_EW_ADD, self.x_hat[u], self.q[u], out=self.x_hat[u])
            codec.decode_average(self.q[u], [self.pay[v] for v in nbrs], w, w_self,
                                 out=self.s[u], zero_base=True, accumulate=True,
                                 workspace=self.ws)
            codec.elementwise(codec.DPZ_EW_CHOCO, self.x[u], self.s[u], self.x_hat[u],
                              self.step_size, out=self.x[u])

    def step(self, mark):
        self.encode()
        mark("encode")
        self.fold()
        mark("fold")


def timed_round(obj):
    """One round; device milliseconds per leg."""
    evs = [torch.cuda.Event(enable_timing=True)]
    names = []
    evs[0].record()

    def mark(leg):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        evs.append(e)
        names.append(leg)

    obj.step(mark)
    evs[-1].synchronize()
    return {leg: evs[i].elapsed_time(evs[i + 1]) for i, leg in enumerate(names)}


def copy_rate(dev):
    a = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    ts = []
    for i in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        if i >= 2:
            ts.append(e0.elapsed_time(e1))
    return 2 * a.numel() * 4 / (float(np.median(ts)) * 1e-3) / 1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=11_000_000)
    ap.add_argument("--alpha", type=float, default=0.01)
    ap.add_argument("--step-size", type=float, default=0.5)
    ap.add_argument("--nodes", type=int, default=96, help="the first nodes of 96_regular (edges "
                    "among them): lower it if the state does not fit the device")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_choco_round needs a ROCm GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    adj = read_edges(os.path.join(GOLDEN, "96_regular.edges"))
    if args.nodes < len(adj):
        adj = [{v for v in a if v < args.nodes} for a in adj[:args.nodes]]
    m, n = len(adj), args.n
    gen = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.randn(m, n, device=dev, generator=gen)
    noise = torch.randn(n, device=dev, generator=gen)  # the "training" step, rolled per node
    eng = ChocoRound(adj, x0, args.alpha, args.step_size)
    base = Baseline(adj, x0, args.alpha, args.step_size)
    del x0
    variants = {"engine": eng, "baseline": base}

    def train(r):
        for obj in variants.values():
            for u in range(m):
                obj.x[u].add_(torch.roll(noise, 7919 * (u + 1) + r), alpha=0.01)

    r = 0
    for _ in range(args.warmup):
        train(r)
        for obj in variants.values():
            timed_round(obj)
        r += 1
    eng.check()
    runs = {name: {} for name in variants}
    for _ in range(args.runs):
        legs = {name: {} for name in variants}
        for _ in range(args.rounds):
            train(r)
            for name, obj in variants.items():
                for leg, ms in timed_round(obj).items():
                    legs[name].setdefault(leg, []).append(ms)
            r += 1
        for name in variants:
            for leg, ts in legs[name].items():
                runs[name].setdefault(leg, []).append(float(np.median(ts)))
    eng.check()
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
               for a, b in ((eng.x, base.x), (eng.x_hat, base.x_hat), (eng.s, base.s)))
    counts = [eng.payload(q)[0].numel() for q in range(m)]
    entries = sum(counts)
    fold_entries = sum(counts[u] + sum(counts[v] for v in adj[u]) for u in range(m))
    bytes_of = {"encode": 40 * n * m + 8 * entries,
                "fold": 20 * n * m + 8 * fold_entries + 16 * entries}
    copy = copy_rate(dev)
    res = {"device": torch.cuda.get_device_name(0), "nodes": m, "n": n, "alpha": args.alpha,
           "k": eng.k, "cap": eng.cap, "max_count": max(counts), "rounds": args.rounds,
           "runs": args.runs, "warmup": args.warmup, "results_equal": bool(same),
           "copy_tb_per_s": round(copy, 3), "bytes": bytes_of}
    for name in variants:
        res[name] = {}
        for leg, t in runs[name].items():
            res[name][leg] = {"min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                              "runs_ms": [round(v, 4) for v in t]}
            if leg in bytes_of and name == "engine":
                res[name][leg]["tb_per_s"] = [round(bytes_of[leg] / (v * 1e-3) / 1e12, 3)
                                              for v in (max(t), min(t))]
                res[name][leg]["of_copy_rate"] = [round(bytes_of[leg] / (v * 1e-3) / 1e12 / copy, 3)
                                                  for v in (max(t), min(t))]
    for leg in ("encode", "fold"):
        e, b = res["engine"][leg], res["baseline"][leg]
        res[f"{leg}_speedup"] = [round(b["min_ms"] / e["max_ms"], 2),
                                 round(b["max_ms"] / e["min_ms"], 2)]
    print(json.dumps(res))
    if not same:
        raise SystemExit("the engine's and the baseline's states differ")


if __name__ == "__main__":
    main()
