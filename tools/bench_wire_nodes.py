#!/usr/bin/env python3
"""Time the wire layer of the round engines on one GPU: what a round's payloads cost to size and
to code for ``compression_class = EliasFpzip``.

Two shapes, one rank each (no collective is timed):
  sw96    ``JwinsBatchRound`` over ``96_nodes_smallworld.edges``, N = 89,834, the tutorial's alpha
          list (partial shares of six sizes beside full shares);
  reg96   ``TopKAccRound`` over ``96_regular.edges``, N = 11,000,000, alpha = 0.01.

After every round of seeded "training" and ``step()``, alternated in this order:
  size     ``wire_bytes()``: one size-only ``dpz_wire_encode_nodes`` call, two launches;
  code     one ``dpz_wire_encode_nodes`` call that writes every node's streams into its slots;
  loop     the same streams node by node, ``codec.elias_encode`` + ``codec.fpz_encode`` over the
           same payload views: six launches and two host synchronisations a node, the only way to
           get the sizes or the bytes without the batched call.
Wall time from the call to the end of ``torch.cuda.synchronize()`` (the loop is bound by its host
synchronisations, which device events would not see); ``--warmup`` untimed rounds, the median over
``--rounds`` rounds, ``--runs`` times over, ranges over the runs.  The batched sizes are checked
against the loop's stream lengths in every round.  Prints one JSON line per shape.

    python tools/bench_wire_nodes.py [--shapes sw96,reg96] [--rounds 10] [--runs 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from decentralizepy_amd import codec  # noqa: E402
from decentralizepy_amd.gossip import read_edges  # noqa: E402
from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound  # noqa: E402
from decentralizepy_amd.gossip_topkacc import TopKAccRound  # noqa: E402

TUTORIAL_ALPHAS = [0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 1.0]  # tutorial/JWINS/config.ini
SHAPES = {"sw96": ("96_nodes_smallworld.edges", 89_834), "reg96": ("96_regular.edges", 11_000_000)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run_shape(name, args, dev):
    edges, n = SHAPES[name]
    adj = read_edges(os.path.join(ROOT, "tests", "golden", edges))
    m = len(adj)
    gen = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.randn(m, n, device=dev, generator=gen)
    noise = torch.randn(n, device=dev, generator=gen)
    eng = JwinsBatchRound(adj, x0, TUTORIAL_ALPHAS) if name == "sw96" else \
        TopKAccRound(adj, x0, 0.01)
    del x0
    ws = codec.Workspace(dev)

    def loop():
        return [[0 if idx is None else codec.elias_encode(idx, workspace=ws).numel(),
                 codec.fpz_encode(vals, workspace=ws).numel()]
                for idx, vals in eng._wire_views()[1]]

    def size():
        eng._wire_reset()
        return eng.wire_bytes()

    runs = {}
    for run in range(-1, args.runs):  # run -1: the warm-up rounds
        ts = {}
        for r in range(args.warmup if run < 0 else args.rounds):
            for u in range(m):
                eng.x[u].add_(torch.roll(noise, 7919 * (u + 1) + r), alpha=0.01)
            ts.setdefault("step", []).append(wall(eng.step)[0])
            t, sizes = wall(size)
            ts.setdefault("size", []).append(t)
            ts.setdefault("code", []).append(wall(lambda: eng._wire_call(True))[0])
            t, lens = wall(loop)
            ts.setdefault("loop", []).append(t)
            if sizes.tolist() != lens:
                raise SystemExit(f"{name}: the batched sizes differ from the loop's streams")
        if run >= 0:
            for leg, v in ts.items():
                runs.setdefault(leg, []).append(float(np.median(v)))
    res = {"device": torch.cuda.get_device_name(0), "shape": name, "nodes": m, "n": n,
           "rounds": args.rounds, "runs": args.runs, "warmup": args.warmup,
           "wire_bytes_last_round": int(sizes.sum())}
    for leg, v in runs.items():
        res[leg] = {"min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    for leg in ("size", "code"):
        res[f"loop_over_{leg}"] = [round(res["loop"]["min_ms"] / res[leg]["max_ms"], 2),
                                   round(res["loop"]["max_ms"] / res[leg]["min_ms"], 2)]
    res["size_share_of_step"] = [round(res["size"]["min_ms"] / res["step"]["max_ms"], 4),
                                 round(res["size"]["max_ms"] / res["step"]["min_ms"], 4)]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="sw96,reg96")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wire_nodes needs a ROCm GPU; there is no CPU path")
    for name in args.shapes.split(","):
        run_shape(name, args, torch.device("cuda:0"))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
