#!/usr/bin/env python3
"""Time a whole-topology JWINS round on one GPU: the batched engine against ``JwinsRound``.

Two shapes, one rank each (no collective is part of the timing), the tutorial's alpha list, sym2
at level 4, ``metadata_cap = 0.5``:

  ref96     ``96_regular.edges`` x N = 89,834 (the reference's CIFAR LeNet): 96 small models, a
            node's kernels take microseconds, the round is bound by the host;
  c3_16     ``regular_16.edges`` x N = 25,000,000 (DESIGN's JWINS C3 shape (b)): the kernels take
            the time;
  sw96      ``96_nodes_smallworld.edges`` x N = 89,834: 3 to 10 neighbours per node, the fold's
            any-degree launches (not among the default shapes).

Two variants of the same round, alternated round by round in one process, from the same models
and the same seeded "training" step between rounds, so their states stay equal in every bit
(models, init models, accumulators, counters and payloads; checked after the first two rounds,
before anything is timed, and after the last round):

  engine     ``gossip_jwins_batch.JwinsBatchRound.step``: one launch set per leg for all nodes,
             no host synchronisation;
  baseline   ``gossip_jwins.JwinsRound`` through its own legs (``encode_all``, ``exchange``,
             ``fold_all``): each node's kernels as separate calls on three streams, the status
             words read back once per round.  Its ``fold_all`` holds the fold, the inverse, the
             accumulating transform and the model copy, so the engine's ``fold`` + ``post`` legs
             are compared with it as ``fold_post``.

Per round: device events per leg, ``host_ms`` (wall clock until ``step`` returns: the enqueue,
and for the baseline its read-back) and ``wall_ms`` (wall clock until the round's last event has
completed).  ``--warmup`` untimed rounds, the median over ``--rounds`` rounds, ``--runs`` times
over; the range over the runs is reported, and a speed-up as the range [baseline min / engine
max, baseline max / engine min]: a range that contains 1 is no difference.  Prints one JSON line
per shape.

    python tools/bench_jwins_round.py [--shapes ref96,c3_16,sw96] [--rounds 50] [--runs 3]
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
from decentralizepy_amd.gossip import read_edges  # noqa: E402
from decentralizepy_amd.gossip_jwins import JwinsRound  # noqa: E402
from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound  # noqa: E402

ALPHAS = [0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 1.0]  # tutorial/JWINS/config.ini
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = {"ref96": ("96_regular.edges", 89_834), "c3_16": ("regular_16.edges", 25_000_000),
          "sw96": ("96_nodes_smallworld.edges", 89_834)}


class Baseline:
    """``JwinsRound`` with a ``step(mark)`` over its own legs."""

    def __init__(self, adj, x_init, dev):
        self.eng = JwinsRound(adj, x_init, str(ALPHAS), metadata_cap=0.5, device=dev)
        self.x = self.eng.x

    def step(self, mark):
        e = self.eng
        e.alphas = [rng.choice(e.alpha_list) for rng in e.rngs]
        self.lay = e._layout(e.alphas)
        lay, s_idx, s_val = self.lay
        e.encode_all(lay)
        mark("encode")
        e.exchange(s_idx, s_val)
        mark("exchange")
        e.fold_all(lay, s_idx, s_val)
        mark("fold_post")
        e.round += 1

    def payload(self, q):
        return self.eng._payload(q, *self.lay)


class Engine:
    def __init__(self, adj, x_init, dev):
        self.eng = JwinsBatchRound(adj, x_init, ALPHAS, metadata_cap=0.5, device=dev)
        self.x = self.eng.x

    def step(self, mark):
        self.eng.step(mark=mark)

    def payload(self, q):
        return self.eng.payload(q)


def timed_round(obj):
    """One round: device milliseconds per leg, host_ms until step returned, wall_ms until the
    device finished."""
    evs = [torch.cuda.Event(enable_timing=True)]
    names = []
    t0 = time.perf_counter()
    evs[0].record()

    def mark(leg):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        evs.append(e)
        names.append(leg)

    obj.step(mark)
    t1 = time.perf_counter()
    evs[-1].synchronize()
    t2 = time.perf_counter()
    out = {leg: evs[i].elapsed_time(evs[i + 1]) for i, leg in enumerate(names)}
    out["device_ms"] = evs[0].elapsed_time(evs[-1])
    out["host_ms"] = (t1 - t0) * 1e3
    out["wall_ms"] = (t2 - t0) * 1e3
    return out


def eq(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_state(eng, base):
    a, b = eng.eng, base.eng
    ok = eq(a.x, b.x) and eq(a.x0, b.x0) and eq(a.acc, b.acc) and torch.equal(a.counter, b.counter)
    ok = ok and a.alphas == b.alphas
    for u in range(a.n_nodes):
        (ai, av), (bi, bv) = eng.payload(u), base.payload(u)
        ok = ok and (ai is None) == (bi is None) and (ai is None or torch.equal(ai, bi))
        ok = ok and eq(av, bv)
    return bool(ok)


def run_shape(args, name, dev):
    edges, n = SHAPES[name]
    adj = read_edges(os.path.join(GOLDEN, edges))
    m = len(adj)
    need = 14 * m * 4 * n + (1 << 30)  # both variants' rows, payload buffers, the initial models
    free, _ = torch.cuda.mem_get_info(dev)
    if need > 0.9 * free:
        raise SystemExit(f"{name}: the state needs {need / 2**30:.1f} GiB, {free / 2**30:.1f} GiB "
                         "of HBM are free")
    gen = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.randn(m, n, device=dev, generator=gen)
    noise = torch.randn(n, device=dev, generator=gen)  # the "training" step, rolled per node
    variants = {"engine": Engine(adj, x0, dev), "baseline": Baseline(adj, x0, dev)}
    del x0
    eng, base = variants["engine"], variants["baseline"]

    def train(r):
        for obj in variants.values():
            for u in range(m):
                obj.x[u].add_(torch.roll(noise, 7919 * (u + 1) + r), alpha=0.01)

    r = 0
    for _ in range(2):  # the check at the timed size, before anything is timed
        train(r)
        for obj in variants.values():
            timed_round(obj)
        r += 1
    torch.cuda.synchronize()
    if not same_state(eng, base):
        raise SystemExit(f"{name}: the engine's and the baseline's states differ after two "
                         "rounds; nothing was timed")
    for _ in range(args.warmup):
        train(r)
        for obj in variants.values():
            timed_round(obj)
        r += 1
    runs = {v: {} for v in variants}
    for _ in range(args.runs):
        legs = {v: {} for v in variants}
        for _ in range(args.rounds):
            train(r)
            torch.cuda.synchronize()
            for v, obj in variants.items():
                for leg, ms in timed_round(obj).items():
                    legs[v].setdefault(leg, []).append(ms)
            r += 1
        for v in variants:
            for leg, ts in legs[v].items():
                runs[v].setdefault(leg, []).append(float(np.median(ts)))
    torch.cuda.synchronize()
    same = same_state(eng, base)
    res = {"shape": name, "device": torch.cuda.get_device_name(0), "nodes": m, "n": n,
           "m_len": eng.eng.M, "alpha_list": ALPHAS, "rounds": args.rounds, "runs": args.runs,
           "warmup": args.warmup + 2, "total_rounds": r, "equal_after_two_rounds": True,
           "results_equal": same}
    for v in variants:
        res[v] = {leg: {"min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                        "runs_ms": [round(x, 4) for x in t]} for leg, t in runs[v].items()}
    e, b = res["engine"], res["baseline"]
    e["fold_post"] = {"min_ms": round(e["fold"]["min_ms"] + e["post"]["min_ms"], 4),
                      "max_ms": round(e["fold"]["max_ms"] + e["post"]["max_ms"], 4)}
    for leg in ("encode", "fold_post", "device_ms", "host_ms", "wall_ms"):
        res[f"{leg}_speedup"] = [round(b[leg]["min_ms"] / e[leg]["max_ms"], 2),
                                 round(b[leg]["max_ms"] / e[leg]["min_ms"], 2)]
    print(json.dumps(res), flush=True)
    if not same:
        raise SystemExit(f"{name}: the engine's and the baseline's states differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ref96,c3_16")
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jwins_round needs a ROCm GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        if name not in SHAPES:
            raise SystemExit(f"unknown shape {name}")
        run_shape(args, name, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
