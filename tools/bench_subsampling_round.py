#!/usr/bin/env python3
"""Time one rank's share of a whole-topology SubSampling round on the GPU.

The rank is rank 0 of 8 over ``tests/golden/96_regular.edges``: 12 owned nodes whose 3 to 4
neighbours lie anywhere among the 96.  Two variants of the same round, alternated in one call:

  (a) ``SubSamplingRound.step()``: one launch per phase for the 12 nodes (dpz_mt_mask_batch,
      dpz_mask_gather_nodes, dpz_mask_decode_average_nodes);
  (b) the yardstick: the same round composed from the single-node entry points in a host loop
      (``codec.mt_mask``, ``codec.mask_gather``, ``codec.mask_decode_average`` per node), into
      the same row layout, with no host synchronisation at all (so it skips the look at the counts
      that a real caller of the unbounded single gather would need: that favours (b)).

One GPU cannot run the 8-rank all-gather, so the remote nodes' rows are generated once before
the timing (their masks and gathers through the same kernels) and the ``exchange`` leg of both
variants is the part of the all-gather a rank does for itself: the device copy of its 12 rows
into the gathered buffer plus the status words.  The xGMI transfer is NOT measured here.

Device events around each leg, a warm-up, then the median over ``--rounds`` rounds (default
100), ``--runs`` times over (default 3), a, b, a, b, ...; ranges over the runs are reported.
``gate``: the slowest (a) run beats the fastest (b) run by more than both spreads together; the
tool exits non-zero when it does not.  Prints one JSON line.

    python tools/bench_subsampling_round.py [--n 11000000] [--alphas 0.1,0.01] [--rounds 100]
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
from decentralizepy_amd.gossip import read_edges  # noqa: E402
from decentralizepy_amd.gossip_subsampling import SubSamplingRound  # noqa: E402

LEGS = ("mask", "gather", "exchange", "fold")
WORLD = 8


def local_exchange(eng):
    """What a rank's all-gather does for the rank itself (no process group on one GPU)."""
    def exchange():
        eng.recv[:eng.per].copy_(eng.send)
        eng.guard.copy_(eng.recv[:, 2])
    return exchange


def make_engine(adj, x, alpha, seeds):
    eng = SubSamplingRound(adj, x, alpha, seeds, rank=0, world=WORLD)
    eng.exchange = local_exchange(eng)
    return eng


def with_slack(eng):
    """Variant (b)'s single gather takes no cap: a mask past its slot (8 sigma make that a 1e-15
    event; the engine reports it instead) writes on into the following rows.  Its send rows
    become the head of a buffer with n values of slack behind them, so that stays in bounds."""
    extra = -(-eng.N // eng.row_words) + 1
    eng._slack = torch.zeros(eng.per + extra, eng.row_words, dtype=torch.int32,
                             device=eng.device)
    eng.send = eng._slack[:eng.per]
    return eng


def fill_remote_rows(eng, x):
    """Rows of the nodes of ranks 1..7, once: masks and gathers of stand-in models."""
    per, n = eng.per, eng.N
    count = torch.zeros(per, dtype=torch.int64, device=eng.device)
    for r in range(1, WORLD):
        rows = eng.recv[r * per:(r + 1) * per]
        codec.mt_mask_batch([eng.seeds[r * per + j] for j in range(per)], [eng.alpha] * per, n,
                            eng.device, mask=eng._masks(rows), rank_tab=eng._ranks(rows),
                            count=count, workspace=eng._ws)
        tab = codec.gather_node_table(x, eng._masks(rows), eng._ranks(rows), eng._vals(rows),
                                      count, rows[:, 2])
        codec.mask_gather_nodes(tab, n, eng.cap)
        rows[:, :2].copy_(count.view(torch.int32).view(per, 2))
    torch.cuda.synchronize()
    assert not bool(eng.recv[:, 2].any()), "a remote stand-in mask overflowed its slot"


def loop_round(eng, mark):
    """Variant (b): the engine's state and row layout, the single-node entry points per node."""
    m, t = eng.hi - eng.lo, eng.round
    rows = eng.send[:m]
    for j in range(m):
        codec.mt_mask(eng.seeds[eng.lo + j] + t, eng.alpha, eng.N, eng.device,
                      mask=eng._masks(rows[j]), rank_tab=eng._ranks(rows[j]),
                      count=eng._count[j:j + 1], workspace=eng._ws)
    mark("mask")
    for j in range(m):
        codec.mask_gather(eng.x[j], eng._masks(rows[j]), eng._ranks(rows[j]),
                          eng._vals(rows[j]), counter=eng.counter[j])
    mark("gather")
    eng.exchange()
    mark("exchange")
    for j, (nbrs, w, w_self) in enumerate(eng.weights):
        pays = [(eng._masks(eng.recv[q]), eng._ranks(eng.recv[q]), eng._vals(eng.recv[q]))
                for q in nbrs]
        codec.mask_decode_average(eng.x[j], pays, w, w_self, out=eng.out[j])
    mark("fold")
    eng.x, eng.out = eng.out, eng.x
    eng.round += 1


def timed_rounds(run_round, rounds):
    """Median per leg and of the whole round over ``rounds`` rounds, by device events."""
    per_leg = {leg: [] for leg in LEGS + ("total",)}
    for _ in range(rounds):
        evs = [torch.cuda.Event(enable_timing=True)]
        evs[0].record()

        def mark(leg):
            evs.append(torch.cuda.Event(enable_timing=True))
            evs[-1].record()

        run_round(mark)
        evs[-1].synchronize()
        assert len(evs) == len(LEGS) + 1
        for i, leg in enumerate(LEGS):
            per_leg[leg].append(evs[i].elapsed_time(evs[i + 1]))
        per_leg["total"].append(evs[0].elapsed_time(evs[-1]))
    return {leg: float(np.median(v)) for leg, v in per_leg.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=11_000_000)
    ap.add_argument("--alphas", default="0.1,0.01")
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_subsampling_round needs a ROCm GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    adj = read_edges(os.path.join(ROOT, "tests", "golden", "96_regular.edges"))
    n = args.n
    seeds = [1_000_003 * (i + 1) for i in range(len(adj))]
    per = -(-len(adj) // WORLD)
    x = torch.randn(per, n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    res = {"n": n, "nodes": per, "world": WORLD, "rounds": args.rounds, "runs": args.runs,
           "device": torch.cuda.get_device_name(0), "exchange": "local copy only, no xGMI",
           "alphas": {}}
    for alpha in (float(a) for a in args.alphas.split(",")):
        a_eng = make_engine(adj, x, alpha, seeds)
        b_eng = with_slack(make_engine(adj, x, alpha, seeds))
        for eng in (a_eng, b_eng):
            fill_remote_rows(eng, x)
        variants = (("a", lambda mark: a_eng.step(mark)),
                    ("b", lambda mark: loop_round(b_eng, mark)))
        for _ in range(args.warmup):
            for _, fn in variants:
                fn(lambda leg: None)
        torch.cuda.synchronize()
        # both variants ran the same rounds so far: the same models, counters and rows (the loop
        # keeps its counts outside the rows' headers)
        same = (torch.equal(a_eng.x, b_eng.x) and torch.equal(a_eng.counter, b_eng.counter)
                and torch.equal(a_eng.send[:, 4:], b_eng.send[:, 4:]))
        runs = {"a": [], "b": []}
        for _ in range(args.runs):
            for name, fn in variants:
                runs[name].append(timed_rounds(fn, args.rounds))
        r = {"cap": a_eng.cap, "row_bytes": 4 * a_eng.row_words, "results_equal": bool(same)}
        for name in ("a", "b"):
            r[name] = {leg: {"min": min(t[leg] for t in runs[name]),
                             "max": max(t[leg] for t in runs[name]),
                             "runs_ms": [round(t[leg], 4) for t in runs[name]]}
                       for leg in LEGS + ("total",)}
        ta, tb = r["a"]["total"], r["b"]["total"]
        spread = (ta["max"] - ta["min"]) + (tb["max"] - tb["min"])
        r["gate"] = bool(tb["min"] - ta["max"] > spread)
        r["speedup_worst"] = tb["min"] / ta["max"]
        res["alphas"][str(alpha)] = r
        del a_eng, b_eng
        torch.cuda.empty_cache()
    print(json.dumps(res))
    failed = [a for a, r in res["alphas"].items() if not (r["gate"] and r["results_equal"])]
    if failed:
        raise SystemExit(f"gate failed at alpha {failed}: the batched round does not beat the "
                         "host loop by more than the runs' spread, or the two disagree")


if __name__ == "__main__":
    main()
