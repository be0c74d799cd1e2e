#!/usr/bin/env python3
"""Time the fold leg of a whole-topology full-model round on the GPU.

Shapes (one rank holds every node, so no exchange is part of the timing):

  el         the EL tutorial round: 16 nodes over tests/golden/fullyConnected_16.edges, every
             node sends to 7 peers drawn by the EL-Local sampler at random_seed 90 (round 0's
             send sets), PlainAverageSharing weights; N = 89,834 (LeNet) and N = 11,000,000;
  fullshare  the D-PSGD full share over tests/golden/96_regular.edges, Metro-Hastings weights,
             N = 11,000,000 (``--n-full``; lower it if 2 x 96 x N floats do not fit the device).

Three variants of the same folds, alternated in one call, from the same models into the same
output rows:

  baseline   one ``codec.decode_average`` with dense payloads per node, in a host loop (what
             existed before the dense kernel; a node with an empty list is a row copy);
  direct     ONE ``dpz_dense_average_nodes`` launch, mode DPZ_DENSE_DIRECT;
  staged     ONE launch, mode DPZ_DENSE_STAGED ("unsupported" where no tile fits the sources).

Device events around ``reps`` back-to-back calls (so that a window is milliseconds, not one
launch), the median over ``--rounds`` windows, ``--runs`` times over, the variants alternating;
the range over the runs is reported with each variant's rate on its OWN algorithmic bytes:
4 N (sum(count_i + 1) + m) for baseline and direct, 4 N (n_src + m) for staged.  ``auto`` says
which path the library's rule takes at the shape and ``auto_ok`` whether that path is not the
slower of the two by more than the runs' spread; the tool exits non-zero when it is, or when
the variants' outputs differ in any bit.  Prints one JSON line.

    python tools/bench_epidemic_round.py [--n-el 89834,11000000] [--n-full 11000000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from decentralizepy_amd import _lib, codec  # noqa: E402
from decentralizepy_amd.gossip import read_edges  # noqa: E402
from decentralizepy_amd.gossip_epidemic import EpidemicRound, FullShareRound  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
VARIANTS = ("baseline", "direct", "staged")


def baseline_fold(eng, lists, ws):
    n = eng.N
    for j, (senders, weights, w_self) in enumerate(lists):
        out = eng._nxt[j, :n]
        if not senders:
            out.copy_(eng._cur[j, :n])
            continue
        codec.decode_average(eng._cur[j, :n], [(None, eng._cur[q, :n]) for q in senders], weights,
                             w_self, out=out, workspace=ws)


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def bench_shape(eng, args):
    lists = eng.lists(0)
    m, n_src, n = eng.hi - eng.lo, eng.n_nodes, eng.N
    reads = sum(len(s) + 1 for s, _, _ in lists)
    table = eng._table(lists)
    ws = codec.Workspace(eng.device)
    tile = codec.dense_tile_elems(n_src)
    fns = {"baseline": lambda: baseline_fold(eng, lists, ws),
           "direct": lambda: codec.dense_average_nodes(table, n, _lib.DPZ_DENSE_DIRECT)}
    if tile:
        fns["staged"] = lambda: codec.dense_average_nodes(table, n, _lib.DPZ_DENSE_STAGED)
    bytes_of = {"baseline": 4 * n * (reads + m), "direct": 4 * n * (reads + m),
                "staged": 4 * n * (n_src + m)}
    # every variant's output, once, before any timing: they must agree in every bit
    outs = {}
    for name, fn in fns.items():
        eng._nxt.fill_(float("nan"))
        fn()
        torch.cuda.synchronize()
        outs[name] = eng._nxt[:m].clone().view(torch.int32)
    same = all(torch.equal(outs["baseline"][:, :n], o[:, :n]) for o in outs.values())
    del outs
    # a window of about 5 ms: from one warm call of the slowest variant
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    reps = {name: max(1, min(200, int(5.0 / max(window_ms(fn, 3), 1e-3))))
            for name, fn in fns.items()}
    runs = {name: [] for name in fns}
    for _ in range(args.runs):
        for name, fn in fns.items():
            runs[name].append(float(np.median([window_ms(fn, reps[name])
                                               for _ in range(args.rounds)])))
    r = {"n": n, "nodes": m, "sources": n_src, "row_reads": reads, "tile": tile,
         "results_equal": bool(same), "launches": {"baseline": sum(1 for _ in lists), "direct": 1,
                                                   "staged": 1}}
    for name in VARIANTS:
        if name not in fns:
            r[name] = "unsupported: no tile fits the sources"
            continue
        t = runs[name]
        r[name] = {"min_ms": min(t), "max_ms": max(t), "runs_ms": [round(v, 5) for v in t],
                   "reps": reps[name], "bytes": bytes_of[name],
                   "tb_per_s": [round(bytes_of[name] / (v * 1e-3) / 1e12, 3)
                                for v in (max(t), min(t))]}
    staged_auto = codec.dense_auto_mode(n_src, reads, n) == _lib.DPZ_DENSE_STAGED
    r["auto"] = "staged" if staged_auto else "direct"
    if tile:
        chosen, other = r[r["auto"]], r["direct" if staged_auto else "staged"]
        spread = (chosen["max_ms"] - chosen["min_ms"]) + (other["max_ms"] - other["min_ms"])
        r["auto_ok"] = bool(chosen["min_ms"] <= other["max_ms"] + spread)
    else:
        r["auto_ok"] = True
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-el", default="89834,11000000")
    ap.add_argument("--n-full", type=int, default=11_000_000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_epidemic_round needs a ROCm GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "runs": args.runs,
           "shapes": {}}
    el_adj = read_edges(os.path.join(GOLDEN, "fullyConnected_16.edges"))
    for n in (int(v) for v in args.n_el.split(",") if v):
        x = torch.randn(len(el_adj), n, device=dev, generator=gen)
        eng = EpidemicRound(el_adj, x, 7, 90)
        del x
        res["shapes"][f"el16_d7_n{n}"] = bench_shape(eng, args)
        del eng
        torch.cuda.empty_cache()
    if args.n_full:
        adj = read_edges(os.path.join(GOLDEN, "96_regular.edges"))
        x = torch.randn(len(adj), args.n_full, device=dev, generator=gen)
        eng = FullShareRound(adj, x)
        del x
        res["shapes"][f"fullshare96_n{args.n_full}"] = bench_shape(eng, args)
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(res))
    bad = [k for k, r in res["shapes"].items() if not (r["results_equal"] and r["auto_ok"])]
    if bad:
        raise SystemExit(f"{bad}: the variants disagree, or auto takes the slower path")


if __name__ == "__main__":
    main()
