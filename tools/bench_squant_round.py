#!/usr/bin/env python3
"""Time a whole-topology top-k round with ``compression="EliasQuantization"`` on one GPU.

Shape: the 96 nodes of ``96_regular.edges`` on one rank (no collective is part of the timing) at
N = 11,000,000, or ``--shape sw96``: ``96_nodes_smallworld.edges`` at N = 89,834; alpha = 0.01,
float_precision k = 32767 (``--alpha``, ``--k``), accumulation mode "acc".

Two engines from the same models, alternated round by round in one process, the same seeded
"training" step added to both between rounds:

  quantised  ``TopKAccRound(compression="EliasQuantization", float_precision=k)``: its encode leg
             ends with the index copy and ONE ``dpz_squant_encode_nodes`` call, its exchange leg
             is ONE ``dpz_squant_decode_nodes`` call and the guard words (on one rank no
             all-gather runs, so what the smaller rows save on the wire is NOT measured; the row
             sizes are reported);
  plain      the same engine uncompressed.

Their models differ after a round (the quantiser is lossy): only times are compared.  After each
round of the quantised engine three more spans are timed on the same payloads:

  quantise   the index copy and the ``dpz_squant_encode_nodes`` call alone (run again: same rows);
  decode     the exchange leg alone (run again: same values);
  loop       today's per-payload calls, node after node: ``codec.quant_encode`` (which reads its
             info record back, one synchronisation per payload) and ``codec.quant_decode``.

Device events around every span, ``--warmup`` untimed rounds, the median over ``--rounds`` rounds,
``--runs`` times over; every figure is the range [min, max] over the runs.  Prints one JSON line
with the device and host names.

    python tools/bench_squant_round.py [--shape sw96] [--n 11000000] [--alpha 0.01] [--k 32767]
"""
import argparse
import json
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from decentralizepy_amd import codec  # noqa: E402
from decentralizepy_amd.gossip import read_edges  # noqa: E402
from decentralizepy_amd.gossip_topkacc import TopKAccRound  # noqa: E402

SHAPES = {"sw96": ("96_nodes_smallworld.edges", 89_834)}


def span(fn):
    """Device milliseconds of what ``fn`` enqueues (host waits inside it included)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed_round(eng):
    """One round; device milliseconds per leg."""
    evs, names = [torch.cuda.Event(enable_timing=True)], []
    evs[0].record()

    def mark(leg):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        evs.append(e)
        names.append(leg)

    eng.step(mark=mark)
    evs[-1].synchronize()
    return {leg: evs[i].elapsed_time(evs[i + 1]) for i, leg in enumerate(names)}


def loop(eng, k):
    """The per-payload calls over the owned nodes' selections of the last encode."""
    ws = codec.Workspace(eng.device)
    for j in range(eng.m):
        vals = eng._pay(eng.send[j])[1]
        body, info = codec.quant_encode(vals, k, workspace=ws)
        codec.quant_decode(body, vals.numel(), info.w, info.scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=11_000_000)
    ap.add_argument("--alpha", type=float, default=0.01)
    ap.add_argument("--k", type=int, default=32767)
    ap.add_argument("--edges", default=os.path.join(ROOT, "tests", "golden", "96_regular.edges"))
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.shape:
        args.edges, args.n = os.path.join(ROOT, "tests", "golden", SHAPES[args.shape][0]), \
            SHAPES[args.shape][1]
    if not torch.cuda.is_available():
        raise SystemExit("bench_squant_round needs a ROCm GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    adj = read_edges(args.edges)
    m, n = len(adj), args.n
    need = (2 * 5 * m + 2 * m + 16) * 4 * n
    free, _ = torch.cuda.mem_get_info(dev)
    if need > 0.9 * free:
        raise SystemExit(f"the state needs {need / 2**30:.1f} GiB, {free / 2**30:.1f} GiB of HBM "
                         "are free: lower --n")
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(m, n, device=dev, generator=gen)
    engines = {"quantised": TopKAccRound(adj, x, args.alpha, float_precision=args.k,
                                         compression="EliasQuantization", device=dev),
               "plain": TopKAccRound(adj, x, args.alpha, device=dev)}
    del x
    noise = torch.empty(m, n, device=dev)
    q = engines["quantised"]
    runs = {}
    for run in range(args.runs):
        acc = {}
        for r in range(args.warmup + args.rounds):
            noise.normal_(0.0, 0.01, generator=gen)
            for name, eng in engines.items():  # alternated round by round
                eng.x.add_(noise)
                t = {f"{name}.{leg}": ms for leg, ms in timed_round(eng).items()}
                t[f"{name}.round"] = sum(t.values())
                if eng is q:
                    t["quantise"] = span(q._squant_rows_encode)
                    t["decode"] = span(q.exchange)
                    t["loop"] = span(lambda: loop(q, args.k))
                if r >= args.warmup:
                    for key, ms in t.items():
                        acc.setdefault(key, []).append(ms)
        for key, ms in acc.items():
            runs.setdefault(key, []).append(float(np.median(ms)))
    if q.guard.any():
        raise SystemExit("a quantised row was refused")
    res = {"device": torch.cuda.get_device_name(dev), "host": socket.gethostname(), "nodes": m,
           "n": n, "alpha": args.alpha, "k": q.k, "float_precision": args.k,
           "rounds": args.rounds, "runs": args.runs,
           "row_words": {"plain": q.row_words, "quantised": q.csend.shape[1]},
           "ms": {key: [round(min(v), 4), round(max(v), 4)] for key, v in sorted(runs.items())}}
    a, b = res["ms"]["quantised.round"], res["ms"]["plain.round"]
    res["quantised_over_plain"] = [round(a[0] / b[1], 3), round(a[1] / b[0], 3)]
    a, b = res["ms"]["loop"], [res["ms"]["quantise"][i] + res["ms"]["decode"][i] for i in (0, 1)]
    res["loop_over_batched"] = [round(a[0] / b[1], 2), round(a[1] / b[0], 2)]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
