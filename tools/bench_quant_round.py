#!/usr/bin/env python3
"""Time the legs of a quantised whole-topology full-model round on the GPU.

Workloads, each at float_precision k = 32767 (16-bit fields) and k = 127 (8-bit fields):

  el16       16 nodes over tests/golden/fullyConnected_16.edges on one rank, EL-Local at degree
             7, random_seed 90 (``QuantEpidemicRound`` in place: no all-gather);
  fs96r12    rank 0 of 8 of the D-PSGD full share over tests/golden/96_regular.edges: the
             rank's 12 nodes fold from the 96 gathered rows (``QuantFullShareRound``).  One GPU
             stands in for the world: the other ranks' rows are encoded once beforehand and the
             all-gather is replaced by the copy of the rank's own block into the gathered buffer,
             so the "exchange" leg here is a device copy, NOT a measurement of the interconnect.

Three variants of the same round, alternated in one call on the same models:

  quant      the engine: ``dpz_quant_encode_nodes``, the exchange, ``dpz_qdense_average_nodes``;
  plain      the uncompressed ``EpidemicRound`` / ``FullShareRound`` (another result: a yardstick
             of time and bytes only);
  composed   what existed before: per owned node ``quant_encode`` (one host round trip each),
             ``quant_decode`` of every distinct row the rank folds into an fp32 row, one
             ``dense_average_nodes`` over the decoded rows.  Each distinct row is decoded once
             per round, which favours this variant over a per-receiver decode.

Per variant: the legs by device events recorded after each leg is enqueued (``mark``), and the
wall time of a step (host clock around ``--steps`` steps ending in a synchronise: the host work of
a step, table building and round trips, shows only there); the median over ``--windows`` windows,
``--runs`` times over with the variants alternating, min and max over the runs reported.  The
quant and the composed variant must agree in every bit; the tool exits non-zero otherwise.
Prints one JSON line.

    python tools/bench_quant_round.py [--n 11000000] [--k 32767,127]
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
from decentralizepy_amd import _lib, codec  # noqa: E402
from decentralizepy_amd.gossip import read_edges  # noqa: E402
from decentralizepy_amd.gossip_epidemic import EpidemicRound, FullShareRound  # noqa: E402
from decentralizepy_amd.gossip_quant import QuantEpidemicRound, QuantFullShareRound  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def loop_back(eng):
    """One GPU stands in for the world: the all-gather becomes the copy of the own block."""
    eng.all_gather = lambda recv, send: recv[:eng.per].copy_(send)


class Composed:
    """Per-node quant_encode + quant_decode of every distinct row + one dense fold, over the
    models and the gathered rows of a quantised engine (foreign rows: their packed bodies)."""

    def __init__(self, eng, lists):
        self.eng, self.lists = eng, lists
        self.need = sorted({q for s, _, _ in lists for q in s})
        dev, n = eng.device, eng.N
        self.dec = torch.zeros(len(self.need), eng.stride, dtype=torch.float32, device=dev)
        self.out = torch.zeros(eng.m, eng.stride, dtype=torch.float32, device=dev)
        self.ws = codec.Workspace(dev)
        at = {q: i for i, q in enumerate(self.need)}
        self.foreign = {}
        for q in self.need:
            if not eng.lo <= q < eng.hi:
                info = eng.rows[q, codec.QROW_INFO:codec.QROW_BODY].cpu().numpy()
                body = eng.rows[q, codec.QROW_BODY:].view(torch.uint8)
                self.foreign[q] = (body, int(info[1]), float(info[3:4].view(np.float32)[0]))
        srcs = [self.dec[i, :n] for i in range(len(self.need))] + \
            [eng._cur[j, :n] for j in range(eng.m)]
        self.table = codec.DenseTable(
            srcs, [(self.out[j], len(self.need) + j, w_self, [(at[q], w) for q, w in zip(s, ws)])
                   for j, (s, ws, w_self) in enumerate(lists)], dev)

    def step(self, mark=None):
        mark = mark or (lambda leg: None)
        eng, n = self.eng, self.eng.N
        own = {}
        for j in range(eng.m):
            body, info = codec.quant_encode(eng._cur[j, :n], eng.k, workspace=self.ws)
            own[eng.lo + j] = (body, info.w, float(info.scale))
        mark("encode")
        for i, q in enumerate(self.need):
            body, w, scale = own[q] if q in own else self.foreign[q]
            codec.quant_decode(body, n, w, scale, out=self.dec[i])
        mark("decode")
        codec.dense_average_nodes(self.table, n)
        mark("fold")


def measure(step, legs, reset, args):
    """Median over the windows of (wall ms per step, {leg: ms per step}); ``reset`` runs before
    every window, outside the timing."""
    wall, leg_ms = [], {leg: [] for leg in legs}
    for _ in range(args.windows):
        evs = []
        reset()

        def mark(leg):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            evs.append(e)

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            mark("start")
            step(mark)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / args.steps)
        per = len(legs) + 1
        for i, leg in enumerate(legs):
            leg_ms[leg].append(sum(evs[s * per + i].elapsed_time(evs[s * per + i + 1])
                                   for s in range(args.steps)) / args.steps)
    return float(np.median(wall)), {leg: float(np.median(v)) for leg, v in leg_ms.items()}


def bench(name, quant, plain, fresh_lists, args):
    n, m = quant.N, quant.m
    lists = fresh_lists()
    quant.step()  # the rows now hold this rank's streams too
    torch.cuda.synchronize()
    comp = Composed(quant, lists)
    # the engine's fold of these lists against the composed sequence, on the same models
    quant.encode()
    quant.exchange()
    quant.fold(lists, quant._table(lists))
    comp.step()
    torch.cuda.synchronize()
    same = torch.equal(quant._nxt[:m, :n].view(torch.int32), comp.out[:, :n].view(torch.int32))
    quant.check()
    # The reference's quantiser rescales by mean|x| where it normalised by max|x|, so without
    # training between the rounds every round shrinks the models (by about the node's own weight)
    # and a few dozen rounds reach subnormal norms: every window starts from the same models.
    x0, p0 = quant.x.clone(), plain.x.clone()

    def reset():
        quant.x.copy_(x0)
        plain.x.copy_(p0)

    variants = {"quant": (quant.step, ("encode", "exchange", "fold")),
                "plain": (plain.step, ("exchange", "fold")),
                "composed": (comp.step, ("encode", "decode", "fold"))}
    for step, _ in variants.values():
        for _ in range(args.warmup):
            step()
    reset()
    runs = {v: [] for v in variants}
    for _ in range(args.runs):
        for v, (step, legs) in variants.items():
            runs[v].append(measure(step, legs, reset, args))
            quant.check()
    d = sum(len(s) for s, _, _ in lists)
    w = quant.slot_bits
    r = {"n": n, "nodes": m, "sources": quant.n_nodes, "senders_folded": d, "k": quant.k,
         "slot_bits": w, "results_equal": bool(same),
         "auto": {1: "staged", 2: "direct"}[codec.qdense_auto_mode(
             quant.rows.shape[0], d + m, n)] if quant.mode == 0 else quant.mode,
         # algorithmic bytes of the fold (direct path) and of a rank's all-gather block
         "fold_bytes": {"quant": n * (8 * m + d * w // 8), "plain": n * (8 * m + 4 * d)},
         "gather_block_bytes": {"quant": 4 * quant.per * quant.row_words,
                                "plain": 4 * plain.per * plain.stride}}
    for v, (_, legs) in variants.items():
        walls = [t for t, _ in runs[v]]
        r[v] = {"step_wall_ms": [round(min(walls), 4), round(max(walls), 4)]}
        for leg in legs:
            t = [ms[leg] for _, ms in runs[v]]
            r[v][leg + "_ms"] = [round(min(t), 4), round(max(t), 4)]
    print(name, json.dumps(r), file=sys.stderr, flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=11_000_000)
    ap.add_argument("--k", default="32767,127")
    ap.add_argument("--workloads", default="el16,fs96r12")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mode", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_quant_round needs a ROCm GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    n = args.n
    res = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "windows": args.windows,
           "runs": args.runs, "shapes": {}}
    for k in (int(v) for v in args.k.split(",") if v):
        if "el16" in args.workloads:
            adj = read_edges(os.path.join(GOLDEN, "fullyConnected_16.edges"))
            x = torch.randn(16, n, device=dev, generator=gen)
            quant = QuantEpidemicRound(adj, x, 7, 90, k, mode=args.mode)
            plain = EpidemicRound(adj, x, 7, 90)
            del x
            res["shapes"][f"el16_d7_n{n}_k{k}"] = bench(
                "el16", quant, plain, lambda: EpidemicRound(
                    adj, torch.zeros(16, 4, device=dev), 7, 90).lists(0), args)
            del quant, plain
            torch.cuda.empty_cache()
        if "fs96r12" in args.workloads:
            adj = read_edges(os.path.join(GOLDEN, "96_regular.edges"))
            x = torch.randn(12, n, device=dev, generator=gen)
            quant = QuantFullShareRound(adj, x, k, rank=0, world=8, mode=args.mode)
            plain = FullShareRound(adj, x, rank=0, world=8)
            loop_back(quant)
            loop_back(plain)
            for b in range(8):  # every rank's rows, encoded once: block 0 last, from x itself
                blk = x if b == 7 else torch.randn(12, n, device=dev, generator=gen)
                quant.x.copy_(blk)
                quant.encode()
                quant.recv[(7 - b) * 12:(8 - b) * 12].copy_(quant.send)
                plain.recv[(7 - b) * 12:(8 - b) * 12, :n].copy_(blk)
            del x, blk
            res["shapes"][f"fs96_rank12_n{n}_k{k}"] = bench(
                "fs96r12", quant, plain, lambda: quant.lists(0), args)
            del quant, plain
            torch.cuda.empty_cache()
    print(json.dumps(res))
    bad = [s for s, r in res["shapes"].items() if not r["results_equal"]]
    if bad:
        raise SystemExit(f"{bad}: the engine and the composed sequence disagree")


if __name__ == "__main__":
    main()
