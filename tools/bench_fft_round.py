#!/usr/bin/env python3
"""Time a whole-topology FFT-sharing round on one GPU: ``FftRound`` against the per-node plugin's
call sequence.

Three shapes, one rank each (no collective is part of the timing), ``alpha = 0.1``,
``accumulation`` with ``accumulate_averaging_changes``:

  ref96     ``96_regular.edges`` x N = 90,112 (the native even size nearest the reference's CIFAR
            LeNet, 89,834 = 2 * 44,917, which has no native plan): 96 small models, a node's
            kernels take microseconds, the round is bound by the host;
  c4_96     ``96_regular.edges`` x N = 11,000,000 (DESIGN's C4 model; 5.5 M = 220 * 125 * 200);
  c3_16     ``regular_16.edges`` x N = 25,000,000.

Two variants of the same round, alternated round by round in one process, from the same models
and the same seeded "training" step between rounds, so their states stay equal in every bit
(models, init models, accumulators, counters and payloads; checked after the first two rounds,
before anything is timed, and after the last round):

  engine     ``gossip_fft.FftRound.step``: one launch set per leg for all nodes, no host
             synchronisation;
  baseline   the device calls ``sharing.JWINS.FFT`` makes, node after node on device rows:
             ``elementwise(SUB)``, two ``rfft``, ``cplx_key``, the exact ``topk_encode`` with the
             counter, ``cplx_gather``, ``cplx_pair_indices``; ``decode_average`` over the float
             view; ``irfft``, ``elementwise(SUB)``, ``rfft``, ``elementwise(ADD)``, the copy of the
             model.  The plugin's trip of every payload through host numpy arrays is NOT part of
             it, so it is a lower bound of what plugin objects cost.

Per round: device events per leg, ``host_ms`` (wall clock until ``step`` returns) and ``wall_ms``
(wall clock until the round's last event has completed).  ``--warmup`` untimed rounds, the median
over ``--rounds`` rounds, ``--runs`` times over; the range over the runs is reported, and a
speed-up as the range [baseline min / engine max, baseline max / engine min]: a range that
contains 1 is no difference.  Prints one JSON line per shape.

    python tools/bench_fft_round.py [--shapes ref96,c4_96,c3_16] [--rounds 0] [--runs 3]

``--chirp`` times another pair instead, at a size without a native plan (``--shapes lenet96``:
``96_regular.edges`` x N = 89,834): ``FftRound(chirp=True)`` (reported as ``engine``: the chirp-z
launch sets) against ``FftRound()`` (reported as ``baseline``: hipFFT node after node).  They are
two algorithms for the same transforms, so what is checked is that their F(x) of the first round
(from equal models) agree to 1e-5 of the largest coefficient; a selection whose k-th and
(k + 1)-th keys lie closer than the rounding may differ, and the models then go their own way.
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
from decentralizepy_amd.gossip import mh_weights, read_edges  # noqa: E402
from decentralizepy_amd.gossip_fft import FftRound  # noqa: E402

ALPHA = 0.1
GOLDEN = os.path.join(ROOT, "tests", "golden")
# edges, N, timed rounds per run (when --rounds is 0)
SHAPES = {"ref96": ("96_regular.edges", 90_112, 50),
          "c4_96": ("96_regular.edges", 11_000_000, 8),
          "c3_16": ("regular_16.edges", 25_000_000, 8),
          "small16": ("regular_16.edges", 4_100, 20),  # a quick check of the tool itself
          # --chirp only: the reference's CIFAR LeNet itself, a size without a native plan
          "lenet96": ("96_regular.edges", 89_834, 50),
          "chirp16": ("regular_16.edges", 8_198, 20)}


class Baseline:
    """The per-node plugin's device calls, node after node, on device rows of its own."""

    def __init__(self, adj, x_init, dev):
        self.adj, self.dev = adj, dev
        m, n = x_init.shape
        self.n, self.M = n, n // 2 + 1
        self.k = round(ALPHA * self.M)
        self.x, self.x0 = x_init.clone(), x_init.clone()
        c = dict(dtype=torch.complex64, device=dev)
        self.fx = torch.empty(m, self.M, **c)
        self.ch = torch.empty(m, self.M, **c)
        self.acc = torch.zeros(m, self.M, **c)
        self.counter = torch.zeros(m, self.M, dtype=torch.int32, device=dev)
        self.diff = torch.empty(n, device=dev)
        self.d = torch.empty(self.M, **c)
        self.key = torch.empty(self.M, device=dev)
        pad = -(-2 * self.k // 64) * 64  # payload rows on 256-byte boundaries, as the engine's
        self.idx = torch.empty(m, pad, dtype=torch.int32, device=dev)[:, :self.k]
        self.pair = torch.empty(m, pad, dtype=torch.int32, device=dev)[:, :2 * self.k]
        self.val = torch.empty(m, pad, **c)[:, :self.k]
        self.ws = codec.Workspace(dev)
        self.weights = [mh_weights(adj, i) for i in range(m)]

    def step(self, mark):
        m, n = self.x.shape
        for j in range(m):
            codec.elementwise(codec.DPZ_EW_SUB, self.x[j], self.x0[j], out=self.diff)
            codec.rfft(self.x[j], out=self.fx[j], workspace=self.ws)
            codec.rfft(self.diff, out=self.ch[j], workspace=self.ws)
            codec.cplx_key(self.ch[j], self.acc[j], codec.DPZ_ACC_ADD, out=self.key)
            codec.topk_encode(self.key, self.k, counter=self.counter[j], idx_out=self.idx[j],
                              workspace=self.ws, exact=True)
            codec.cplx_gather(self.fx[j], self.idx[j], acc=self.acc[j], out=self.val[j])
            codec.cplx_pair_indices(self.idx[j], out=self.pair[j])
        mark("encode")
        mark("exchange")
        for j, (nbrs, w, w_self) in enumerate(self.weights):
            pays = [(self.pair[q], torch.view_as_real(self.val[q]).view(-1)) for q in nbrs]
            codec.decode_average(torch.view_as_real(self.fx[j]).view(-1), pays, w, w_self,
                                 out=torch.view_as_real(self.ch[j]).view(-1), workspace=self.ws)
        mark("fold")
        for j in range(m):
            codec.irfft(self.ch[j], n, out=self.x[j], workspace=self.ws)
            codec.elementwise(codec.DPZ_EW_SUB, self.x[j], self.x0[j], out=self.diff)
            codec.rfft(self.diff, out=self.d, workspace=self.ws)
            a = torch.view_as_real(self.acc[j]).view(-1)
            codec.elementwise(codec.DPZ_EW_ADD, a, torch.view_as_real(self.d).view(-1), out=a)
        self.x0.copy_(self.x)
        mark("post")

    def payload(self, q):
        return self.idx[q], self.val[q]


class Engine:
    def __init__(self, adj, x_init, dev, chirp=False):
        self.eng = FftRound(adj, x_init, ALPHA, accumulation=True,
                            accumulate_averaging_changes=True, device=dev, chirp=chirp)
        self.x, self.x0 = self.eng.x, self.eng.x0
        self.acc, self.counter = self.eng.acc, self.eng.counter

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
    a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def close_state(eng, base, m):
    """--chirp: two algorithms for the same transforms.  F(x) of the first round comes from equal
    models and agrees to rounding; where the k-th and the (k + 1)-th key of a node lie closer than
    that rounding the selections differ, and the models follow their own course from there (one
    tipped coefficient moves a model by about 1e-3), so nothing else is compared."""
    f, g = eng.eng.fx, base.eng.fx
    return float((f - g).abs().max()) <= 1e-5 * float(g.abs().max())


def same_state(eng, base, m):
    ok = eq(eng.x, base.x) and eq(eng.x0, base.x0) and eq(eng.acc, base.acc)
    ok = ok and torch.equal(eng.counter, base.counter)
    for u in range(m):
        (ai, av), (bi, bv) = eng.payload(u), base.payload(u)
        ok = ok and torch.equal(ai, bi) and eq(av, bv)
    return bool(ok)


def run_shape(args, name, dev):
    edges, n, rounds = SHAPES[name]
    rounds = args.rounds or rounds
    adj = read_edges(os.path.join(GOLDEN, edges))
    m = len(adj)
    if not codec.fft_native(n) and not args.chirp:
        raise SystemExit(f"{name}: N = {n} has no native plan")
    need = 26 * m * 4 * n + (1 << 30)  # both variants' rows, the workspace, the initial models
    free, _ = torch.cuda.mem_get_info(dev)
    if need > 0.9 * free:
        raise SystemExit(f"{name}: the state needs {need / 2**30:.1f} GiB, {free / 2**30:.1f} GiB "
                         "of HBM are free")
    gen = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.randn(m, n, device=dev, generator=gen)
    noise = torch.randn(n, device=dev, generator=gen)  # the "training" step, rolled per node
    if args.chirp:  # the chirp-z engine against the same engine without the keyword
        variants = {"engine": Engine(adj, x0, dev, chirp=True), "baseline": Engine(adj, x0, dev)}
    else:
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
        if args.chirp and r == 1 and not close_state(eng, base, m):
            raise SystemExit(f"{name}: the two engines' F(x) of the first round differ by more "
                             "than rounding; nothing was timed")
    if not args.chirp and not same_state(eng, base, m):
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
        for _ in range(rounds):
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
    same = None if args.chirp else same_state(eng, base, m)  # --chirp: checked after round one
    res = {"shape": name, "device": torch.cuda.get_device_name(0), "nodes": m, "n": n,
           "m_len": eng.eng.M, "k": eng.eng.k, "alpha": ALPHA, "rounds": rounds,
           "runs": args.runs, "warmup": args.warmup + 2, "total_rounds": r,
           "equal_after_two_rounds": True, "results_equal": same, "chirp": args.chirp,
           "batched": eng.eng.batched, "native": eng.eng.native}
    for v in variants:
        res[v] = {leg: {"min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                        "runs_ms": [round(x, 4) for x in t]} for leg, t in runs[v].items()}
    e, b = res["engine"], res["baseline"]
    for leg in ("encode", "fold", "post", "device_ms", "host_ms", "wall_ms"):
        res[f"{leg}_speedup"] = [round(b[leg]["min_ms"] / e[leg]["max_ms"], 2),
                                 round(b[leg]["max_ms"] / e[leg]["min_ms"], 2)]
    print(json.dumps(res), flush=True)
    if same is False:
        raise SystemExit(f"{name}: the engine's and the baseline's states differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ref96,c4_96,c3_16")
    ap.add_argument("--rounds", type=int, default=0, help="0: the shape's own count")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chirp", action="store_true",
                    help="time FftRound(chirp=True) (as 'engine') against FftRound() (as "
                         "'baseline'); their states agree to rounding, not bit for bit")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fft_round needs a ROCm GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    for name in args.shapes.split(","):
        if name not in SHAPES:
            raise SystemExit(f"unknown shape {name}")
        run_shape(args, name, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
