#!/usr/bin/env python3
"""Time the legs of a whole-topology top-k round with accumulated changes on one GPU.

Shape: the 96 nodes of ``96_regular.edges`` on one rank (no collective is part of the timing),
N = 11,000,000, alpha in {0.01, 0.1}, both accumulation modes (``--edges``, ``--n``, ``--alphas``,
``--modes``; ``--shape sw96``: ``96_nodes_smallworld.edges``, 3 to 10 neighbours per node, at
N = 89,834, the shape of the same name of ``bench_jwins_round.py``).  The state is 5 x nodes x 4 N bytes per variant (x, x0, acc, counter, the fold's
output); it is checked against the free HBM before anything is allocated.

Two variants of the same round, alternated round by round in one process, from the same models
and the same seeded "training" step between rounds, so their states stay equal in every bit
(checked after the first two rounds, before anything is timed, and after the last round):

  engine     ``gossip_topkacc.TopKAccRound.step``: the ``dpz_topkacc_encode_nodes`` launch set for
             all nodes, the status words' copy (the exchange on one rank), the batched one-launch
             fold, in mode "avg" ONE ``dpz_topkacc_post_nodes`` launch;
  baseline   the per-node device call sequence of the plugin ``sharing/PartialModel.py``, node
             after node: ``topk_encode`` with the accumulator (its own choice of path, completed
             per call, ``hint`` and ``keep_x`` as the plugin passes them), ``decode_average`` over
             the neighbours' payloads into a fresh row, and in mode "avg" the accumulate-only
             ``topk_encode(new, 0, x0=prev, acc=...)``.  The plugin's host round trips (the model
             goes through the state_dict every round) are NOT part of it: the averaged model is
             copied over the baseline's model outside the timed legs.  The baseline's encode
             updates its counter in the call, as the engine's does; the plugin defers that to a
             ring of index lists.

Device events per leg (through the ``mark`` of either ``step``), ``--warmup`` untimed rounds, the
median over ``--rounds`` rounds, ``--runs`` times over; the range over the runs is reported, and a
leg's speed-up as the range [baseline min / engine max, baseline max / engine min].  Rates are over
the ENGINE's algorithmic bytes per node, k = round(alpha N):
  encode     the first pass reads x, x0, acc and writes the key row (16 N), four passes read the
             key row (16 N): 32 N, plus per entry idx and val written, x read, the counter read
             and written, acc written (24 k; the scattered part moves in 32-byte sectors);
  post       x, x0, acc read and acc written: 16 N.
``copy_tb_per_s`` is a device-to-device copy of 1 GiB timed in the same process.  Prints one JSON
line per (alpha, mode).

    python tools/bench_topkacc_round.py [--n 11000000] [--alphas 0.01,0.1] [--modes acc,avg] [--shape sw96]
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
from decentralizepy_amd.gossip_topkacc import TopKAccRound  # noqa: E402


class Baseline:
    """The same round through the per-node plugin's device calls (sharing/PartialModel.py)."""

    def __init__(self, adj, x_init, alpha, avg):
        m, n = x_init.shape
        self.m, self.n, self.k, self.avg = m, n, round(alpha * n), avg
        self.mode = codec.DPZ_ACC_ADD if avg else codec.DPZ_ACC_ACCUMULATE
        self.x = [x_init[u].clone() for u in range(m)]
        self.x0 = [x_init[u].clone() for u in range(m)]
        self.out = [torch.empty_like(self.x[0]) for _ in range(m)]
        self.acc = [torch.zeros_like(self.x[0]) for _ in range(m)]
        i32 = dict(dtype=torch.int32, device=x_init.device)
        self.counter = [torch.zeros(n, **i32) for _ in range(m)]
        self.pi = [torch.empty(self.k, **i32) for _ in range(m)]
        self.pv = [torch.empty(self.k, device=x_init.device) for _ in range(m)]
        self.weights = [mh_weights(adj, u) for u in range(m)]
        self.ws = codec.Workspace(x_init.device)

    def step(self, mark):
        k, ws = self.k, self.ws
        for u in range(self.m):  # get_data_to_send
            codec.topk_encode(self.x[u], k, x0=self.x0[u], acc=self.acc[u], acc_mode=self.mode,
                              counter=self.counter[u], idx_out=self.pi[u], val_out=self.pv[u],
                              workspace=ws, hint=True, keep_x=True)
        mark("encode")
        for u, (nbrs, w, w_self) in enumerate(self.weights):  # _averaging
            codec.decode_average(self.x[u], [(self.pi[q], self.pv[q]) for q in nbrs], w, w_self,
                                 out=self.out[u], workspace=ws)
        mark("fold")
        if self.avg:  # _post_step
            for u in range(self.m):
                codec.topk_encode(self.out[u], 0, x0=self.x0[u], acc=self.acc[u],
                                  acc_mode=codec.DPZ_ACC_ACCUMULATE, workspace=ws)
            mark("post")
        self.x0, self.out = self.out, self.x0  # init_model = the averaged model

    def load_model(self):
        """The averaged model becomes the model (the plugin's load_state_dict; not timed)."""
        for u in range(self.m):
            self.x[u].copy_(self.x0[u])


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

    obj.step(mark=mark)
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


def eq(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_state(eng, base, payloads=True):
    ok = True
    for u in range(base.m):
        ok = ok and eq(eng.x0[u], base.x0[u]) and eq(eng.acc[u], base.acc[u])
        ok = ok and torch.equal(eng.counter[u], base.counter[u])
        if payloads:
            idx, vals = eng.payload(u)
            ok = ok and torch.equal(idx, base.pi[u]) and eq(vals, base.pv[u])
    return bool(ok)


def run_config(args, adj, dev, alpha, avg, copy):
    m, n = len(adj), args.n
    gen = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.randn(m, n, device=dev, generator=gen)
    noise = torch.randn(n, device=dev, generator=gen)  # the "training" step, rolled per node
    eng = TopKAccRound(adj, x0, alpha, accumulate_averaging_changes=avg)
    base = Baseline(adj, x0, alpha, avg)
    del x0
    variants = {"engine": eng, "baseline": base}

    def train(r):
        base.load_model()
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
    equal_after_two = same_state(eng, base)
    if not equal_after_two:
        raise SystemExit(f"alpha {alpha} avg {avg}: the engine's and the baseline's states differ "
                         "after two rounds; nothing was timed")
    for _ in range(args.warmup):
        train(r)
        for obj in variants.values():
            timed_round(obj)
        r += 1
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
    torch.cuda.synchronize()
    same = same_state(eng, base)
    k = eng.k
    bytes_of = {"encode": (32 * n + 24 * k) * m, "post": 16 * n * m}
    res = {"device": torch.cuda.get_device_name(0), "nodes": m, "n": n, "alpha": alpha,
           "mode": "avg" if avg else "acc", "k": k, "rounds": args.rounds, "runs": args.runs,
           "warmup": args.warmup + 2, "total_rounds": r, "equal_after_two_rounds": equal_after_two,
           "results_equal": same, "copy_tb_per_s": round(copy, 3), "bytes": bytes_of}
    for name in variants:
        res[name] = {}
        for leg, t in runs[name].items():
            res[name][leg] = {"min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                              "runs_ms": [round(v, 4) for v in t]}
            if name == "engine" and leg in bytes_of:
                res[name][leg]["tb_per_s"] = [round(bytes_of[leg] / (v * 1e-3) / 1e12, 3)
                                              for v in (max(t), min(t))]
                res[name][leg]["of_copy_rate"] = [round(bytes_of[leg] / (v * 1e-3) / 1e12 / copy, 3)
                                                  for v in (max(t), min(t))]
        res[name]["round_ms"] = [round(sum(res[name][leg][key] for leg in runs[name]), 4)
                                 for key in ("min_ms", "max_ms")]
    for leg in runs["baseline"]:
        e, b = res["engine"][leg], res["baseline"][leg]
        res[f"{leg}_speedup"] = [round(b["min_ms"] / e["max_ms"], 2),
                                 round(b["max_ms"] / e["min_ms"], 2)]
    e, b = res["engine"]["round_ms"], res["baseline"]["round_ms"]
    res["round_speedup"] = [round(b[0] / e[1], 2), round(b[1] / e[0], 2)]
    print(json.dumps(res), flush=True)
    if not same:
        raise SystemExit("the engine's and the baseline's states differ")


SHAPES = {"sw96": ("96_nodes_smallworld.edges", 89_834)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=11_000_000)
    ap.add_argument("--alphas", default="0.01,0.1")
    ap.add_argument("--modes", default="acc,avg")
    ap.add_argument("--edges", default=os.path.join(ROOT, "tests", "golden", "96_regular.edges"))
    ap.add_argument("--nodes", type=int, default=0,
                    help="keep only the first NODES nodes of the graph (0: all); lower it if the "
                         "state does not fit the device")
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None,
                    help="a named (edges, n) pair instead of --edges and --n")
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.shape:
        args.edges, args.n = os.path.join(ROOT, "tests", "golden", SHAPES[args.shape][0]), \
            SHAPES[args.shape][1]
    if not torch.cuda.is_available():
        raise SystemExit("bench_topkacc_round needs a ROCm GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    adj = read_edges(args.edges)
    if args.nodes:
        adj = [{q for q in s if q < args.nodes} for s in adj[:args.nodes]]
    m, n = len(adj), args.n
    # both variants' five rows per node, the initial models while both are built, payloads and
    # temporaries, the 2 GiB of the copy-rate probe
    need = (2 * 5 * m + m + 16) * 4 * n + (2 << 30)
    free, _ = torch.cuda.mem_get_info(dev)
    if need > 0.9 * free:
        raise SystemExit(f"the state needs {need / 2**30:.1f} GiB, {free / 2**30:.1f} GiB of HBM "
                         "are free: lower --nodes or --n")
    copy = copy_rate(dev)
    for alpha in [float(a) for a in args.alphas.split(",")]:
        for mode in args.modes.split(","):
            if mode not in ("acc", "avg"):
                raise SystemExit(f"unknown mode {mode}")
            run_config(args, adj, dev, alpha, mode == "avg", copy)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
