#!/usr/bin/env python3
"""Time the legs of a whole-federation STC round on one GPU.

Shape: 96 clients and the server on one rank (no exchange is part of the timing), N = 11,000,000,
alpha = 0.01, everyone works (``--clients``, ``--n``, ``--alpha``).  The state is 3 x clients x 4 N
bytes per variant (x, prev_model, residuals) plus the server's rows and the baseline's N-length
temporaries; it is checked against the free HBM before anything is allocated.

Two variants of the same round, alternated round by round in one process, from the same models
and the same seeded "training" step between rounds, so their states stay equal in every bit
(checked after the last round):

  engine     ``gossip_stc.StcRound.step``: the ``dpz_stc_encode_nodes`` launch set for all
             clients, ONE ``dpz_stc_server_fold`` launch, the encode launch set in server form,
             ONE ``dpz_stc_apply_nodes`` launch;
  baseline   the per-node device call sequence of the plugin ``sharing/STC.py``: per client
             ``topk_encode`` with the residual accumulator (the sampled path, completed per call)
             and ``replace`` (model_change); on the server the zero-based ``decode_average`` over
             all payloads and the dense ``[1.0], 1.0`` add, ``topk_encode`` of the change, a
             ``clone`` and ``scatter_fill``; per client and for the server the add-only
             ``decode_average`` into an N-length copy.  The plugin's host round trips (the model
             goes through the state_dict every call) are NOT part of it; ``prev_model = flat`` is
             a device-to-device copy here, where the plugin keeps the fresh upload.

Device events per leg (through the ``mark`` of either ``step``), ``--warmup`` untimed rounds, the
median over ``--rounds`` rounds, ``--runs`` times over; the range over the runs is reported.
Rates are over each leg's algorithmic bytes of the ENGINE, C = clients, k = round(alpha N):
  encode     the first pass reads x, prev, r and writes r, prev (20 N), four passes read r (16 N):
             36 N per client, plus 12 k per client written (idx, val, the cleared residuals);
  fold       r_s read and written once (8 N) plus 8 k per payload read;
  broadcast  five passes over r_s (20 N) plus 12 k written;
  apply      per target the row (8 k) and a read-modify-write of k scattered floats (8 k): the
             useful bytes; the traffic is in 32-byte sectors.
``copy_tb_per_s`` is a device-to-device copy of 1 GiB timed in the same process.  Prints one JSON
line.

    python tools/bench_stc_round.py [--n 11000000] [--alpha 0.01] [--clients 96]
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
from decentralizepy_amd.gossip_stc import StcRound  # noqa: E402

LEGS = ("encode", "fold", "broadcast", "apply")


class Baseline:
    """The same round through the per-node plugin's device calls (sharing/STC.py)."""

    def __init__(self, x_init, server_init, alpha):
        m, n = x_init.shape
        self.m, self.n, self.k = m, n, round(alpha * n)
        self.x = [x_init[u].clone() for u in range(m)]
        self.prev = [x_init[u].clone() for u in range(m)]
        self.r = [torch.zeros_like(self.x[0]) for _ in range(m)]
        self.server_x = server_init.clone()
        self.server_r = torch.zeros_like(self.server_x)
        self.tmp = torch.empty_like(self.server_x)
        self.total = torch.empty_like(self.server_x)
        self.change = torch.empty_like(self.server_x)
        i32 = dict(dtype=torch.int32, device=x_init.device)
        self.pi = [torch.empty(self.k, **i32) for _ in range(m)]
        self.pv = [torch.empty(self.k, device=x_init.device) for _ in range(m)]
        self.ws = codec.Workspace(x_init.device)
        self.bcast = None

    def step(self, mark):
        k, ws = self.k, self.ws
        for u in range(self.m):  # get_data_to_send
            codec.topk_encode(self.x[u], k, x0=self.prev[u], acc=self.r[u],
                              acc_mode=codec.DPZ_ACC_ACCUMULATE, vals_src=self.r[u],
                              idx_out=self.pi[u], val_out=self.pv[u], workspace=ws)
            self.prev[u].copy_(self.x[u])
            codec.replace(self.r[u], self.pi[u], self.pv[u], out=self.tmp, workspace=ws)
        mark("encode")
        w = 1.0 / self.m  # _averaging_server
        codec.decode_average(self.server_r, list(zip(self.pi, self.pv)), [w] * self.m, None,
                             out=self.total, zero_base=True, workspace=ws)
        codec.decode_average(self.server_r, [(None, self.total)], [1.0], 1.0, out=self.change,
                             workspace=ws)
        mark("fold")
        bi, bv = codec.topk_encode(self.change, k, vals_src=self.change, workspace=ws)
        res = self.change.clone()  # server_broadcast
        codec.scatter_fill(res, bi, 0.0)
        self.server_r = res
        self.bcast = (bi, bv)
        mark("broadcast")
        for u in range(self.m):  # process_received
            out = codec.decode_average(self.x[u], [(bi, bv)], add_only=True, out=self.tmp,
                                       workspace=ws)
            self.x[u], self.tmp = out, self.x[u]
        out = codec.decode_average(self.server_x, [(bi, bv)], add_only=True, out=self.tmp,
                                   workspace=ws)
        self.server_x, self.tmp = out, self.server_x
        mark("apply")


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
    return {leg: evs[i].elapsed_time(evs[i + 1]) for i, leg in enumerate(names) if leg in LEGS}


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
    ap.add_argument("--clients", type=int, default=96,
                    help="lower it if the state does not fit the device")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stc_round needs a ROCm GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    m, n = args.clients, args.n
    # both variants' x, prev, r, the initial models while both are built, the server rows and
    # temporaries, the 2 GiB of the copy-rate probe
    need = (2 * 3 * m + m + 16) * 4 * n + (2 << 30)
    free, _ = torch.cuda.mem_get_info(dev)
    if need > 0.9 * free:
        raise SystemExit(f"the state needs {need / 2**30:.1f} GiB, {free / 2**30:.1f} GiB of HBM "
                         "are free: lower --clients or --n")
    gen = torch.Generator(device=dev).manual_seed(1)
    x0 = torch.randn(m, n, device=dev, generator=gen)
    xs0 = torch.randn(n, device=dev, generator=gen)
    noise = torch.randn(n, device=dev, generator=gen)  # the "training" step, rolled per client
    eng = StcRound(m, x0, xs0, args.alpha)
    base = Baseline(x0, xs0, args.alpha)
    del x0, xs0
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

    def eq(a, b):
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))

    same = all(eq(eng.x[u], base.x[u]) and eq(eng.prev[u], base.prev[u])
               and eq(eng.r[u], base.r[u]) for u in range(m))
    same = same and eq(eng.server_x, base.server_x) and eq(eng.server_r, base.server_r)
    bi, bv = eng.broadcast()
    same = same and torch.equal(bi, base.bcast[0]) and eq(bv, base.bcast[1])
    k = eng.k
    bytes_of = {"encode": (36 * n + 12 * k) * m, "fold": 8 * n + 8 * k * m,
                "broadcast": 20 * n + 12 * k, "apply": 16 * k * (m + 1)}
    copy = copy_rate(dev)
    res = {"device": torch.cuda.get_device_name(0), "clients": m, "n": n, "alpha": args.alpha,
           "k": k, "rounds": args.rounds, "runs": args.runs, "warmup": args.warmup,
           "results_equal": bool(same), "copy_tb_per_s": round(copy, 3), "bytes": bytes_of}
    for name in variants:
        res[name] = {}
        for leg, t in runs[name].items():
            res[name][leg] = {"min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                              "runs_ms": [round(v, 4) for v in t]}
            if name == "engine":
                res[name][leg]["tb_per_s"] = [round(bytes_of[leg] / (v * 1e-3) / 1e12, 3)
                                              for v in (max(t), min(t))]
                res[name][leg]["of_copy_rate"] = [round(bytes_of[leg] / (v * 1e-3) / 1e12 / copy, 3)
                                                  for v in (max(t), min(t))]
        res[name]["round_ms"] = [round(sum(res[name][leg][key] for leg in LEGS), 4)
                                 for key in ("min_ms", "max_ms")]
    for leg in LEGS:
        e, b = res["engine"][leg], res["baseline"][leg]
        res[f"{leg}_speedup"] = [round(b["min_ms"] / e["max_ms"], 2),
                                 round(b["max_ms"] / e["min_ms"], 2)]
    print(json.dumps(res))
    if not same:
        raise SystemExit("the engine's and the baseline's states differ")


if __name__ == "__main__":
    main()
