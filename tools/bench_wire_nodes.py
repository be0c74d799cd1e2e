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

``--decode`` times the receiving half instead, over the streams one ``dpz_wire_encode_nodes`` call
wrote for the round's payloads (``--precision``: the engines' ``float_precision``):
  batched  ONE ``dpz_wire_decode_nodes`` call over all nodes: three launches, the stream lengths
           and the trailers read on the device;
  loop     node by node ``codec.elias_decode_async`` + ``codec.fpz_decode``: a memset, three
           launches and a check kernel for the indices and one launch for the values.  The loop is
           handed every stream's length, ``nbits`` and ``first`` from a host copy made BEFORE the
           timer starts (a receiver of device-resident rows would pay a read-back per node for
           them), so it is timed without any host synchronisation of its own.
The two outputs are compared bit for bit in every round.

    python tools/bench_wire_nodes.py [--shapes sw96,reg96] [--rounds 10] [--runs 3]
                                     [--decode] [--precision 0]
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
    alpha = args.alpha or 0.01
    eng = JwinsBatchRound(adj, x0, TUTORIAL_ALPHAS, float_precision=args.precision) \
        if name == "sw96" and not args.alpha else \
        TopKAccRound(adj, x0, alpha, float_precision=args.precision)
    del x0
    ws = codec.Workspace(dev)
    if args.decode:
        return run_decode(name, args, eng, noise, ws)

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


def run_decode(name, args, eng, noise, ws):
    dev, m, prec = eng.device, eng.m, eng.float_precision
    runs, launches = {}, {}
    for run in range(-1, args.runs):
        ts = {}
        for r in range(args.warmup if run < 0 else args.rounds):
            for u in range(m):
                eng.x[u].add_(torch.roll(noise, 7919 * (u + 1) + r), alpha=0.01)
            eng.step()
            sizes, status, buf, offs = eng._wire_call(True)
            views = eng._wire_views()[1]
            counts = [v.numel() for _, v in views]
            out_i = [torch.empty(c, dtype=torch.int32, device=dev) for c in counts]
            out_v = [torch.empty(c, dtype=torch.float32, device=dev) for c in counts]
            loop_v = [torch.empty(c, dtype=torch.float32, device=dev) for c in counts]
            tab = codec.WireDecodeTable(m, dev)
            base, hs, hbuf = buf.data_ptr(), sizes.tolist(), buf.cpu().numpy()
            ends = [o[0] if o[0] is not None else o[1] for o in offs[1:]] + [buf.numel()]
            for j, ((oi, ov), (idx, _)) in enumerate(zip(offs, views)):
                tab.set(j, None if oi is None else base + oi, base + ov, counts[j],
                        None if oi is None else out_i[j], out_v[j], sizes[j],
                        0 if oi is None else ov - oi, ends[j] - ov)
            tab.upload()
            st = torch.zeros(m, dtype=torch.int32, device=dev)
            lst = torch.zeros(1, dtype=torch.int32, device=dev)
            dws = codec.wire_decode_workspace(
                m, max(0 if oi is None else ov - oi for oi, ov in offs), max(counts), dev)
            trailers = [None if oi is None else tuple(
                int(v) for v in hbuf[oi + hs[j][0] - 16:oi + hs[j][0]].view("<i8"))
                for j, (oi, _) in enumerate(offs)]

            def batched():
                codec.wire_decode_nodes(tab, st, prec, dws)

            def loop():
                res = []
                for j, (oi, ov) in enumerate(offs):
                    if oi is not None:
                        first, nbits = trailers[j]
                        res.append(codec.elias_decode_async(buf[oi:ov], hs[j][0], nbits, first,
                                                            counts[j], lst, workspace=ws))
                    else:
                        res.append(None)
                    codec.fpz_decode(buf[ov:ov + hs[j][1]], counts[j], prec, out=loop_v[j],
                                     status=lst)
                return res

            ts.setdefault("batched", []).append(wall(batched)[0])
            t, loop_i = wall(loop)
            ts.setdefault("loop", []).append(t)
            same = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                       for a, b in zip(out_v, loop_v))
            same = same and all(li is None or torch.equal(li, a) for li, a in zip(loop_i, out_i))
            if not same or int(st.any()) or int(lst.any()):
                raise SystemExit(f"{name}: the batched decode differs from the loop's")
            if prec == 0 and not all(
                    torch.equal(v.view(torch.int32), o.view(torch.int32)) and
                    (i is None or torch.equal(i, oi_)) for (i, v), o, oi_ in zip(views, out_v, out_i)):
                raise SystemExit(f"{name}: the decoded payloads differ from the encoded ones")
        if run >= 0:
            for leg, v in ts.items():
                runs.setdefault(leg, []).append(float(np.median(v)))
    res = {"device": torch.cuda.get_device_name(0), "bench": "decode", "shape": name, "nodes": m,
           "n": eng.N if hasattr(eng, "N") else None, "precision": prec,
           "alpha": args.alpha or None, "rounds": args.rounds, "runs": args.runs,
           "warmup": args.warmup, "wire_bytes_last_round": int(sizes.sum()),
           "raw_bytes_last_round": int(sum(8 * c if i is not None else 4 * c
                                           for c, (i, _) in zip(counts, views)))}
    for leg, v in runs.items():
        res[leg] = {"min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    res["loop_over_batched"] = [round(res["loop"]["min_ms"] / res["batched"]["max_ms"], 2),
                                round(res["loop"]["max_ms"] / res["batched"]["min_ms"], 2)]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="sw96,reg96")
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--decode", action="store_true",
                    help="time the batched decode against the node-by-node decode loop")
    ap.add_argument("--precision", type=int, default=0, help="the engines' float_precision")
    ap.add_argument("--alpha", type=float, default=0.0,
                    help="TopKAccRound at this alpha for every shape (0: the shapes' own engines)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wire_nodes needs a ROCm GPU; there is no CPU path")
    for name in args.shapes.split(","):
        run_shape(name, args, torch.device("cuda:0"))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
