#!/usr/bin/env python3
"""Time the quantiser's kernels on the GPU against ``pack_fp16``, the value packer already in
the tree, at the same n in the same run.

Per shape (default n = 167,772 — 1 % of the 64 MiB tensor — and n = 16,777,216) and per run:
a warm-up, then ``--iters`` rounds of ``codec.quant_encode`` (k = 32767, so 16 bits per value),
``codec.quant_decode`` and ``codec.pack_fp16`` under ``codec.KernelTimer`` (the library's event
pair around each launch), ``--runs`` runs in one process.  Reported per run: the mean device time
per launch of the statistics pass, the pack pass, the unpack kernel and pack_fp16, the ratio
(stats + pack) / pack_fp16, and GiB/s over the bytes each moves (encode 4N + 4N + 2N, pack_fp16
4N + 2N, decode 2N + 4N).  ``--cache-n`` adds a shape past the 256 MiB Infinity Cache: the pack
pass's rate there against its rate at the 64 MiB tensor says whether the second read of x is
served by that cache.  Reads no reference files.  Prints one JSON line (``--out`` also writes it).

    python tools/quant_probe.py [--shapes 167772,16777216] [--iters 50] [--runs 3]
                                [--cache-n 134217728] [--out profiles/quant_probe.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from decentralizepy_amd import codec  # noqa: E402

K = 32767
GIB = float(2 ** 30)


def one_run(x, ws, half, out, iters, warmup):
    n = x.numel()

    def round_():
        body, info = codec.quant_encode(x, K, workspace=ws)
        codec.quant_decode(body, n, info.w, info.scale, out=out)
        codec.pack_fp16(x, out=half)
        return info

    for _ in range(warmup):
        info = round_()
    torch.cuda.synchronize()
    assert info.w == 16, info.w
    with codec.KernelTimer() as t:
        for _ in range(iters):
            round_()
        torch.cuda.synchronize()
    us = {name: 1e3 * ms / cnt for name, (ms, cnt) in t.result.items()}
    for name in ("quant_stats", "quant_pack", "quant_unpack", "fp16"):
        assert t.result[name][1] == iters, (name, t.result[name])
    enc = us["quant_stats"] + us["quant_pack"]

    def rate(nbytes, t_us):
        return nbytes / (t_us * 1e-6) / GIB

    return {"stats_us": us["quant_stats"], "pack_us": us["quant_pack"],
            "unpack_us": us["quant_unpack"], "fp16_us": us["fp16"], "encode_us": enc,
            "ratio_encode_over_fp16": enc / us["fp16"],
            "encode_GiBps": rate(10 * n, enc), "stats_GiBps": rate(4 * n, us["quant_stats"]),
            "pack_GiBps": rate(6 * n, us["quant_pack"]), "fp16_GiBps": rate(6 * n, us["fp16"]),
            "decode_GiBps": rate(6 * n, us["quant_unpack"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="167772,16777216")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cache-n", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quant_probe needs a ROCm GPU; there is no CPU path")
    if args.iters < 50 or args.runs < 3:
        raise SystemExit("the protocol wants at least 50 timed launches and three runs")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "k": K, "iters": args.iters,
           "warmup": args.warmup, "runs": args.runs, "shapes": {}}
    shapes = [int(s) for s in args.shapes.split(",")] + ([args.cache_n] if args.cache_n else [])
    for n in shapes:
        g = torch.Generator(device=dev).manual_seed(n)
        x = 0.01 * torch.randn(n, device=dev, generator=g)
        ws = codec.Workspace(dev)
        half = torch.empty(n, dtype=torch.float16, device=dev)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        runs = [one_run(x, ws, half, out, args.iters, args.warmup) for _ in range(args.runs)]
        ratios = [r["ratio_encode_over_fp16"] for r in runs]
        res["shapes"][str(n)] = {
            "runs": runs, "ratio_min": min(ratios), "ratio_max": max(ratios),
            "ratio_spread": max(ratios) - min(ratios), "traffic_ratio": 10 / 6,
            "over_traffic_by_more_than_spread":
                bool(min(ratios) - 10 / 6 > max(ratios) - min(ratios))}
        del x, half, out, ws
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
