#!/usr/bin/env python3
"""Time the SubSampling kernels on the GPU against the host alternative they replace.

At n elements (default 2^24) and each alpha: ``codec.mt_mask`` (jump-ahead MT19937 mask),
``codec.mask_gather`` and the 3-payload ``codec.mask_decode_average``, by device events (a
warm-up, then the median of ``--iters`` launches), ``--runs`` times over in one process; and, in
the same process, the alternative: ``torch.rand(n, generator=g) <= alpha`` on the host, packed,
plus the H2D of the packed mask (host clock around work that ends in a synchronise).  Prints one
JSON line.  ``gate``: the slowest mask run beats the fastest host run by more than both spreads;
the tool exits non-zero when it does not.

    python tools/bench_subsampling.py [--n 16777216] [--alphas 0.1,0.5] [--iters 100] [--runs 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from decentralizepy_amd import _lib, codec  # noqa: E402


def event_median_ms(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def host_mask_ms(seed, alpha, n, dev, reps=3):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = torch.Generator()
        g.manual_seed(seed)
        m = (torch.rand(size=(n,), generator=g) <= alpha).numpy()
        words = np.packbits(m, bitorder="little")
        torch.from_numpy(words).to(dev)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--alphas", default="0.1,0.5")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_subsampling needs a ROCm GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    n = args.n
    ws = codec.Workspace(dev)
    x = torch.randn(n, device=dev)
    out = torch.empty_like(x)
    t0 = time.perf_counter()
    L = _lib.lib()
    chunks = -(-n // L.dpz_mt_chunk_elems())
    probe = np.empty(1, np.uint32)  # the last chunk's window builds every table the mask needs
    L.dpz_mt_raw_host(1, (chunks - 1) * L.dpz_mt_chunk_elems(), 1, probe.ctypes.data)
    res = {"n": n, "iters": args.iters, "runs": args.runs,
           "device": torch.cuda.get_device_name(0),
           "table_build_host_ms": (time.perf_counter() - t0) * 1e3, "alphas": {}}
    for alpha in (float(a) for a in args.alphas.split(",")):
        pays = []
        for seed in (11, 12, 13):
            mask, rank_tab, count = codec.mt_mask(seed, alpha, n, dev, workspace=ws)
            k = int(count.item())
            pays.append((mask, rank_tab, torch.randn(max(k, 1), device=dev)[:k]))
        mask, rank_tab, vals = pays[0]
        k = vals.numel()
        ks = [p[2].numel() for p in pays]
        gather_bytes = 4 * n + n / 8 + 4 * k
        fold_bytes = 8 * n + sum(n / 8 + 4 * kk for kk in ks)
        r = {"k": ks, "mask_ms": [], "gather_ms": [], "fold3_ms": [], "host_mask_ms": []}
        m2, r2, c2 = (torch.empty_like(mask), torch.empty_like(rank_tab),
                      torch.empty(1, dtype=torch.int64, device=dev))
        for _ in range(args.runs):
            r["mask_ms"].append(event_median_ms(
                lambda: codec.mt_mask(11, alpha, n, dev, m2, r2, c2, workspace=ws), args.iters))
            r["gather_ms"].append(event_median_ms(
                lambda: codec.mask_gather(x, mask, rank_tab, vals), args.iters))
            r["fold3_ms"].append(event_median_ms(
                lambda: codec.mask_decode_average(x, pays, [0.25] * 3, 0.25, out=out), args.iters))
            r["host_mask_ms"].append(host_mask_ms(11, alpha, n, dev))
        r["gather_GBps"] = gather_bytes / (min(r["gather_ms"]) * 1e-3) / 1e9
        r["fold3_GBps"] = fold_bytes / (min(r["fold3_ms"]) * 1e-3) / 1e9
        spread = (max(r["mask_ms"]) - min(r["mask_ms"])) + \
            (max(r["host_mask_ms"]) - min(r["host_mask_ms"]))
        r["gate"] = bool(min(r["host_mask_ms"]) - max(r["mask_ms"]) > spread)
        res["alphas"][str(alpha)] = r
    print(json.dumps(res))
    failed = [a for a, r in res["alphas"].items() if not r["gate"]]
    if failed:
        raise SystemExit(f"gate failed at alpha {failed}: the mask does not beat the host "
                         "alternative by more than the runs' spread")


if __name__ == "__main__":
    main()
