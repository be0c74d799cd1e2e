#!/usr/bin/env python3
"""Time one batched chirp-z call, fused against unfused, on one GPU.

``rfft_chirp_nodes`` and ``irfft_chirp_nodes`` of ``--jobs`` rows of ``--n`` reals, with
``fused=True`` and ``fused=False`` alternated call by call on the same rows and tables: device
events around each call, the median over ``--reps`` calls, ``--runs`` times over.  Prints one JSON
line: the two padded lengths, min-max of the runs' medians per variant and direction, and the
speed-up as the range [unfused min / fused max, unfused max / fused min] (a range that contains 1
is no difference).  Before anything is timed the two forward results are compared (bit for bit
where both run the same padded length and plan; reported as ``rel_diff``).

    python tools/bench_fft_chirp_fused.py --n 11000006 --jobs 96
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=89_834)
    ap.add_argument("--jobs", type=int, default=96)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fft_chirp_fused needs a ROCm GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    n, jobs = args.n, args.jobs
    x = torch.randn(jobs, n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    back = torch.empty_like(x)
    out = {f: torch.zeros(jobs, n // 2 + 1, dtype=torch.complex64, device=dev)
           for f in (True, False)}
    ws = {f: codec.fft_chirp_nodes_workspace(jobs, n, dev, fused=f) for f in (True, False)}
    fwd = {f: codec.FftNodesTable(list(x), None, list(out[f]), False, dev) for f in (True, False)}
    inv = {f: codec.IfftNodesTable(list(out[f]), list(back), dev) for f in (True, False)}
    calls = {"rfft": (codec.rfft_chirp_nodes, fwd), "irfft": (codec.irfft_chirp_nodes, inv)}

    def timed(what, fused):
        call, tabs = calls[what]
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        call(tabs[fused], n, ws[fused], fused=fused)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    for what in calls:  # warm-up: tables, code objects
        for f in (True, False):
            timed(what, f)
    timed("rfft", True), timed("rfft", False)
    diff = float((out[True] - out[False]).abs().max() / out[False].abs().max())
    res = {"n": n, "jobs": jobs, "reps": args.reps, "runs": args.runs,
           "device": torch.cuda.get_device_name(0), "P_fused": codec.fft_chirp_fused_length(n),
           "P_unfused": codec.fft_chirp_length(n), "rel_diff": diff}
    for what in calls:
        med = {True: [], False: []}
        for _ in range(args.runs):
            ts = {True: [], False: []}
            for _ in range(args.reps):
                for f in (True, False):
                    ts[f].append(timed(what, f))
            for f in med:
                med[f].append(round(float(np.median(ts[f])), 1))
        res[f"{what}_fused_us"], res[f"{what}_unfused_us"] = med[True], med[False]
        res[f"{what}_speedup"] = [round(min(med[False]) / max(med[True]), 2),
                                  round(max(med[False]) / min(med[True]), 2)]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
