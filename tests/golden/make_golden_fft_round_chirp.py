#!/usr/bin/env python3
"""Generate the FFT-round fixture of a size WITHOUT a native FFT plan (tests/golden/
fft_round_chirp.json + fft_round_chirp4.npz) from the UNMODIFIED reference
``decentralizepy.sharing.JWINS.FFT.FFT`` (sacs-epfl/decentralizepy), with
``make_golden_fft_round``'s ``run``, ``Retry`` and seed search.  Run in the build container only
(the reference is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fft_round_chirp.py

The run ``chirp4``: one reference ``FFT`` object per node of the 4-node graph with edges (0, 1),
(1, 2), (2, 3), (1, 3) (degrees 1, 3, 2, 2), N = 8,198 = 2 * 4,099 (4,099 is prime and above the
native passes' largest radix), shape (90, 90, 98), k = 410, ``accumulation`` with
``accumulate_averaging_changes``, 2 rounds, seeds from 74.  The same arrays, assertions (every k-th
key at least MIN_GAP from the next, no -0.0, all finite, the file under 1,000,000 bytes) and
storage of ``acc_enc`` as the existing generator's.
"""
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import make_golden_fft_round as mfr  # noqa: E402  (the reference's FFT class, run, Retry)

ops, mg, Graph = mfr.ops, mfr.mg, mfr.Graph
EDGES = [[0, 1], [1, 2], [2, 3], [1, 3]]


def main():
    mg.torch.set_num_threads(4)
    g = Graph(4)
    for a, b in EDGES:
        g.adj_list[a].add(b)
        g.adj_list[b].add(a)
    assert [len(g.neighbors(u)) for u in range(4)] == [1, 3, 2, 2]
    meta = dict(name="chirp4", edges=EDGES, rounds=2, accumulation=True,
                accumulate_averaging_changes=True)
    for seed in range(74, 74 + 4000, 10):
        try:
            arrays = mfr.run(meta, g, (90, 90, 98), seed)
            break
        except mfr.Retry as e:
            print("retry:", meta["name"], seed, e, flush=True)
    else:
        raise SystemExit("no well-separated seed")
    assert meta["min_gap"] >= ops.MIN_GAP and (meta["n"], meta["k"]) == (8198, 410)
    path = os.path.join(OUT, "fft_round_chirp4.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(meta["name"], meta["n"], meta["m_len"], meta["k"], meta["seed"], meta["min_gap"], size,
          "bytes", flush=True)
    assert size < 1_000_000
    with open(os.path.join(OUT, "fft_round_chirp.json"), "w") as f:
        json.dump({"numpy": np.__version__, "torch": mg.torch.__version__,
                   "reference": "sacs-epfl/decentralizepy v1", "runs": [meta]}, f, indent=1)


if __name__ == "__main__":
    main()
