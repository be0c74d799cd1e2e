#!/usr/bin/env python3
"""Generate tests/golden/elias_edges.npz + elias_edges.json from the UNMODIFIED reference.

Run in the build container only (the reference is not present on the GPU box); no test runs it:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_elias_edges.py

It imports sacs-epfl/decentralizepy's ``Elias`` from /root/reference/src (as make_golden.py does)
and runs ``Elias().compress`` / ``.decompress`` on the structural edge cases of
tests/codec_edges.py: stream lengths on the decode-chunk and super-map edges, codes straddling a
chunk edge, encode blocks that end in mid-word, gaps on both sides of every power of two.

* small cases (L <= 70 000 code bits): ``<name>_input`` (int32), ``<name>_bytes`` (uint8, what
  compress returned) and ``<name>_decoded`` (int64, what decompress returned) in the .npz.  Runs
  of consecutive integers deflate badly, so where a case has more than DIGEST_ABOVE values (the
  three ``ones`` cases around 2^16) the input and the decode go into the .json as sha256 of
  their bytes instead, which keeps the .npz under 300 KB; the bytes are stored in full;
* large cases (L around 2^20): only the sha256 of the reference's bytes, their length and the
  value count, in the .json.
"""
import hashlib
import json
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference/src"
OUT = os.path.dirname(os.path.abspath(__file__))

DIGEST_ABOVE = 20_000

sys.path.insert(0, REF)
from decentralizepy.compression.Elias import Elias  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from tests import codec_edges as ce  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    arrays, small = {}, []
    for name, idx in ce.golden_small_cases().items():
        enc = np.asarray(Elias().compress(idx.copy()), dtype=np.uint8)  # compress sorts in place
        dec = np.asarray(Elias().decompress(enc.copy()))
        assert dec.dtype == np.int64
        rec = {"name": name, "k": int(idx.size), "nbytes": int(enc.size)}
        arrays[f"{name}_bytes"] = enc
        if idx.size > DIGEST_ABOVE:
            rec["input_sha256"] = sha(idx)
            rec["decoded_sha256"] = sha(dec)
            rec["decoded_count"] = int(dec.size)
        else:
            arrays[f"{name}_input"] = idx
            arrays[f"{name}_decoded"] = dec
        small.append(rec)
    large = []
    for name, idx in ce.golden_large_cases().items():
        enc = np.asarray(Elias().compress(idx.copy()), dtype=np.uint8)
        large.append({"name": name, "k": int(idx.size), "nbytes": int(enc.size),
                      "sha256": sha(enc)})
    path = os.path.join(OUT, "elias_edges.npz")
    np.savez_compressed(path, **arrays)
    with open(os.path.join(OUT, "elias_edges.json"), "w") as f:
        json.dump({"small": small, "large": large,
                   "generator": "tests/golden/make_golden_elias_edges.py",
                   "reference": "sacs-epfl/decentralizepy v1 (/root/reference/src)",
                   "numpy": np.__version__}, f, indent=1)
    print("wrote", len(small), "small and", len(large), "large cases,",
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
