#!/usr/bin/env python3
"""Generate the quantiser's golden fixtures (tests/golden/quantization.json + quantization_*.npz)
from the UNMODIFIED reference (sacs-epfl/decentralizepy): ``compression/Quantization.py``,
``compression/EliasQuantization.py``, ``sharing/Sharing.py``, ``sharing/PartialModel.py`` and
``sharing/PlainAverageSharing.py``.  Run in the build container only (the reference is not on the
GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_quantization.py

Codec cases: the reference's ``compress_float`` / ``decompress_float`` on inputs from a recorded
recipe (tests/quantization_ops.py:case_input) — float_precision k in KS crossed with n in NS on
0.01 * N(0, 1) data, a ties case, a division case (a reciprocal multiply would change a value), a
tiny case (subnormal norm), a mixed-magnitude case (the chunked summation order shows) and one
n = 200,003 case.  Cases up to n = 20,001 store every array; the larger ones only the header, the
scale bits and SHA-256 of the body and of the decoded values.  The json records the numpy version
the reference ran under: the scale depends on numpy's summation order.

Plugin runs: one reference node with its neighbours' messages, two rounds each — Sharing with
Quantization (n = 20,001 and n = 2001), PartialModel (alpha = 0.1) with EliasQuantization,
PlainAverageSharing uncompressed with 2 and with 6 neighbours and with Quantization.  Recorded:
the node's wire dict with its params unpickled, the neighbours' wire values as reference nodes
sent them, and the model after averaging.
"""
import json
import os
import pickle
import sys
import tempfile
from collections import OrderedDict, deque

import numpy as np

sys.dont_write_bytecode = True
REF = "/root/reference/src"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
import torch  # noqa: E402

from decentralizepy.compression.Quantization import Quantization  # noqa: E402
from decentralizepy.mappings.Linear import Linear  # noqa: E402
from decentralizepy.models.Model import Model  # noqa: E402
from decentralizepy.sharing.PartialModel import PartialModel  # noqa: E402
from decentralizepy.sharing.PlainAverageSharing import PlainAverageSharing  # noqa: E402
from decentralizepy.sharing.Sharing import Sharing  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from oracle import topk as otopk  # noqa: E402  (tie check only)
from tests import quantization_ops as ops  # noqa: E402  (recipes, sha and the asserted properties)

f32 = np.float32
STORE_MAX = 20001


# ---- codec cases ------------------------------------------------------------------------------
def run_case(case):
    x = ops.case_input(case)
    assert x.dtype == f32 and x.size == case["n"]
    blob = Quantization(case["k"]).compress_float(x.copy())
    scale, to_send = pickle.loads(blob)
    assert isinstance(scale, np.float32) and to_send.dtype == np.uint8
    out = Quantization(case["k"]).decompress_float(blob)
    assert out.dtype == f32 and out.shape == (case["n"],)
    case.update(w=int(to_send[1]), padding=int(to_send[0]), scale_bits=ops.bits_of(scale),
                body_sha=ops.sha(to_send[2:]), out_sha=ops.sha(out))
    return x, to_send, out


def division_seed(k, n):
    """A seed whose data shows the division: x * fl(1 / norm) rounds some value differently."""
    for seed in range(3000, 3100):
        x = ops.recipe(seed, n, 0.01)
        norm = ops.params(x, k)[1]
        if np.any(np.rint(x * f32(f32(1) / norm)) != np.rint(x / norm)):
            return seed
    raise RuntimeError("no seed shows the division")


def mixed_seed(n):
    """A seed whose data shows the chunking: one whole-array pairwise tree gives another sum."""
    for seed in range(4000, 4100):
        a = np.abs(ops.mixed(seed, n))
        assert ops.abs_sum(a) == a.sum()
        if ops.pairwise(a) != ops.abs_sum(a):
            return seed
    raise RuntimeError("no seed shows the chunked order")


def codec_cases():
    cases = []
    for ki, k in enumerate(ops.KS):
        for ni, n in enumerate(ops.NS):
            cases.append(dict(name=f"k{k}_n{n}", kind="normal", seed=1000 + 10 * ki + ni, k=k,
                              n=n, file=f"quantization_k{k}.npz"))
    sp = "quantization_special.npz"
    cases.append(dict(name="ties", kind="ties", seed=0, k=255, n=511, file=sp))
    cases.append(dict(name="division", kind="normal", seed=division_seed(2 ** 20, 20001),
                      k=2 ** 20, n=20001, file=sp))
    cases.append(dict(name="tiny", kind="tiny", seed=5, k=255, n=1000, file=sp))
    n_mixed = 3 * 8192 + 4099
    cases.append(dict(name="mixed", kind="mixed", seed=mixed_seed(n_mixed), k=32767, n=n_mixed))
    cases.append(dict(name="large", kind="normal", seed=2000, k=32767, n=200003))
    files = {}
    for case in cases:
        x, to_send, out = run_case(case)
        if case["name"] == "ties":  # norm is exactly 2^-10 and every quantised value is even
            assert ops.params(x, 255)[1] == f32(2.0 ** -10)
            assert np.all(ops.quantise(x[:-1], 2.0 ** -10) % 2 == 0)
        if case["name"] == "tiny":
            assert 0 < ops.params(x, 255)[1] < np.finfo(f32).tiny
        if "file" in case:
            assert case["n"] <= STORE_MAX
            z = files.setdefault(case["file"], {})
            z[case["name"] + "/x"], z[case["name"] + "/to_send"] = x, to_send
            z[case["name"] + "/out"] = out
        print(case["name"], "w", case["w"], "padding", case["padding"], flush=True)
    for fname, z in files.items():
        path = os.path.join(OUT, fname)
        np.savez_compressed(path, **z)
        print(fname, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 2 ** 20
    return cases


# ---- plugin runs ------------------------------------------------------------------------------
class Net(Model):
    """Two-tensor model: weight (rows, cols) and bias (nb,)."""

    def __init__(self, rows, cols, nb):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.zeros(rows, cols))
        self.bias = torch.nn.Parameter(torch.zeros(nb))


class Graph:
    def __init__(self, nbrs):
        self.nbrs = set(nbrs)

    def neighbors(self, uid):
        return self.nbrs


def set_flat(model, flat):
    new, pos = {}, 0
    for key, v in model.state_dict().items():
        new[key] = torch.from_numpy(flat[pos:pos + v.numel()].reshape(v.shape).copy())
        pos += v.numel()
    model.load_state_dict(new)


def get_flat(model):
    return torch.cat([v.flatten() for v in model.state_dict().values()]).numpy().copy()


BIG, SMALL = [100, 199, 101], [40, 49, 41]  # n = 20,001 and n = 2001
CLASSES = {"Sharing": Sharing, "PartialModel": PartialModel,
           "PlainAverageSharing": PlainAverageSharing}
PLUGINS = [
    dict(name="sharing_quant", cls="Sharing", shape=BIG, compression="Quantization",
         float_precision=32767, nbrs=3),
    dict(name="sharing_quant_small", cls="Sharing", shape=SMALL, compression="Quantization",
         float_precision=255, nbrs=3),
    dict(name="partial_eliasquant", cls="PartialModel", shape=BIG, kwargs={"alpha": 0.1},
         compression="EliasQuantization", float_precision=32767, nbrs=3),
    dict(name="plain_2", cls="PlainAverageSharing", shape=BIG, nbrs=2),
    dict(name="plain_6", cls="PlainAverageSharing", shape=BIG, nbrs=6),
    dict(name="plain_quant", cls="PlainAverageSharing", shape=SMALL, compression="Quantization",
         float_precision=32767, nbrs=3),
]
ROUNDS = 2


class TieError(RuntimeError):
    pass


def run_plugin(p, x0_seed):
    rows, cols, nb = p["shape"]
    n = rows * cols + nb
    kwargs = dict(p.get("kwargs", {}))
    comp = p.get("compression")
    partial = p["cls"] == "PartialModel"
    sc = dict(name=p["name"], **{"class": p["cls"]}, kwargs=kwargs, shape=p["shape"], n=n,
              compression=comp, float_precision=p.get("float_precision"), partial=partial,
              degree=p["cls"] != "PlainAverageSharing", x0_seed=x0_seed,
              neighbours=[{"degree": 2 + j, "x_seed": 500 + 100 * j} for j in range(p["nbrs"])],
              rounds=[])
    ckw = dict(kwargs)
    if comp:
        ckw.update(compress=True, compression_package="decentralizepy.compression." + comp,
                   compression_class=comp, float_precision=p["float_precision"])
    uids = list(range(1, p["nbrs"] + 1))
    model = Net(rows, cols, nb)
    arrays = {"x0": ops.recipe(x0_seed, n)}
    set_flat(model, arrays["x0"])
    with tempfile.TemporaryDirectory() as tmp:
        plugin = CLASSES[p["cls"]](0, 0, None, Linear(1, 8), Graph(uids), model, None, tmp, **ckw)
    rng = np.random.default_rng(x0_seed + 1)
    for r in range(ROUNDS):
        x_r = (get_flat(model) + ops.recipe(x0_seed + 2 + r, n, 0.01)).astype(f32)
        assert np.any(x_r != arrays["x0"])  # a nonzero model change in round 0
        set_flat(model, x_r)
        arrays[f"r{r}_x"] = x_r
        data = plugin.get_data_to_send(degree=len(uids))
        sc["rounds"].append({"keys": list(data)})
        assert data["iteration"] == r and ("degree" in data) == sc["degree"]
        if partial:
            assert "send_partial" in data
            change = plugin.model.model_change.numpy()
            if otopk.kth_has_tie(otopk.keys_u32(change), round(kwargs["alpha"] * n)):
                raise TieError(p["name"])
        if comp:
            scale, to_send = pickle.loads(data["params"])
            assert isinstance(scale, np.float32)
            arrays[f"r{r}_scale"], arrays[f"r{r}_to_send"] = np.array([scale], f32), to_send
            if partial:
                arrays[f"r{r}_indices_stream"] = ops.as_bytes(data["indices"]).copy()
        else:
            arrays[f"r{r}_params"] = np.asarray(data["params"], dtype=f32).copy()
        peers = OrderedDict()
        for j, nbm in enumerate(sc["neighbours"]):
            pre = f"r{r}_nbr{j}"
            if partial:
                k = round(kwargs["alpha"] * n)
                idx = np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32)
                m = {"alpha": kwargs["alpha"], "indices": idx,
                     "params": ops.recipe(nbm["x_seed"] + 10 * r, k, 0.05), "send_partial": True}
            else:
                m = {"params": ops.recipe(nbm["x_seed"] + 10 * r, n, 0.5)}
            if comp:  # as a reference node puts it on the wire
                if partial:
                    m["indices"] = plugin.compressor.compress(m["indices"])
                    arrays[pre + "_indices_stream"] = ops.as_bytes(m["indices"]).copy()
                m["params"] = plugin.compressor.compress_float(m["params"])
                scale, to_send = pickle.loads(m["params"])
                arrays[pre + "_scale"], arrays[pre + "_to_send"] = np.array([scale], f32), to_send
            if sc["degree"]:
                m["degree"] = nbm["degree"]
            m["iteration"] = r
            m["CHANNEL"] = "DPSGD"
            peers[uids[j]] = deque([m])
        plugin._averaging(peers)
        assert plugin.communication_round == r + 1
        arrays[f"r{r}_model_after"] = get_flat(model)
    path = os.path.join(OUT, f"quantization_plugin_{p['name']}.npz")
    np.savez_compressed(path, **arrays)
    print(p["name"], os.path.getsize(path), "bytes", flush=True)
    assert os.path.getsize(path) < 2 ** 20
    return sc


def plugin_scenarios():
    out = []
    for i, p in enumerate(PLUGINS):
        for attempt in range(20):
            try:
                out.append(run_plugin(p, 7000 + 100 * i + 10 * attempt))
                break
            except TieError as e:
                print("retry:", e)
        else:
            raise RuntimeError(f"{p['name']}: no tie-free seed found")
    return out


def main():
    meta = {"numpy": np.__version__, "codec": codec_cases(), "plugins": plugin_scenarios()}
    with open(os.path.join(OUT, "quantization.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
