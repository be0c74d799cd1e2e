"""numpy restatement of the reference quantiser (compression/Quantization.py) — TEST
INFRASTRUCTURE ONLY — and the replay of its recorded runs (tests/golden/quantization*.{json,npz},
make_golden_quantization.py) against the restatement (CPU tests) or the device codec and plugins
(GPU tests).

The restatement spells out every fp32 operation, so it does not depend on the numpy that runs it:
the sum of |x| is numpy's ``add.reduce`` order written as array steps (consecutive chunks of 8192
elements, each numpy's pairwise tree — eight strided accumulators per leaf of at most 128
elements, halves of ``len/2 - (len/2) % 8`` above that — and the chunk sums added one after
another), the divisions are IEEE fp32 divisions, ``rint`` rounds ties to even.
"""
import hashlib
import json
import os
import pickle
from collections import deque

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHUNK = 8192
LEAF = 128
KS = [1, 7, 255, 256, 32767, 2 ** 20, 2 ** 30 - 1]
NS = [1, 2, 7, 8, 9, 33, 1000, 20001]
SUM_SIZES = [1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 8321, 28675, 100000, 131072,
             2 ** 20 + 5]
f32 = np.float32


# ---- summation order ---------------------------------------------------------------------------
def _leaf(a):
    """numpy's pairwise leaf over an fp32 array of at most 128 elements."""
    n = len(a)
    if n < 8:
        s = f32(0)
        for v in a:
            s = f32(s + v)
        return s
    body = n - n % 8
    r = a[:8].copy()
    for i in range(8, body, 8):
        r = r + a[i:i + 8]
    res = f32(f32(f32(r[0] + r[1]) + f32(r[2] + r[3])) + f32(f32(r[4] + r[5]) + f32(r[6] + r[7])))
    for v in a[body:]:
        res = f32(res + v)
    return res


def pairwise(a):
    """numpy's pairwise sum of an fp32 array (one tree over the whole array)."""
    n = len(a)
    if n <= LEAF:
        return _leaf(a)
    h = n // 2
    h -= h % 8
    return f32(pairwise(a[:h]) + pairwise(a[h:]))


def _full_chunks(a):
    """The pairwise sums of the rows of an (m, 8192) fp32 array: a perfect tree over 64 leaves."""
    r = a.reshape(a.shape[0], CHUNK // LEAF, LEAF // 8, 8)
    acc = r[:, :, 0, :].copy()
    for i in range(1, LEAF // 8):
        acc = acc + r[:, :, i, :]
    while acc.shape[-1] > 1:  # ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7))
        acc = acc[..., 0::2] + acc[..., 1::2]
    acc = acc[..., 0]
    while acc.shape[-1] > 1:  # adjacent leaves, level by level
        acc = acc[:, 0::2] + acc[:, 1::2]
    return acc[:, 0]


def abs_sum(x):
    """``np.abs(x).sum()`` of a contiguous 1-D fp32 array, operation by operation."""
    a = np.abs(np.ascontiguousarray(x, dtype=f32).reshape(-1))
    assert a.dtype == f32 and a.size >= 1
    nfull = a.size // CHUNK
    sums = list(_full_chunks(a[:nfull * CHUNK].reshape(nfull, CHUNK))) if nfull else []
    if a.size % CHUNK:
        sums.append(pairwise(a[nfull * CHUNK:]))
    return np.add.accumulate(np.asarray(sums, dtype=f32), dtype=f32)[-1]  # a sequential chain


# ---- codec ---------------------------------------------------------------------------------------
def params(x, k):
    """(scale, norm, p, w) of the encode of x with float_precision k."""
    x = np.ascontiguousarray(x, dtype=f32).reshape(-1)
    if x.size < 1:
        raise ValueError("empty")
    if not np.all(np.isfinite(x)):
        raise ValueError("non-finite")
    m = np.max(np.abs(x))
    if m == 0:
        raise ValueError("all zero")
    kf = f32(k)
    scale = f32(f32(abs_sum(x) / f32(x.size)) / kf)
    norm = f32(m / kf)
    qmax = abs(int(np.rint(f32(m / norm))))
    p = 1 << qmax.bit_length()  # 2^ceil(log2 qmax), doubled when it equals qmax
    return scale, norm, p, p.bit_length()


def quantise(x, norm):
    return np.rint(np.ascontiguousarray(x, dtype=f32).reshape(-1) / f32(norm)).astype(np.int32)


def pack(u, w):
    """The stream body: value i at stream bits [i*w, (i+1)*w), MSB first; bytes fill LSB first."""
    u = np.asarray(u, dtype=np.uint64)
    shifts = np.arange(w - 1, -1, -1, dtype=np.uint64)
    bits = ((u[:, None] >> shifts[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little")


def encode(x, k):
    """(np.float32 scale, uint8 to_send) — reference Quantization.compress_float before the
    pickle."""
    scale, norm, p, w = params(x, k)
    q = quantise(x, norm)
    body = pack(q.astype(np.int64) + (p - 1), w)
    padding = (8 - (q.size * w) % 8) % 8
    return scale, np.concatenate([np.array([padding, w], np.uint8), body])


def decode(scale, to_send):
    """fp32 values — reference Quantization.decompress_float after the unpickle."""
    to_send = np.asarray(to_send, dtype=np.uint8)
    padding, w = int(to_send[0]), int(to_send[1])
    bits = np.unpackbits(to_send[2:], bitorder="little")
    bits = bits[:bits.size - padding].reshape(-1, w).astype(np.int64)
    weights = np.int64(1) << np.arange(w - 1, -1, -1, dtype=np.int64)
    v = (bits * weights).sum(axis=1) - (1 << (w - 1)) + 1
    return (v.astype(np.float64) * np.float64(scale)).astype(f32)


def wire(scale, to_send):
    return pickle.dumps((f32(scale), np.asarray(to_send, dtype=np.uint8)))


def unwire(data):
    scale, to_send = pickle.loads(data)
    return scale, to_send


def as_bytes(v):
    return np.frombuffer(memoryview(np.ascontiguousarray(v)), dtype=np.uint8)


def bits_of(scale):
    return int(np.asarray(scale, dtype=f32).reshape(1).view(np.uint32)[0])


# ---- the recorded reference runs -------------------------------------------------------------
def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def recipe(seed, n, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(f32)


def mixed(seed, n):
    """Mostly 1e-3 with a few 1e3 values (the summation-order case)."""
    rng = np.random.default_rng(seed)
    x = (1e-3 * rng.standard_normal(n)).astype(f32)
    x[rng.choice(n, size=max(n // 2000, 3), replace=False)] = f32(1e3)
    return x


def case_input(case):
    """The input of a codec case from its recorded recipe."""
    kind, n = case["kind"], case["n"]
    if kind == "normal":
        return recipe(case["seed"], n, 0.01)
    if kind == "ties":  # norm is exactly 2^-10, every value but the max sits on a tie
        j = np.arange(-255, 255, dtype=np.float64)
        return np.concatenate([(j + 0.5) * 2.0 ** -10, [255 * 2.0 ** -10]]).astype(f32)
    if kind == "tiny":  # max|x| ~ 1e-38: norm is subnormal
        return (1e-38 * np.random.default_rng(case["seed"]).uniform(-1, 1, n)).astype(f32)
    if kind == "mixed":
        return mixed(case["seed"], n)
    raise KeyError(kind)


def meta():
    with open(os.path.join(GOLDEN, "quantization.json")) as f:
        return json.load(f)


def codec_cases():
    return meta()["codec"]


def codec_ids():
    return [c["name"] for c in codec_cases()]


_npz = {}


def _arrays(fname):
    if fname not in _npz:
        _npz[fname] = dict(np.load(os.path.join(GOLDEN, fname)))
    return _npz[fname]


def load_case(name):
    """(case, x, to_send or None, out or None): the recorded arrays where the case stores them."""
    case = next(c for c in codec_cases() if c["name"] == name)
    x = case_input(case)
    if "file" not in case:
        return case, x, None, None
    z = _arrays(case["file"])
    np.testing.assert_array_equal(z[name + "/x"].view(np.uint32), x.view(np.uint32))
    return case, x, z[name + "/to_send"], z[name + "/out"]


def check_case(case, scale, to_send, out, rec_to_send=None, rec_out=None):
    """One codec result against the record: header, scale bits, stream and decoded values."""
    to_send = np.asarray(to_send)
    out = np.ascontiguousarray(out)
    assert to_send.dtype == np.uint8 and out.dtype == f32
    assert bits_of(scale) == case["scale_bits"], (bits_of(scale), case["scale_bits"])
    assert (int(to_send[0]), int(to_send[1])) == (case["padding"], case["w"])
    assert out.size == case["n"]
    if rec_to_send is not None:
        np.testing.assert_array_equal(to_send, rec_to_send)
        np.testing.assert_array_equal(out.view(np.uint32), rec_out.view(np.uint32))
    assert sha(to_send[2:]) == case["body_sha"]
    assert sha(out) == case["out_sha"]


# ---- plugin runs ------------------------------------------------------------------------------
def plugin_scenarios():
    return meta()["plugins"]


def plugin_ids():
    return [s["name"] for s in plugin_scenarios()]


def load_plugin(name):
    sc = next(s for s in plugin_scenarios() if s["name"] == name)
    return sc, _arrays(f"quantization_plugin_{name}.npz")


def neighbour_msgs(sc, arrays, r):
    """The neighbours' wire dicts of round r as the reference nodes sent them."""
    msgs = []
    for j, nb in enumerate(sc["neighbours"]):
        pre = f"r{r}_nbr{j}"
        m = {}
        if sc["compression"]:
            m["params"] = wire(arrays[pre + "_scale"][0], arrays[pre + "_to_send"])
        else:
            m["params"] = recipe(nb["x_seed"] + 10 * r, sc["n"], 0.5)
        if sc["partial"]:
            m = {"alpha": sc["kwargs"]["alpha"], "indices": arrays[pre + "_indices_stream"].copy(),
                 "params": m["params"], "send_partial": True}
        if sc["degree"]:
            m["degree"] = nb["degree"]
        m["iteration"] = r
        m["CHANNEL"] = "DPSGD"
        msgs.append(m)
    return msgs


def check_sent(sc, arrays, r, data):
    """The node's wire dict of round r against the record (params unpickled)."""
    assert list(data) == sc["rounds"][r]["keys"], list(data)
    assert data["iteration"] == r
    if sc["degree"]:
        assert data["degree"] == len(sc["neighbours"])
    if sc["compression"]:
        scale, to_send = unwire(data["params"])
        assert isinstance(scale, np.float32)
        assert bits_of(scale) == bits_of(arrays[f"r{r}_scale"][0])
        np.testing.assert_array_equal(to_send, arrays[f"r{r}_to_send"])
    else:
        np.testing.assert_array_equal(np.asarray(data["params"]).view(np.uint32),
                                      arrays[f"r{r}_params"].view(np.uint32))
    if sc["partial"]:  # the Elias stream of the indices, byte for byte
        np.testing.assert_array_equal(as_bytes(data["indices"]), arrays[f"r{r}_indices_stream"])


def replay_plugin(name, tmpdir):
    """Drive the device plugin through the scenario the way the Node drives the reference:
    get_data_to_send(), then _averaging(peer_deques); every wire dict and every averaged model
    must equal the record bit for bit."""
    import importlib

    from tests import scenario
    sc, arrays = load_plugin(name)
    model = scenario.make_model(sc["shape"])
    scenario.set_flat(model, arrays["x0"])
    kwargs = dict(sc["kwargs"])
    if sc["compression"]:
        kwargs.update(compress=True, compression_class=sc["compression"],
                      compression_package="decentralizepy_amd.compression." + sc["compression"])
        if sc["float_precision"] is not None:
            kwargs["float_precision"] = sc["float_precision"]
    cls = getattr(importlib.import_module("decentralizepy_amd.sharing." + sc["class"]),
                  sc["class"])
    uids = list(range(1, len(sc["neighbours"]) + 1))
    plugin = cls(0, 0, None, scenario._Mapping(8), scenario._Graph(uids), model, None,
                 str(tmpdir), **kwargs)
    for r in range(len(sc["rounds"])):
        scenario.set_flat(model, arrays[f"r{r}_x"])
        check_sent(sc, arrays, r, plugin.get_data_to_send(degree=len(uids)))
        peers = {uid: deque([m]) for uid, m in zip(uids, neighbour_msgs(sc, arrays, r))}
        plugin._averaging(peers)
        assert plugin.communication_round == r + 1
        np.testing.assert_array_equal(scenario.get_flat(model).view(np.uint32),
                                      arrays[f"r{r}_model_after"].view(np.uint32))
    return plugin
