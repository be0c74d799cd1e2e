"""numpy restatement of the reference SubSampling plugin (sharing/SubSampling.py) — TEST
INFRASTRUCTURE ONLY — and the replay of its recorded runs (tests/golden/subsampling*.{json,npz},
make_golden_subsampling.py) against the restatement (CPU tests) or the device plugin (GPU tests).

The mask rule: ``torch.rand(n, generator=g) <= alpha`` after ``g.manual_seed(seed)`` is MT19937
seeded with ``seed & 0xffffffff``, one tempered 32-bit output per element, u = (out & 0xFFFFFF) *
2^-24 in fp32, compared with alpha rounded to fp32: ``(out & 0xFFFFFF) <= floor(float64(float32(
alpha)) * 2^24)``.  numpy's ``RandomState(seed).bytes`` is the same output stream.
"""
import hashlib
import json
import os
from collections import deque

import numpy as np

from oracle import fold as ofold

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def raw_outputs(seed, n):
    """The first n tempered 32-bit outputs of MT19937 seeded with ``seed & 0xffffffff``."""
    return np.frombuffer(np.random.RandomState(int(seed) & 0xffffffff).bytes(4 * int(n)), "<u4")


def threshold(alpha):
    """out24 <= threshold <=> u <= alpha; -1 selects nothing (alpha < 0 or NaN)."""
    a = np.float32(alpha)
    if not a >= 0:
        return -1
    return int(min(np.floor(np.float64(a) * 2.0 ** 24), 2.0 ** 24))


def mask(seed, alpha, n):
    return (raw_outputs(seed, n) & 0xFFFFFF).astype(np.int64) <= threshold(alpha)


def pack(m):
    """A boolean mask as the library's words: bit b of uint32 word w <-> element 32w + b."""
    b = np.packbits(np.asarray(m, dtype=bool), bitorder="little")
    b = np.concatenate([b, np.zeros(-len(b) % 4, np.uint8)])
    return b.view("<u4")


def encode(x, seed, alpha, counter=None):
    """``x[mask]`` (SubSampling.py:152-161); ``counter[mask] += 1`` when given."""
    m = mask(seed, alpha, len(x))
    if counter is not None:
        counter[m] += 1
    return np.asarray(x, dtype=np.float32)[m]


def indices(seed, alpha, n, k=None):
    idx = np.flatnonzero(mask(seed, alpha, n))
    if k is not None and len(idx) != k:  # T[binary_mask] = params raises in the reference
        raise ValueError(f"{k} params for a mask of {len(idx)} elements")
    return idx


def replace(local, seed, alpha, params):
    """deserialized_model (SubSampling.py:235-308) on the flat model."""
    return ofold.replace(local, indices(seed, alpha, len(local), len(params)), params)


def fold(local, payloads, weights, w_self=None):
    """``payloads``: list of (seed, alpha, params); the fold of oracle.fold over the masks."""
    pays = [(indices(s, a, len(local), len(p)), np.asarray(p, np.float32)) for s, a, p in payloads]
    return ofold.fold(local, pays, weights, w_self)


class OracleNode:
    """numpy mirror of a reference SubSampling node (flat model, fp32 exact)."""

    def __init__(self, x0, seed, alpha, layerwise):
        self.model = np.array(x0, dtype=np.float32)
        self.seed, self.alpha, self.layerwise = seed, alpha, layerwise
        self.counter = np.zeros(len(x0), np.int32)
        self.communication_round = 0

    def get_data_to_send(self):
        s = self.seed + self.communication_round
        params = encode(self.model, s, self.alpha, None if self.layerwise else self.counter)
        return {"seed": s, "alpha": self.alpha, "params": params}

    def averaging(self, msgs, server=False):
        pays = [(m["seed"], m["alpha"], m["params"]) for m in msgs]
        if server:
            self.model = fold(self.model, pays, [1 / len(msgs)] * len(msgs), None)
        else:
            w = [ofold.mh_weight(len(msgs), m["degree"]) for m in msgs]
            wt = 0
            for v in w:
                wt += v
            self.model = fold(self.model, pays, w, 1 - wt)
        self.communication_round += 1


# ---- the recorded reference runs ----------------------------------------------------------------
def scenarios():
    with open(os.path.join(GOLDEN, "subsampling.json")) as f:
        return json.load(f)["scenarios"]


def names():
    return [s["name"] for s in scenarios()]


def recipe(seed, n, scale=1.0):
    """The models of a scenario: a recorded generator recipe (the large scenario stores no
    arrays, only this and the hashes of its outputs)."""
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load(name):
    """(meta, arrays): the inputs of the scenario — x0 and the neighbours' models from the
    recipe — plus, for the small scenarios, every recorded array."""
    meta = next(s for s in scenarios() if s["name"] == name)
    arrays = {"x0": recipe(meta["x0_seed"], meta["n"])}
    for j, nb in enumerate(meta["neighbours"]):
        arrays[f"nbr{j}_x"] = recipe(nb["x_seed"], meta["n"], 0.5)
    path = os.path.join(GOLDEN, f"subsampling_{name}.npz")
    if os.path.exists(path):
        rec = dict(np.load(path))
        for key in ("x0",) + tuple(f"nbr{j}_x" for j in range(len(meta["neighbours"]))):
            np.testing.assert_array_equal(rec.pop(key).view(np.uint32), arrays[key].view(np.uint32))
        arrays.update(rec)
    return meta, arrays


def neighbour_msgs(meta, arrays, r):
    """The neighbours' wire dicts of round r.  Recorded params where the scenario stores them;
    the large scenario restates them (x[mask]) and checks the recorded hash and count."""
    msgs = []
    for j, nb in enumerate(meta["neighbours"]):
        seed = nb["seed"] + r
        key = f"r{r}_nbr{j}_params"
        if key in arrays:
            params = arrays[key].copy()
        else:
            params = encode(arrays[f"nbr{j}_x"], seed, nb["alpha"])
            assert sha(params) == meta["rounds"][r]["nbr_sha"][j]
        assert len(params) == meta["rounds"][r]["nbr_k"][j]
        msgs.append({"seed": seed, "alpha": nb["alpha"], "params": params,
                     "degree": nb["degree"], "iteration": r, "CHANNEL": "DPSGD"})
    return msgs


def check_round(meta, arrays, r, params, counter, model):
    mr = meta["rounds"][r]
    params, counter, model = (np.ascontiguousarray(a) for a in (params, counter, model))
    assert params.dtype == np.float32 and len(params) == mr["k"]
    assert counter.dtype == np.int32 and model.dtype == np.float32
    if f"r{r}_params" in arrays:
        np.testing.assert_array_equal(params.view(np.uint32), arrays[f"r{r}_params"].view(np.uint32))
        np.testing.assert_array_equal(counter, arrays[f"r{r}_counter"])
        np.testing.assert_array_equal(model.view(np.uint32),
                                      arrays[f"r{r}_model_after"].view(np.uint32))
    assert sha(params) == mr["params_sha"]
    assert sha(counter) == mr["counter_sha"]
    assert sha(model) == mr["model_sha"]


def replay_oracle(name):
    meta, arrays = load(name)
    node = OracleNode(arrays["x0"], meta["seed"], meta["alpha"], meta["layerwise"])
    for r in range(len(meta["rounds"])):
        data = node.get_data_to_send()
        assert data["seed"] == meta["seed"] + r
        counter = node.counter.copy()
        node.averaging(neighbour_msgs(meta, arrays, r),
                       server=meta["averaging"] == "_averaging_server")
        check_round(meta, arrays, r, data["params"], counter, node.model)


# ---- device plugin backend -------------------------------------------------------------------------
def make_model(shape):
    import torch

    class Net(torch.nn.Module):
        """Three state tensors (the layerwise form draws the mask tensor by tensor)."""

        def __init__(self, rows, cols, nb, ne):
            super().__init__()
            self.weight = torch.nn.Parameter(torch.zeros(rows, cols))
            self.bias = torch.nn.Parameter(torch.zeros(nb))
            self.scale = torch.nn.Parameter(torch.zeros(ne))
            self.shared_parameters_counter = None

    return Net(*shape)


def replay_plugin(name, tmpdir, compression_class=None):
    """Drive decentralizepy_amd.sharing.SubSampling through the scenario the way the Node
    drives the reference: get_data_to_send(), then _averaging(peer_deques).  With
    ``compression_class`` the params leg travels compressed in both directions."""
    from decentralizepy_amd.sharing.SubSampling import SubSampling
    from tests import scenario
    meta, arrays = load(name)
    model = make_model(meta["shape"])
    scenario.set_flat(model, arrays["x0"])
    kwargs = dict(alpha=meta["alpha"], layerwise=meta["layerwise"])
    if compression_class:
        kwargs.update(compress=True, compression_class=compression_class,
                      compression_package=f"decentralizepy_amd.compression.{compression_class}")
    uids = [1, 2, 3]
    plugin = SubSampling(0, 0, None, scenario._Mapping(), scenario._Graph(uids), model, None,
                         str(tmpdir), **kwargs)
    plugin.seed = meta["seed"]
    for r in range(len(meta["rounds"])):
        data = plugin.get_data_to_send(degree=3)
        assert list(data) == ["seed", "alpha", "params", "degree", "iteration"]
        assert data["seed"] == meta["seed"] + r and data["alpha"] == meta["alpha"]
        assert data["degree"] == 3 and data["iteration"] == r
        if compression_class:
            data = plugin.decompress_data(dict(data))
        counter = model.shared_parameters_counter.numpy().copy()
        msgs = neighbour_msgs(meta, arrays, r)
        if compression_class:
            msgs = [plugin.compress_data(m) for m in msgs]
        peers = {uid: deque([m]) for uid, m in zip(uids, msgs)}
        getattr(plugin, meta["averaging"])(peers)
        assert plugin.communication_round == r + 1
        check_round(meta, arrays, r, np.asarray(data["params"]), counter,
                    scenario.get_flat(model))
    return plugin
