"""numpy restatement of the batched JWINS selection (dpz_jwins_encode_nodes; reference
sharing/JWINS/Wavelet.py:142-231 over sharing/PartialModel.py:326-329) on ``oracle.topk.encode``
with ACC_ADD and a separate value source, plus the recipes the recorded whole-topology runs
(tests/golden/make_golden_jwins_round.py) are rebuilt from - TEST INFRASTRUCTURE ONLY."""
import json
import os

import numpy as np

from oracle import topk as otopk
from tests.choco_round_ops import EDGES_IRR6, adjacency  # noqa: F401 - the 6-node graph's edges

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TUTORIAL_ALPHAS = [0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 1.0]  # tutorial/JWINS/config.ini
f32 = np.float32


def perturbation(seed, r, u, n):
    """The "training" of node u before round r: a fixed seeded step, added in fp32."""
    rng = np.random.default_rng([seed, r, u])
    return (0.01 * rng.standard_normal(n)).astype(f32)


def train(x, meta, r, u):
    """Node u's model before round r's exchange, from its model after round r - 1."""
    return (x + perturbation(meta["seed"], r, u, x.size)).astype(f32)


def key(c, acc):
    """The selection's key vector fl(c + acc), as the first pass stores it into the c row."""
    return (np.asarray(c, f32) + np.asarray(acc, f32)).astype(f32)


def kth_has_tie(c, acc, k):
    return otopk.kth_has_tie(otopk.keys_u32(key(c, acc)), k)


def encode_node(c, acc, vals_src, counter, k):
    """One node of dpz_jwins_encode_nodes in place on acc and counter (None: not kept).  k >= 1:
    ``(idx ascending, vals_src[idx])`` of the k largest |c + acc|, ties to the lowest indices,
    counter[idx] += 1, acc[idx] = +0.  k == 0, a full share: acc = +0 everywhere, ``(None, a
    copy of vals_src)``."""
    if k == 0:
        acc[:] = 0.0
        return None, np.array(vals_src, dtype=f32, copy=True)
    return otopk.encode(c, None, acc, otopk.ACC_ADD, k, vals_src=vals_src, counter=counter)


def load_runs():
    """[(meta, arrays)] of the recorded reference runs."""
    with open(os.path.join(GOLDEN, "jwins_round.json")) as f:
        metas = json.load(f)["runs"]
    return [(m, dict(np.load(os.path.join(GOLDEN, f"jwins_round_{m['name']}.npz"),
                             allow_pickle=False))) for m in metas]


def run_adjacency(meta):
    if "edges_file" in meta:
        from decentralizepy_amd.gossip import read_edges
        return read_edges(os.path.join(GOLDEN, meta["edges_file"]))
    return adjacency(meta["nodes"], [tuple(e) for e in meta["edges"]])


def u32(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def check_payload(meta, arr, r, u, alpha, idx, vals):
    """Node u's alpha and payload of round r against the recording (a full share is recorded by
    its alpha alone: its values are the W(x) the recorded models follow from)."""
    assert alpha == arr[f"r{r}_alpha"][u], f"alpha r{r} {u}"
    if alpha >= meta["metadata_cap"]:
        assert idx is None and f"r{r}_n{u}_idx" not in arr and len(vals) == meta["m_len"]
        return
    np.testing.assert_array_equal(np.asarray(idx), arr[f"r{r}_n{u}_idx"], err_msg=f"idx r{r} {u}")
    np.testing.assert_array_equal(u32(vals), u32(arr[f"r{r}_n{u}_vals"]),
                                  err_msg=f"vals r{r} {u}")


def check_state(meta, arr, r, x, acc=None, counter=None, lo=0):
    """Rows [lo, lo + len(x)) after round r against the recording, bit for bit; after the last
    round the accumulators and counters too."""
    m = len(x)
    np.testing.assert_array_equal(u32(x), u32(arr[f"r{r}_x"][lo:lo + m]), err_msg=f"x r{r}")
    if r == meta["rounds"] - 1 and acc is not None:
        np.testing.assert_array_equal(u32(acc), u32(arr["acc"][lo:lo + m]), err_msg="acc")
        np.testing.assert_array_equal(np.asarray(counter), arr["counter"][lo:lo + m],
                                      err_msg="counter")


def drive(eng, meta, arr, lo=0, every_payload=False):
    """The recorded rounds through an engine: training into ``eng.x`` in place, a step, the
    comparison of draws, payloads, models and, at the end, the accumulators and counters."""
    import torch
    m = eng.hi - eng.lo
    x_ptr = eng.x.data_ptr()
    for r in range(meta["rounds"]):
        x = eng.x.cpu().numpy()
        for j in range(m):
            x[j] = train(x[j], meta, r, lo + j)
        eng.x.copy_(torch.from_numpy(x).to(eng.x.device))
        eng.step()
        assert eng.round == r + 1 and eng.x.data_ptr() == x_ptr
        for u in (range(meta["nodes"]) if every_payload else range(lo, lo + m)):
            idx, vals = eng.payload(u)
            check_payload(meta, arr, r, u, eng.alphas[u],
                          None if idx is None else idx.cpu().numpy(), vals.cpu().numpy())
        assert torch.equal(eng.x, eng.x0)
        check_state(meta, arr, r, eng.x.cpu().numpy(), eng.acc.cpu().numpy(),
                    eng.counter.cpu().numpy(), lo=lo)
