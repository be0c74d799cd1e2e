"""numpy restatement of an STC federation round (reference sharing/STC.py: 259-270 + 308-316 the
client's encode, :333-362 the server's average, :318-331 its broadcast, :281-306 the receipt), one
fp32 rounding per operation, in the sparse form the engine pins, plus the recipes
the recorded runs (tests/golden/make_golden_stc_round.py) are rebuilt from."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def perturbation(seed, r, u, n):
    """The "training" of client u before round r: a fixed seeded step, added in fp32."""
    rng = np.random.default_rng([seed, r, u])
    return (0.01 * rng.standard_normal(n)).astype(np.float32)


def train(x, meta, r, u):
    """Client u's model before round r's encode, from its model after its last receipt."""
    return (x + perturbation(meta["seed"], r, u, x.size)).astype(np.float32)


def keys(c):
    """|c| as the order-preserving uint32 key of the codec (every NaN -> 0x7FC00000)."""
    b = np.ascontiguousarray(c, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.where(b > 0x7F800000, np.uint32(0x7FC00000), b).astype(np.uint32)


def select(c, k):
    """The k largest keys of c, ties at the k-th key to the lowest indices; ascending int32."""
    order = np.argsort(-keys(c).astype(np.int64), kind="stable")[:k]
    return np.sort(order).astype(np.int32)


def tie_run(c, k):
    """(indices whose key equals the k-th largest key, how many of them the selection takes)."""
    ks = keys(c)
    T = np.sort(ks)[ks.size - k]
    return np.flatnonzero(ks == T), k - int((ks > T).sum())


def encode(x, prev, r, k):
    """A client's ``get_data_to_send`` in place on prev and r: c = fl(fl(x - prev) + r), the
    payload (idx, c[idx]), prev = x, r = c with +0 at idx.  x None: the server's broadcast form,
    r already holds c and prev is not touched."""
    if x is not None:
        c = (x - prev).astype(np.float32) + r
        prev[:] = x
    else:
        c = r.copy()
    idx = select(c, k)
    vals = c[idx].astype(np.float32)
    r[:] = c
    r[idx] = 0.0
    return idx, vals


def server_fold(r_s, pays, w):
    """``_averaging_server`` in place: total = +0, total[idx] = fl(total[idx] + fl(vals w)) per
    payload in order, r_s = fl(r_s + total) (the server's change vector).  w is rounded to fp32 as
    torch rounds a scalar."""
    total = np.zeros_like(r_s)
    for idx, vals in pays:
        total[idx] = total[idx] + vals * np.float32(w)
    r_s[:] = r_s + total
    return total


def apply(x, idx, vals):
    """``process_received`` in place, sparse: only the named elements change."""
    x[idx] = x[idx] + vals


def load_runs():
    """[(meta, arrays)] of the recorded reference runs."""
    with open(os.path.join(GOLDEN, "stc_round.json")) as f:
        metas = json.load(f)["runs"]
    return [(m, dict(np.load(os.path.join(GOLDEN, f"stc_round_{m['name']}.npz"),
                             allow_pickle=False))) for m in metas]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_payload(arr, r, slot, idx, vals, what="payload"):
    """A worker's payload of round r (slot: its place in the round's worker order; None: the
    broadcast) against the recording."""
    name = f"r{r}_b" if slot is None else f"r{r}_p"
    wi, wv = arr[name + "_idx"], arr[name + "_vals"]
    if slot is not None:
        wi, wv = wi[slot], wv[slot]
    np.testing.assert_array_equal(np.asarray(idx), wi, err_msg=f"{what} idx r{r} {slot}")
    np.testing.assert_array_equal(u32(vals), u32(wv), err_msg=f"{what} vals r{r} {slot}")


def check_state(meta, arr, r, x, xs, prev=None, res=None, res_s=None, lo=0):
    """Client rows [lo, lo + len(x)) and the server after round r against the recording, bit for
    bit; after the last round the residuals and prev_model too."""
    m = len(x)
    np.testing.assert_array_equal(u32(x), u32(arr[f"r{r}_x"][lo:lo + m]), err_msg=f"x r{r}")
    np.testing.assert_array_equal(u32(xs), u32(arr[f"r{r}_xs"]), err_msg=f"server x r{r}")
    if r == meta["rounds"] - 1 and prev is not None:
        np.testing.assert_array_equal(u32(prev), u32(arr["prev"][lo:lo + m]), err_msg="prev")
        np.testing.assert_array_equal(u32(res), u32(arr["res"][lo:lo + m]), err_msg="residuals")
        np.testing.assert_array_equal(u32(res_s), u32(arr["res_s"]), err_msg="server residuals")
