"""The numpy side of the whole-topology FFT round (decentralizepy_amd/gossip_fft.py) - TEST
INFRASTRUCTURE ONLY: the loader of the runs recorded from the unmodified reference ``FFT`` class
(tests/golden/make_golden_fft_round.py), ``OracleFftOps``, the CPU stand-in for the HIP codec built
on oracle/fft.py and oracle/topk.py, and ``encode_node``, a numpy restatement of one node of
``dpz_cplx_encode_nodes``."""
import json
import os

import numpy as np
import torch

from oracle import fft as offt
from oracle import fold as ofold
from oracle import topk as otopk
from tests import scenario
from tests.jwins_round_ops import (EDGES_IRR6, adjacency, perturbation,  # noqa: F401
                                   run_adjacency, train)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32, c64 = np.float32, np.complex64
MIN_GAP = 1e-4  # the k-th key's relative distance from the (k + 1)-th in every recorded selection


def kth_gap(key, k):
    """Relative gap between the k-th and the (k + 1)-th largest key."""
    s = np.sort(np.asarray(key, dtype=np.float64))[::-1]
    if k >= len(s):
        return 1.0
    return float((s[k - 1] - s[k]) / max(s[k - 1], 1e-30))


def key_of(change, acc, mode):
    """The accumulation step of ``cplx_key_kernel`` and the fp32 key: (key, acc after the step),
    one fp32 rounding per operation."""
    c = np.asarray(change, dtype=c64).copy()
    if mode == otopk.ACC_ACCUMULATE:
        acc = (acc + c).astype(c64)  # per component: one fp32 add each
        c = acc
    elif mode == otopk.ACC_ADD:
        c = (c + acc).astype(c64)
    return offt.cabs(c), acc


def encode_node(change, acc, mode, vals_src, counter, k):
    """One node of ``dpz_cplx_encode_nodes`` in place on ``acc`` and ``counter`` (None: not
    kept): returns (key fp32[M], pairs int32[2k], vals complex64[k]); the k largest keys, ties to
    the lowest indices, ascending."""
    key, new_acc = key_of(change, acc, mode)
    if mode == otopk.ACC_ACCUMULATE:
        acc[:] = new_acc
    idx = otopk.topk_select(otopk.keys_u32(key), k)
    vals = np.asarray(vals_src, dtype=c64)[idx].copy()
    if counter is not None:
        counter[idx] += 1
    if acc is not None:
        acc[idx] = 0
    return key, offt.pair_indices(idx).astype(np.int32), vals


def _np(t):
    return t.detach().cpu().numpy()


class OracleFftOps:
    """The operations ``FftRound`` asks of its ``ops``, in place on CPU torch tensors (their numpy
    views share memory): float64 numpy transforms rounded to fp32 (oracle/fft.py), the selection
    and the fold with one fp32 rounding per operation."""

    def transform_pair(self, x, x0, fx, ch):
        xn = _np(x)
        fx.copy_(torch.from_numpy(offt.rfft(xn)))
        ch.copy_(torch.from_numpy(offt.rfft(xn - _np(x0))))

    def encode(self, ch, acc, mode, fx, key, counter, k, pair_out, val_out):
        a = None if acc is None else acc.numpy()
        kv, pairs, vals = encode_node(_np(ch), a, mode, _np(fx), counter.numpy(), k)
        key.copy_(torch.from_numpy(kv))
        pair_out.copy_(torch.from_numpy(pairs))
        val_out.copy_(torch.from_numpy(vals.view(f32)))

    def fold_all(self, jobs, n):
        for local, pays, w, w_self, out in jobs:
            p = [(_np(i), _np(v)) for i, v in pays]
            out.copy_(torch.from_numpy(ofold.fold(_np(local), p, w, w_self)))

    def inverse(self, tot, n, out):
        out.copy_(torch.from_numpy(offt.irfft(_np(tot), n)))

    def accumulate(self, acc, new, prev):
        a = acc.numpy()
        a += offt.rfft(_np(new) - _np(prev))


# ---- the recorded reference runs ----------------------------------------------------------------
def patched(base, at, val):
    """``base`` (a (nodes, M) array) with the flat entries ``at`` replaced by ``val``."""
    out = np.array(base, copy=True)
    out.reshape(-1)[at] = val
    return out


def load_runs():
    """[(meta, arrays)] of the recorded reference runs.  A run with
    ``accumulate_averaging_changes`` stores its accumulators after the encode as the entries that
    differ from the accumulators after the previous averaging (zeros before round 0); the full
    rows ``r{r}_acc_enc`` are put together here."""
    with open(os.path.join(GOLDEN, "fft_round.json")) as f:
        metas = json.load(f)["runs"]
    runs = []
    for m in metas:
        arr = dict(np.load(os.path.join(GOLDEN, f"fft_round_{m['name']}.npz"),
                           allow_pickle=False))
        for r in range(m["rounds"]):
            if f"r{r}_acc_enc_at" in arr:
                base = arr[f"r{r - 1}_acc_avg"] if r else np.zeros_like(arr["r0_acc_avg"])
                arr[f"r{r}_acc_enc"] = patched(base, arr.pop(f"r{r}_acc_enc_at"),
                                               arr.pop(f"r{r}_acc_enc_val"))
        runs.append((m, arr))
    return runs


def engine_kwargs(meta):
    return dict(alpha=meta["alpha"], accumulation=meta["accumulation"],
                accumulate_averaging_changes=meta["accumulate_averaging_changes"])


def tol(meta, arr, what, r):
    """The bound of a frequency-domain ("params", "acc_enc", "acc_avg") or time-domain ("model")
    quantity of round r (0-based): ``scenario.fft_tol`` of one transform pair, times r + 1 - each
    round adds one transform pair's rounding to inputs already that far off, and the fold in
    between is a convex combination, which does not amplify an error."""
    return scenario.fft_tol(what, meta["n"], float(np.abs(arr["x0"]).max())) * (r + 1)


def close(got, ref, meta, arr, what, r, errs=None):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    bound = tol(meta, arr, what, r)
    if errs is not None:
        errs.setdefault(what, []).append(err / bound)
    assert np.isfinite(got.view(f32)).all() and err <= bound, (what, r, err, bound)


def drive(eng, meta, arr, lo=0, every_payload=False, errs=None):
    """The recorded rounds through an engine: training into ``eng.x`` in place, a step, and the
    comparison with the recording: indices and counters exactly, values, accumulators and models
    within ``tol``.  ``errs`` collects every error as a fraction of its bound.  Returns the
    engine's own arrays of every round (for the bit-for-bit comparisons between engines)."""
    m, k = eng.hi - eng.lo, meta["k"]
    x_ptr = eng.x.data_ptr()
    rows, out = slice(lo, lo + m), []
    for r in range(meta["rounds"]):
        x = eng.x.cpu().numpy()
        for j in range(m):
            x[j] = train(x[j], meta, r, lo + j)
        eng.x.copy_(torch.from_numpy(x).to(eng.x.device))
        snap = {}

        def mark(leg):
            if leg == "encode" and eng.acc is not None:
                snap["acc_enc"] = eng.acc.clone()
        eng.step(mark=mark)
        assert eng.round == r + 1 and eng.x.data_ptr() == x_ptr
        got = {}
        for u in (range(meta["nodes"]) if every_payload else range(lo, lo + m)):
            idx, vals = eng.payload(u)
            idx, vals = idx.cpu().numpy(), vals.cpu().numpy()
            assert idx.dtype == np.int32 and vals.dtype == c64 and idx.shape == (k,)
            np.testing.assert_array_equal(idx, arr[f"r{r}_idx"][u], err_msg=f"idx r{r} {u}")
            close(vals, arr[f"r{r}_params"][u], meta, arr, "params", r, errs)
            got[f"idx{u}"], got[f"vals{u}"] = idx, vals
        assert torch.equal(eng.x, eng.x0)
        got["counter"] = eng.counter.cpu().numpy()
        np.testing.assert_array_equal(got["counter"], arr[f"r{r}_counter"][rows])
        got["x"] = eng.x.cpu().numpy()
        close(got["x"], arr[f"r{r}_x"][rows], meta, arr, "model", r, errs)
        assert (eng.acc is not None) == meta["accumulation"]
        if eng.acc is not None:
            got["acc_enc"] = snap["acc_enc"].cpu().numpy()
            got["acc"] = eng.acc.cpu().numpy()
            close(got["acc_enc"], arr[f"r{r}_acc_enc"][rows], meta, arr, "acc_enc", r, errs)
            close(got["acc"], arr[f"r{r}_acc_avg"][rows], meta, arr, "acc_avg", r, errs)
        out.append(got)
    return out


def same_bits(a, b):
    """Two ``drive`` results (or dicts of arrays) agree bit for bit on their common keys."""
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        for name in sorted(set(ra) & set(rb)):
            x, y = np.ascontiguousarray(ra[name]), np.ascontiguousarray(rb[name])
            assert x.shape == y.shape and x.dtype == y.dtype, name
            assert x.tobytes() == y.tobytes(), name
