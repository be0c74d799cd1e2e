"""GPU: dpz_decode_average_batch's any-degree one-launch path (dpz_fold_walk.hip
fold_walk_any_kernel: nodes of any payload count, sparse and dense payloads mixed, more than 16
payloads in further launches that continue the total).  Every case is checked three ways: each
node bit for bit against the oracle's fold (reference sharing/Sharing.py:156-190 over
PartialModel payloads, PartialModel.py:257-303; full shares as JWINS/Wavelet.py:269-309), the
launches against dpz_debug_fold_batch_plan, and the outputs bit for bit against the node-after-
node launches of the diagnostic build (DPZ_FOLD_BATCH=0).  Outputs start as NaN, so an element
no launch wrote shows."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import fold as ofold

pytestmark = pytest.mark.gpu

COUNTS = (1, 3, 4, 5, 8, 12, 13, 16)


def _ptrs(ts):
    return (ctypes.c_void_p * max(1, len(ts)))(*[(t.data_ptr() if t is not None else 0) for t in ts])


def _args(locs, outs, pays, weights, w_selfs):
    m = len(locs)
    idx = [i for p in pays for i, _ in p]
    val = [v for p in pays for _, v in p]
    return dict(
        m=m, n=locs[0].numel(), local=_ptrs(locs), out=_ptrs(outs),
        counts=(ctypes.c_int * m)(*[len(p) for p in pays]), idx=_ptrs(idx), val=_ptrs(val),
        k=(ctypes.c_int64 * len(val))(*[v.numel() for v in val]),
        w=(ctypes.c_float * len(val))(*[x for ws in weights for x in ws]),
        w_self=(ctypes.c_float * m)(*w_selfs))


def _batch(L, a, flags, dev):
    from decentralizepy_amd import codec
    wss = [codec.Workspace(dev) for _ in range(3)]
    dws = [x.get_decode(a["n"], 16) for x in wss]
    st = (ctypes.c_void_p * 3)(*[torch.cuda.current_stream(dev).cuda_stream] * 3)
    rc = L.dpz_decode_average_batch(a["m"], a["local"], a["out"], a["n"], a["counts"], a["idx"],
                                    a["val"], a["k"], a["w"], a["w_self"], flags, _ptrs(dws),
                                    min(d.numel() for d in dws), 3, st)
    torch.cuda.synchronize()
    return rc


def _guarded(L, a, flags, guard, dev):
    rc = L.dpz_decode_average_batch_guarded(
        a["m"], a["local"], a["out"], a["n"], a["counts"], a["idx"], a["val"], a["k"], a["w"],
        a["w_self"], flags, ctypes.c_void_p(guard.data_ptr()), guard.numel(),
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc


def _plan(a, pays, flags, aligned=1):
    from decentralizepy_amd import _lib
    dense = [1 if i is None else 0 for p in pays for i, _ in p]
    out = (ctypes.c_int * 4)()
    assert _lib.lib().dpz_debug_fold_batch_plan(
        a["m"], a["n"], a["counts"], a["k"], (ctypes.c_int * len(dense))(*dense), flags, aligned,
        out) == 0
    return dict(zip(("path", "launches", "first", "passes"), out))


def _sparse(rng, n, k):
    i = np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32)
    return i, rng.standard_normal(k).astype(np.float32)


def _weights(npay):
    w = [1 / (npay + 1)] * npay
    tot = 0
    for v in w:
        tot += v
    return w, 1 - tot


def _case(m, n, alpha, seed, counts, k_one=False):
    """m nodes of the given payload counts, sparse payloads of about alpha * n entries (k_one: one
    payload of a single entry mixed in)."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    xs = [torch.randn(n, generator=g).numpy() for _ in range(m)]
    pays, weights, w_selfs = [], [], []
    for j in range(m):
        p = [_sparse(rng, n, max(1, int(alpha * n * (0.5 + rng.random())))) for _ in range(counts[j])]
        if k_one and j == m // 2:
            p[len(p) // 2] = _sparse(rng, n, 1)
        pays.append(p)
        w, ws = _weights(counts[j])
        weights.append(w)
        w_selfs.append(ws)
    return xs, pays, weights, w_selfs


def _check(dev, monkeypatch, xs, pays, weights, w_selfs, flags, local_of=None):
    """The three checks.  pays: per node [(idx or None, vals)] in numpy; local_of: {(node, payload):
    node b}: that dense payload IS node b's local row on the device."""
    from decentralizepy_amd import _lib, codec
    from decentralizepy_amd._lib import DPZ_FOLD_ALSO_LOCAL, DPZ_FOLD_SELF
    m, n = len(xs), xs[0].size
    local_of = local_of or {}

    def device_side():
        locs = [torch.from_numpy(x).to(dev) for x in xs]
        dp = [[(None if i is None else torch.from_numpy(i).to(dev),
                locs[local_of[(j, q)]] if (j, q) in local_of else torch.from_numpy(v).to(dev))
               for q, (i, v) in enumerate(p)] for j, p in enumerate(pays)]
        outs = [torch.full((n,), float("nan"), device=dev) for _ in range(m)]
        return locs, dp, outs

    locs, dp, outs = device_side()
    a = _args(locs, outs, dp, weights, w_selfs)
    pl = _plan(a, pays, flags)
    assert pl["path"] == 2
    with codec.KernelTimer() as t:
        assert _batch(_lib.lib(), a, flags, dev) == 0
    assert t.result["fold"][1] == pl["launches"] and "fold_offsets" not in t.result
    got = [o.cpu().numpy() for o in outs]
    for j in range(m):
        ref = ofold.fold(xs[j], pays[j], weights[j], w_selfs[j] if flags & DPZ_FOLD_SELF else None)
        np.testing.assert_array_equal(got[j].view(np.uint32), ref.view(np.uint32),
                                      err_msg=f"node {j} of {[len(p) for p in pays]}")
        want_local = ref if flags & DPZ_FOLD_ALSO_LOCAL else xs[j]
        np.testing.assert_array_equal(locs[j].cpu().numpy().view(np.uint32),
                                      want_local.view(np.uint32), err_msg=f"local of node {j}")
    if not os.path.exists(_lib.DIAG_PATH):
        pytest.skip("libdpzcodec_diag.so not built (make -C decentralizepy_amd/csrc diag-lib)")
    monkeypatch.setenv("DPZ_FOLD_BATCH", "0")
    locs, dp, outs = device_side()
    assert _batch(_lib.diag_lib(), _args(locs, outs, dp, weights, w_selfs), flags, dev) == 0
    for j in range(m):
        np.testing.assert_array_equal(outs[j].cpu().numpy().view(np.uint32), got[j].view(np.uint32),
                                      err_msg=f"node {j} against its own launch")
    return pl


@pytest.mark.parametrize("m,n,alpha", [(9, 4_100, 0.01), (30, 100_003, 0.1), (23, 65_536, 0.3)])
def test_mixed_payload_counts(dev, monkeypatch, m, n, alpha):
    """1..16 payloads per node in one batch; 23 x 65,536 has more tiles than the grid has waves
    (runs cross node boundaries) and tiles of more than 64 entries per payload."""
    from decentralizepy_amd._lib import DPZ_FOLD_SELF
    rng = np.random.default_rng(m)
    counts = list(COUNTS) + [int(c) for c in rng.choice(COUNTS, size=m - len(COUNTS))]
    xs, pays, weights, w_selfs = _case(m, n, alpha, m + n, counts, k_one=alpha < 0.3)
    _check(dev, monkeypatch, xs, pays, weights, w_selfs, DPZ_FOLD_SELF)


@pytest.mark.parametrize("n", [2_051, 1_024])
@pytest.mark.parametrize("self_term", [True, False])
def test_dense_payloads(dev, monkeypatch, n, self_term):
    """A dense payload first, in the middle, last, every payload of a node, none (a neighbour in
    the same launch), and node 5's dense payload being node 0's local row (JwinsBatchRound's
    layout on one rank)."""
    from decentralizepy_amd._lib import DPZ_FOLD_SELF
    rng = np.random.default_rng(n)
    g = torch.Generator().manual_seed(n)
    xs = [torch.randn(n, generator=g).numpy() for _ in range(6)]
    k = max(1, n // 5)

    def s():
        return _sparse(rng, n, k)

    def d():
        return None, rng.standard_normal(n).astype(np.float32)

    pays = [[d(), s(), s()], [s(), d(), s()], [s(), s(), d()], [d(), d()], [s(), s()],
            [s(), (None, xs[0]), s(), s(), s()]]
    ww = [_weights(len(p)) for p in pays]
    pl = _check(dev, monkeypatch, xs, pays, [w for w, _ in ww], [x for _, x in ww],
                DPZ_FOLD_SELF if self_term else 0, local_of={(5, 1): 0})
    assert pl["launches"] == 1


@pytest.mark.parametrize("counts", [(17, 2, 33, 16), (2, 95, 16, 17)])
@pytest.mark.parametrize("also_local", [False, True])
def test_more_than_16_payloads(dev, monkeypatch, counts, also_local):
    """Further launches continue the stored total; the self term and the copy over local come
    with a node's last 16 (an earlier copy would change the later terms: the oracle shows it)."""
    from decentralizepy_amd._lib import DPZ_FOLD_ALSO_LOCAL, DPZ_FOLD_SELF
    xs, pays, weights, w_selfs = _case(4, 4_100, 0.05, sum(counts), list(counts))
    pl = _check(dev, monkeypatch, xs, pays, weights, w_selfs,
                DPZ_FOLD_SELF | (DPZ_FOLD_ALSO_LOCAL if also_local else 0))
    assert pl["passes"] == -(-max(counts) // 16) and pl["launches"] == pl["passes"]


@pytest.mark.parametrize("counts", [(6, 6, 6), (33, 2, 5)])
@pytest.mark.parametrize("also_local", [False, True])
def test_guard(dev, counts, also_local):
    """A nonzero guard word: no launch of the call writes; all zero: the fold."""
    from decentralizepy_amd import _lib
    from decentralizepy_amd._lib import DPZ_FOLD_ALSO_LOCAL, DPZ_FOLD_SELF
    n = 4_100
    flags = DPZ_FOLD_SELF | (DPZ_FOLD_ALSO_LOCAL if also_local else 0)
    xs, pays, weights, w_selfs = _case(len(counts), n, 0.05, sum(counts), list(counts))
    locs = [torch.from_numpy(x).to(dev) for x in xs]
    dp = [[(torch.from_numpy(i).to(dev), torch.from_numpy(v).to(dev)) for i, v in p] for p in pays]
    outs = [torch.full((n,), 7.0, device=dev) for _ in counts]
    a = _args(locs, outs, dp, weights, w_selfs)
    guard = torch.zeros(70, dtype=torch.int32, device=dev)
    guard[69] = 3
    assert _guarded(_lib.lib(), a, flags, guard, dev) == 0
    for j in range(len(counts)):
        assert bool((outs[j] == 7.0).all())
        np.testing.assert_array_equal(locs[j].cpu().numpy().view(np.uint32), xs[j].view(np.uint32))
    guard.zero_()
    assert _guarded(_lib.lib(), a, flags, guard, dev) == 0
    for j in range(len(counts)):
        ref = ofold.fold(xs[j], pays[j], weights[j], w_selfs[j])
        np.testing.assert_array_equal(outs[j].cpu().numpy().view(np.uint32), ref.view(np.uint32))


def test_unaligned_row(dev):
    """One row 4 bytes off: the guarded entry refuses the batch and writes nothing;
    dpz_decode_average_batch folds it node after node."""
    from decentralizepy_amd import _lib
    from decentralizepy_amd._lib import DPZ_ERR_UNSUPPORTED, DPZ_FOLD_SELF
    n, counts = 4_100, [5, 6, 2]
    xs, pays, weights, w_selfs = _case(3, n, 0.05, 11, counts)
    locs = [torch.from_numpy(x).to(dev) for x in xs]
    off = torch.empty(n + 4, device=dev)
    off[1:n + 1] = locs[1]
    locs[1] = off[1:n + 1]
    assert locs[1].data_ptr() % 16 == 4
    dp = [[(torch.from_numpy(i).to(dev), torch.from_numpy(v).to(dev)) for i, v in p] for p in pays]
    outs = [torch.full((n,), float("nan"), device=dev) for _ in counts]
    a = _args(locs, outs, dp, weights, w_selfs)
    assert _plan(a, pays, DPZ_FOLD_SELF, aligned=0)["path"] == 0
    guard = torch.zeros(3, dtype=torch.int32, device=dev)
    assert _guarded(_lib.lib(), a, DPZ_FOLD_SELF, guard, dev) == DPZ_ERR_UNSUPPORTED
    assert all(bool(torch.isnan(o).all()) for o in outs)
    assert _batch(_lib.lib(), a, DPZ_FOLD_SELF, dev) == 0
    for j in range(3):
        ref = ofold.fold(xs[j], pays[j], weights[j], w_selfs[j])
        np.testing.assert_array_equal(outs[j].cpu().numpy().view(np.uint32), ref.view(np.uint32))
