"""GPU: the whole-topology Choco round.  ``dpz_choco_encode_nodes`` against the per-node
``codec.topk_threshold(x - x_hat)`` and the numpy restatement, ``dpz_choco_fold_nodes`` against
the restatement and the three-call sequence it replaces (DPZ_EW_ADD, the zero-based accumulating
``decode_average``, DPZ_EW_CHOCO), bit for bit, and the engine (decentralizepy_amd/
gossip_choco.py) against the runs recorded from the reference and the per-node plugin's device
sequence.  Sizes: one element, around a float4, the edges of the compaction chunk / the fold tile,
several of them with a ragged tail."""
import numpy as np
import pytest
import torch

from decentralizepy_amd.gossip_round import up4
from tests import choco_round_ops as ops
from tests.dist_harness import rccl_loopback
from tests.test_cpu_choco_round import RUN_IDS, RUNS, drive

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
HEADER = 4


def _rows(dev, data, aligned):
    """Device rows of the fp32 matrix ``data``: 16-byte aligned rows with prefilled padding, or
    packed rows (unaligned when the width is no multiple of 4).  Returns (view, backing)."""
    m, n = data.shape
    back = torch.full((m, up4(n) + 4 if aligned else n), 7.0, dtype=torch.float32, device=dev)
    back[:, :n] = torch.from_numpy(data).to(dev)
    return back[:, :n], back


def _count(row):
    return int(row[:2].view(torch.int64).item())


# ---- encode -------------------------------------------------------------------------------------
def _encode_data(n, k, C, seed):
    """4 nodes: random; x == x_hat; quantised (a handful of magnitudes, so the ties at T lie on
    both sides of every chunk edge) with exact zeros; fewer than k nonzero differences."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((4, n)).astype(np.float32)
    xh = (x + 0.1 * rng.standard_normal((4, n))).astype(np.float32)
    xh[1] = x[1]
    xh[2] = 0.0
    x[2] = (rng.integers(-5, 6, n) * np.float32(0.05)).astype(np.float32)
    if n > C:  # equal magnitudes, opposite signs, on the two sides of the first chunk edge
        x[2, C - 1], x[2, C] = 0.25, -0.25
    x[3] = xh[3]
    nz = rng.choice(n, size=min(n, k // 2), replace=False)
    x[3, nz] += np.float32(0.5)
    return x, xh


def _run_encode(dev, x, xh, k, cap, aligned):
    from decentralizepy_amd import codec
    m, n = x.shape
    tx, _ = _rows(dev, x, aligned)
    th, _ = _rows(dev, xh, aligned)
    rows = torch.full((m, HEADER + 2 * cap + 4), FILL, dtype=torch.int32, device=dev)
    codec.choco_encode_nodes(codec.choco_node_table(tx, th, rows), n, k, cap)
    return tx, th, rows


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "packed"])
@pytest.mark.parametrize("which", ["1", "3", "4", "5", "C-1", "C", "C+1", "3*C+37"])
def test_encode_nodes_equals_topk_threshold(dev, which, aligned):
    from decentralizepy_amd import codec
    C = codec.choco_chunk_elems()
    n = eval(which, {"C": C})
    ws = codec.Workspace(dev)
    for k in sorted({1, max(1, round(0.05 * n)), n}):
        x, xh = _encode_data(n, k, C, seed=n + k)
        cap = up4(n)
        tx, th, rows = _run_encode(dev, x, xh, k, cap, aligned)
        if not aligned and n % 4:
            assert tx[1].data_ptr() % 16
        got = rows.cpu().numpy()
        counts = []
        for j in range(4):
            err = str((n, k, j))
            idx, vals = ops.select(x[j], xh[j], k)
            c = _count(rows[j])
            counts.append(c)
            assert c == len(idx), err
            assert got[j, 2] == 0 and got[j, 3] == 0, err
            np.testing.assert_array_equal(got[j, HEADER:HEADER + c], idx, err_msg=err)
            np.testing.assert_array_equal(got[j, HEADER + cap:HEADER + cap + c],
                                          vals.view(np.int32), err_msg=err)
            # the rest of both slots and the words past the row: untouched
            assert (got[j, HEADER + c:HEADER + cap].view(np.uint32) == FILL).all(), err
            assert (got[j, HEADER + cap + c:].view(np.uint32) == FILL).all(), err
            ti, tv = codec.topk_threshold(tx[j].contiguous() - th[j].contiguous(), k,
                                          workspace=ws)
            np.testing.assert_array_equal(ti.cpu().numpy(), idx, err_msg=err)
            np.testing.assert_array_equal(ops.u32(tv.cpu().numpy()), ops.u32(vals), err_msg=err)
        assert counts[1] == 0 and counts[3] == min(n, k // 2) and counts[0] >= k
        if n > C:
            assert k == n or counts[2] > k  # the ties (k == n: T = 0, the zeros stay home)
            sel = got[2, HEADER:HEADER + counts[2]]
            assert C - 1 in sel and C in sel  # the largest magnitude, on both sides of the edge


def test_encode_overflow_is_reported_not_truncated(dev):
    from decentralizepy_amd import codec
    C = codec.choco_chunk_elems()
    n, k, cap = C + 1, 100, 64
    x, xh = _encode_data(n, k, C, seed=5)
    _, _, rows = _run_encode(dev, x, xh, k, cap, True)
    got = rows.cpu().numpy()
    want = [ops.select(x[j], xh[j], k) for j in range(4)]
    counts = [len(i) for i, _ in want]
    assert counts[0] >= k > cap and counts[2] > cap and counts[1] == 0 and counts[3] == 50
    assert [_count(rows[j]) for j in range(4)] == counts
    assert got[:, 2].tolist() == [1, 0, 1, 0] and not got[:, 3].any()
    for j, (idx, vals) in enumerate(want):
        c = min(counts[j], cap)
        np.testing.assert_array_equal(got[j, HEADER:HEADER + c], idx[:c])
        np.testing.assert_array_equal(got[j, HEADER + cap:HEADER + cap + c],
                                      vals[:c].view(np.int32))
        assert (got[j, HEADER + c:HEADER + cap].view(np.uint32) == FILL).all()
        assert (got[j, HEADER + cap + c:].view(np.uint32) == FILL).all()  # past val + cap too


# ---- fold ---------------------------------------------------------------------------------------
LISTS = [0, 1, 4, 17]
TINY = 1e-40  # a subnormal fp32 weight: products of ordinary values are subnormal or zero


def _fold_case(n, T, seed=9):
    """18 payloads and 4 receivers with lists of 0, 1, 4 and 17 of them.  Payload 0 is empty,
    payload 1 lies wholly inside one tile, payload 2 names the first and last element of every
    tile, payloads 3, 4 and 5 meet on one index with values whose sum depends on the order."""
    rng = np.random.default_rng(seed)
    pays = []
    for p in range(18):
        if p == 0:
            idx = np.zeros(0, np.int64)
        elif p == 1:
            lo = min(T + 5, n - 1) if n > T + 5 else 0
            idx = np.arange(lo, min(lo + 45, n))
        elif p == 2:
            edges = [e for t in range(0, n, T) for e in (t, min(t + T, n) - 1)]
            idx = np.unique(np.array(edges + [n - 1]))
        elif p == 6:  # every element: the tiny-weight receiver's only payload
            idx = np.arange(n)
        else:
            idx = np.sort(rng.choice(n, size=max(1, int(n * rng.uniform(0.01, 0.3))),
                                     replace=False))
        vals = rng.standard_normal(len(idx)).astype(np.float32)
        vals[vals == 0] = 1.0
        pays.append([idx.astype(np.int32), vals])
    j0 = n // 2
    for p, v in ((3, 3e7), (4, -3e7), (5, 1.0)):  # (s + a) + b) + c != (s + c) + b) + a
        idx, vals = pays[p]
        if j0 not in idx:
            pos = np.searchsorted(idx, j0)
            idx, vals = np.insert(idx, pos, j0), np.insert(vals, pos, 0).astype(np.float32)
        vals[np.searchsorted(idx, j0)] = v
        pays[p] = [idx.astype(np.int32), vals]
    x = rng.standard_normal((4, n)).astype(np.float32)
    xh = rng.standard_normal((4, n)).astype(np.float32)
    s = rng.standard_normal((4, n)).astype(np.float32)
    s[1, ::2] = 0.0  # receiver 1 has the tiny weight: subnormal results where s was +0
    s[2, j0] = 0.25
    lists = [[], [6], [3, 4, 5, 2], list(range(1, 18))]
    weights = [[], [TINY], [0.25, 0.25, 0.25, 0.125], [float(w) for w in
                                                       rng.uniform(0.01, 0.05, 17)]]
    own = [7, 0, 1, 2]  # the receivers' own payloads: ordinary, empty, in one tile, tile edges
    w_self = [1.0, 1.0 - TINY, 0.125, 1.0 - sum(weights[3])]
    return pays, x, xh, s, lists, weights, own, w_self, j0


def _expected(case, step, reverse=False):
    pays, x, xh, s, lists, weights, own, w_self, _ = case
    x, xh, s = x.copy(), xh.copy(), s.copy()
    for r in range(4):
        lst = [(pays[p][0], pays[p][1], w) for p, w in zip(lists[r], weights[r])]
        ops.fold(x[r], xh[r], s[r], pays[own[r]], w_self[r], lst[::-1] if reverse else lst, step)
    return x, xh, s


def _device_case(dev, case, aligned=True):
    from decentralizepy_amd import codec
    pays, x, xh, s, lists, weights, own, w_self, _ = case
    cap = up4(max(len(i) for i, _ in pays)) + 4
    rows = torch.full((len(pays), HEADER + 2 * cap), FILL, dtype=torch.int32, device=dev)
    host = rows.cpu().numpy()
    for p, (idx, vals) in enumerate(pays):  # the slots past the count keep the fill: never read
        host[p, :4] = (len(idx), 0, 0, 0)
        host[p, HEADER:HEADER + len(idx)] = idx
        host[p, HEADER + cap:HEADER + cap + len(idx)] = vals.view(np.int32)
    rows.copy_(torch.from_numpy(host))
    state = [_rows(dev, a, aligned) for a in (x, xh, s)]
    (tx, _), (th, _), (ts, _) = state
    recvs = [(tx[r], th[r], ts[r], rows[own[r]], cap, w_self[r],
              [(rows[p], cap, w) for p, w in zip(lists[r], weights[r])]) for r in range(4)]
    return codec.ChocoTable(recvs, dev), rows, cap, state


def _assert_state(state, want, n, err):
    for (view, back), w, name in zip(state, want, ("x", "x_hat", "s")):
        np.testing.assert_array_equal(ops.u32(view.cpu().numpy()), ops.u32(w),
                                      err_msg=f"{name} {err}")
        assert (back[:, n:] == 7.0).all(), f"padding of {name} {err}"


@pytest.mark.parametrize("which", ["1", "3", "4", "T-1", "T", "T+1", "3*T+37"])
def test_fold_nodes_equals_restatement_and_three_calls(dev, which):
    from decentralizepy_amd import codec
    T = codec.choco_tile_elems()
    n = eval(which, {"T": T})
    step = 0.3
    case = _fold_case(n, T)
    pays, x, xh, s, lists, weights, own, w_self, j0 = case
    want = _expected(case, step)
    # the inputs hold what the case is about
    assert [len(lst) for lst in lists] == LISTS and len(pays[0][0]) == 0
    assert all(j0 in pays[p][0] for p in (3, 4, 5))
    assert _expected(case, step, reverse=True)[2][2, j0] != want[2][2, j0]  # order-sensitive
    sub = (want[2][1] != 0) & (np.abs(want[2][1]) < np.finfo(np.float32).tiny)
    assert sub.any()  # subnormal results occur
    if n > T:
        assert {0, T - 1, T, n - 1} <= set(pays[2][0].tolist())
        assert pays[1][0].min() // T == pays[1][0].max() // T  # wholly inside one tile
    tab, rows, cap, state = _device_case(dev, case)
    guard = torch.zeros(6, dtype=torch.int32, device=dev)
    guard[4] = 1
    codec.choco_fold_nodes(tab, n, step, guard=guard)
    _assert_state(state, (x, xh, s), n, "behind a nonzero guard word: nothing written")
    guard.zero_()
    codec.choco_fold_nodes(tab, n, step, guard=guard)
    _assert_state(state, want, n, str(n))
    assert (ops.u32(state[2][0][1].cpu().numpy()) == ops.u32(want[2][1]))[sub].all()
    # the three calls this launch replaces, on the same inputs
    ws = codec.Workspace(dev)
    for r in range(1, 4):
        tx, th, ts = (torch.from_numpy(a[r].copy()).to(dev) for a in (x, xh, s))
        q = torch.zeros(n, dtype=torch.float32, device=dev)
        qi, qv = (torch.from_numpy(a).to(dev) for a in pays[own[r]])
        q[qi.long()] = qv
        codec.elementwise(codec.DPZ_EW_ADD, th, q, out=th)
        dp = [(torch.from_numpy(pays[p][0]).to(dev), torch.from_numpy(pays[p][1]).to(dev))
              for p in lists[r]]
        codec.decode_average(q, dp, weights[r], w_self[r], out=ts, zero_base=True,
                             accumulate=True, workspace=ws)
        codec.elementwise(codec.DPZ_EW_CHOCO, tx, ts, th, step, out=tx)
        for got, w, name in zip((tx, th, ts), want, ("x", "x_hat", "s")):
            np.testing.assert_array_equal(ops.u32(got.cpu().numpy()), ops.u32(w[r]),
                                          err_msg=f"three calls, {name} of receiver {r}")


def test_fold_nodes_packed_rows_and_no_guard(dev):
    from decentralizepy_amd import codec
    T = codec.choco_tile_elems()
    n = T + 1
    case = _fold_case(n, T, seed=10)
    tab, rows, cap, state = _device_case(dev, case, aligned=False)
    assert state[0][0][1].data_ptr() % 16
    before = rows.clone()
    codec.choco_fold_nodes(tab, n, 0.5)
    for (view, _), w, name in zip(state, _expected(case, 0.5), ("x", "x_hat", "s")):
        np.testing.assert_array_equal(ops.u32(view.cpu().numpy()), ops.u32(w), err_msg=name)
    assert torch.equal(rows, before)  # the payload rows are only read


# ---- the engine ---------------------------------------------------------------------------------
@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_engine_reproduces_the_reference(dev, meta, arr):
    from decentralizepy_amd.gossip_choco import ChocoRound
    eng = ChocoRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]).to(dev), meta["alpha"],
                     meta["step_size"], slot_cap=meta["slot_cap"])
    assert eng.x.is_cuda and eng.x[1].data_ptr() % 16 == 0
    drive(eng, meta, arr)


def test_engine_small_slot_is_reported_and_changes_no_state(dev):
    from decentralizepy_amd.gossip_choco import ChocoRound
    meta, arr = RUNS[RUN_IDS.index("irr6")]
    x0 = np.stack([ops.train(arr["x0"][u], meta, 0, u) for u in range(6)])
    eng = ChocoRound(ops.run_adjacency(meta), torch.from_numpy(x0).to(dev), meta["alpha"],
                     meta["step_size"], slot_cap=meta["k"])
    eng.step()
    over = [u for u in range(6) if arr["counts"][0][u] > eng.cap]
    with pytest.raises(RuntimeError, match=str(over).replace("[", r"\[").replace("]", r"\]")):
        eng.check()
    np.testing.assert_array_equal(ops.u32(eng.x.cpu().numpy()), ops.u32(x0))
    assert not eng.x_hat.any() and not eng.s.any()


def test_step_launch_count_is_independent_of_the_node_count(dev):
    from decentralizepy_amd import codec
    from decentralizepy_amd.gossip_choco import ChocoRound
    seen = []
    for meta, arr in RUNS:  # 16 and 6 nodes
        eng = ChocoRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]).to(dev),
                         meta["alpha"], meta["step_size"], slot_cap=meta["slot_cap"])
        eng.step()  # builds the tables
        with codec.KernelTimer() as t:
            eng.step()
        seen.append({name: cnt for name, (_, cnt) in t.result.items()})
    assert seen[0] == seen[1] == {"topk_exact_hist": 3, "topk_exact_resolve": 3,
                                  "topk_exact_count": 1, "topk_exact_scan": 1,
                                  "topk_exact_write": 1, "fold": 1}


@pytest.fixture
def rccl_group(dev):
    with rccl_loopback(dev) as group:
        yield group


def test_engine_through_rccl_equals_in_place(dev, rccl_group):
    from decentralizepy_amd.gossip_choco import ChocoRound
    meta, arr = RUNS[RUN_IDS.index("irr6")]
    eng = ChocoRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]).to(dev), meta["alpha"],
                     meta["step_size"], rank=0, world=1, group=rccl_group,
                     slot_cap=meta["slot_cap"])
    assert eng.coll and eng.recv is not None
    drive(eng, meta, arr, every_payload=True)


def _plugin_round(x, x_hat, s, adj, k, step, ws):
    """A round of every node through the per-node plugin's device sequence
    (decentralizepy_amd/sharing/Choco.py: _pre_step, then _averaging)."""
    from decentralizepy_amd import codec
    qs = []
    for u in range(len(adj)):
        d = codec.elementwise(codec.DPZ_EW_SUB, x[u], x_hat[u])
        idx, vals = codec.topk_threshold(d, k, workspace=ws)
        qs.append((idx.clone(), vals.clone(), codec.mask_below_threshold(d, ws)))
    for u in range(len(adj)):
        nbrs, w, w_self = ops.mh(adj, u)
        codec.elementwise(codec.DPZ_EW_ADD, x_hat[u], qs[u][2], out=x_hat[u])
        codec.decode_average(qs[u][2], [qs[v][:2] for v in nbrs], w, w_self, out=s[u],
                             zero_base=True, accumulate=True, workspace=ws)
        codec.elementwise(codec.DPZ_EW_CHOCO, x[u], s[u], x_hat[u], step, out=x[u])
    return [len(q[0]) for q in qs]


def test_engine_equals_the_plugin_sequence_on_96_regular(dev):
    import os

    from decentralizepy_amd import codec
    from decentralizepy_amd.gossip import read_edges
    from decentralizepy_amd.gossip_choco import ChocoRound
    adj = read_edges(os.path.join(ops.GOLDEN, "96_regular.edges"))
    n, alpha, step = 4099, 0.01, 0.4
    g = torch.Generator().manual_seed(12)
    x0 = torch.randn(96, n, generator=g)
    eng = ChocoRound(adj, x0.to(dev), alpha, step)
    x = [x0[u].to(dev) for u in range(96)]
    x_hat = [torch.zeros(n, device=dev) for _ in range(96)]
    s = [torch.zeros(n, device=dev) for _ in range(96)]
    ws = codec.Workspace(dev)
    for r in range(2):
        noise = 0.01 * torch.randn(96, n, generator=g)
        eng.x.add_(noise.to(dev))
        for u in range(96):
            x[u].add_(noise[u].to(dev))
        counts = _plugin_round(x, x_hat, s, adj, eng.k, step, ws)
        eng.step()
        eng.check()
        assert [eng.payload(q)[0].numel() for q in range(0, 96, 19)] == counts[::19]
        for name, got, want in (("x", eng.x, x), ("x_hat", eng.x_hat, x_hat), ("s", eng.s, s)):
            np.testing.assert_array_equal(ops.u32(got.cpu().numpy()),
                                          ops.u32(torch.stack(want).cpu().numpy()),
                                          err_msg=f"{name} round {r}")
