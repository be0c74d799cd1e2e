"""GPU: the whole-federation STC round.  ``dpz_stc_encode_nodes`` against the numpy restatement
(tests/stc_round_ops.py) and the single-node ``codec.topk_encode`` on its exact path with the
residual as the accumulator, ``dpz_stc_server_fold`` against the restatement and the per-node
plugin's two ``decode_average`` calls, ``dpz_stc_apply_nodes`` against the restatement, bit for
bit, and the engine (decentralizepy_amd/gossip_stc.py) against the runs recorded from the
reference and against ``decentralizepy_amd.sharing.STC`` plugin objects driven node by node.
Sizes: one element, around a float4, the edges of the compaction chunk / the fold tile, several of
them with a ragged tail."""
from collections import OrderedDict, deque

import numpy as np
import pytest
import torch

from decentralizepy_amd.gossip_round import up4
from tests import scenario
from tests import stc_round_ops as ops
from tests.dist_harness import rccl_loopback
from tests.test_cpu_stc_round import RUN_IDS, RUNS, drive, run_named

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
HEADER = 4
PAD = 7.0


def _rows(dev, data, aligned):
    """Device rows of the fp32 matrix ``data``: 16-byte aligned rows with prefilled padding, or
    packed rows (unaligned when the width is no multiple of 4).  Returns (view, backing)."""
    m, n = data.shape
    back = torch.full((m, up4(n) + 4 if aligned else n), PAD, dtype=torch.float32, device=dev)
    back[:, :n] = torch.from_numpy(data).to(dev)
    return back[:, :n], back


def _packed_rows(pays, k, dev, extra=4):
    """Packed rows ``[k, 0, 0, 0 | up4(k) idx | up4(k) vals]`` of the payloads, the slots past k
    and ``extra`` words past each row prefilled."""
    cap = up4(k)
    host = np.full((len(pays), HEADER + 2 * cap + extra), FILL, dtype=np.uint32).view(np.int32)
    for p, (idx, vals) in enumerate(pays):
        host[p, :4] = (len(idx), 0, 0, 0)
        host[p, HEADER:HEADER + len(idx)] = idx
        host[p, HEADER + cap:HEADER + cap + len(idx)] = vals.view(np.int32)
    return torch.from_numpy(host).to(dev)


# ---- encode -------------------------------------------------------------------------------------
QUANT_P = np.array([0.04] + [0.92 / 9] * 9 + [0.04])  # of -5 .. 5: the top magnitude is rare


def _encode_data(n, k, C, seed):
    """5 nodes (x, prev, r): random; x == prev with r == 0 (every key equal); quantised (a handful
    of magnitudes, +-0.25 on the two sides of the first chunk edge); fewer than k nonzero changes;
    the server form (x and prev absent, r holds c)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((5, n)).astype(np.float32)
    prev = (x + 0.1 * rng.standard_normal((5, n))).astype(np.float32)
    r = (0.05 * rng.standard_normal((5, n))).astype(np.float32)
    prev[1], r[1] = x[1], 0.0
    x[2] = (rng.choice(np.arange(-5, 6), size=n, p=QUANT_P) * np.float32(0.05)).astype(np.float32)
    prev[2], r[2] = 0.0, 0.0
    if n > C:
        x[2, C - 1], x[2, C] = 0.25, -0.25
    x[3], r[3] = prev[3], 0.0
    nz = rng.choice(n, size=min(n, k // 2), replace=False)
    x[3, nz] += np.float32(0.5)
    return x, prev, r


def _expected_encode(x, prev, r, k):
    prev, r = prev.copy(), r.copy()
    pays = [ops.encode(None if j == 4 else x[j], None if j == 4 else prev[j], r[j], k)
            for j in range(5)]
    return pays, prev, r


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "packed"])
@pytest.mark.parametrize("which", ["1", "3", "4", "5", "C-1", "C", "C+1", "3*C+37"])
def test_encode_nodes_equals_restatement_and_topk_encode(dev, which, aligned):
    from decentralizepy_amd import codec
    C = codec.stc_chunk_elems()
    n = eval(which, {"C": C})
    ws = codec.Workspace(dev)
    for k in sorted({1, max(1, round(0.05 * n)), n}):
        err = str((n, k))
        x, prev, r = _encode_data(n, k, C, seed=n + k)
        pays, want_prev, want_r = _expected_encode(x, prev, r, k)
        if n > C and k < n:
            # the quantised node's input is what the tie allotment needs (k == n selects every
            # element: no tie can be left): the k-th key ties, the run lies in at least two
            # chunks, some of it is taken and some left
            run, taken = ops.tie_run(x[2], k)
            assert len(run) > 1 and len(np.unique(run // C)) >= 2, err
            assert 0 < taken < len(run), err
            if which == "3*C+37" and k > 1:  # the taken ties themselves span a chunk edge
                assert run[taken - 1] >= C and run[0] < C, err
        assert (pays[1][0] == np.arange(k)).all()  # equal keys: the lowest k indices win
        tx, bx = _rows(dev, x, aligned)
        tp, bp = _rows(dev, prev, aligned)
        tr, br = _rows(dev, r, aligned)
        if not aligned and n % 4:
            assert tr[1].data_ptr() % 16
        cap = up4(k)
        rows = torch.from_numpy(np.full((5, HEADER + 2 * cap + 4), FILL, dtype=np.uint32)
                                .view(np.int32)).to(dev)
        xs = [tx[j] for j in range(4)] + [None]
        ps = [tp[j] for j in range(4)] + [None]
        tab = codec.stc_node_table(xs, ps, tr, rows)
        codec.stc_encode_nodes(tab, n, k)
        got = rows.cpu().numpy()
        for j, (idx, vals) in enumerate(pays):
            e = f"{err} node {j}"
            assert got[j, :4].tolist() == [k, 0, 0, 0], e
            np.testing.assert_array_equal(got[j, HEADER:HEADER + k], idx, err_msg=e)
            np.testing.assert_array_equal(got[j, HEADER + cap:HEADER + cap + k],
                                          vals.view(np.int32), err_msg=e)
            # the rest of both slots and the words past the row: untouched
            assert (got[j, HEADER + k:HEADER + cap].view(np.uint32) == FILL).all(), e
            assert (got[j, HEADER + cap + k:].view(np.uint32) == FILL).all(), e
        np.testing.assert_array_equal(ops.u32(tr.cpu().numpy()), ops.u32(want_r), err_msg=err)
        np.testing.assert_array_equal(ops.u32(tp.cpu().numpy()), ops.u32(want_prev), err_msg=err)
        np.testing.assert_array_equal(ops.u32(tx.cpu().numpy()), ops.u32(x), err_msg=err)
        assert (want_prev[:4] == x[:4]).all() and (want_prev[4] == prev[4]).all()
        for back in (bx, bp, br):
            assert (back[:, n:] == PAD).all(), f"padding {err}"
        # the single-node encode on its exact path, the residual as the accumulator
        for j in range(4):
            sx, sp, sr = (torch.from_numpy(a[j].copy()).to(dev) for a in (x, prev, r))
            si, sv = codec.topk_encode(sx, k, x0=sp, acc=sr, acc_mode=codec.DPZ_ACC_ACCUMULATE,
                                       vals_src=sr, workspace=ws, exact=True)
            e = f"{err} topk_encode node {j}"
            np.testing.assert_array_equal(si.cpu().numpy(), pays[j][0], err_msg=e)
            np.testing.assert_array_equal(ops.u32(sv.cpu().numpy()), ops.u32(pays[j][1]),
                                          err_msg=e)
            np.testing.assert_array_equal(ops.u32(sr.cpu().numpy()), ops.u32(want_r[j]),
                                          err_msg=e)
        sc = torch.from_numpy(r[4].copy()).to(dev)  # the plugin's server_broadcast
        si, sv = codec.topk_encode(sc, k, vals_src=sc, workspace=ws, exact=True)
        codec.scatter_fill(sc, si, 0.0)
        np.testing.assert_array_equal(si.cpu().numpy(), pays[4][0], err_msg=err)
        np.testing.assert_array_equal(ops.u32(sv.cpu().numpy()), ops.u32(pays[4][1]), err_msg=err)
        np.testing.assert_array_equal(ops.u32(sc.cpu().numpy()), ops.u32(want_r[4]), err_msg=err)


# ---- server fold --------------------------------------------------------------------------------
def _fold_case(n, P, k, seed):
    """P payloads of k ascending entries.  With P >= 3 payloads 0, 1 and 2 meet on one index with
    values whose fp32 sum depends on the order; with k >= 3 the last payload holds a value whose
    product with the weight is subnormal and a negative one whose product underflows to -0."""
    rng = np.random.default_rng(seed)
    j0 = n // 2
    w = 1.0 / P if P > 1 else 0.5
    pays = []
    for p in range(P):
        if k == n:
            idx = np.arange(n)
        elif p < 3:
            others = np.delete(np.arange(n), j0)
            idx = np.sort(np.append(rng.choice(others, size=k - 1, replace=False), j0))
        else:
            idx = np.sort(rng.choice(n, size=k, replace=False))
        vals = rng.standard_normal(k).astype(np.float32)
        vals[vals == 0] = 1.0
        pays.append((idx.astype(np.int32), vals))
    if P >= 3:
        for p, v in ((0, 3e7), (1, -3e7), (2, 1.0)):
            pays[p][1][np.searchsorted(pays[p][0], j0)] = v
    special = None
    if k >= 3:
        idx, vals = pays[P - 1]
        free = [e for e in range(k) if idx[e] != j0]
        vals[free[0]], vals[free[-1]] = 2e-38, -1e-45
        special = (idx[free[0]], idx[free[-1]])
    r_s = rng.standard_normal(n).astype(np.float32)
    r_s[::3] = 0.0
    r_s[1::7] = -0.0
    return pays, w, r_s, j0, special


@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("which", ["1", "5", "T-1", "T", "T+1", "3*T+37"])
def test_server_fold_equals_restatement_and_two_calls(dev, which, dense):
    from decentralizepy_amd import codec
    T = codec.stc_tile_elems()
    n = eval(which, {"T": T})
    k = n if dense else max(1, round(0.1 * n))
    ws = codec.Workspace(dev)
    for P in (1, 3, 8, 9, 17):
        err = str((n, k, P))
        pays, w, r_s, j0, special = _fold_case(n, P, k, seed=n + P)
        want = r_s.copy()
        total = ops.server_fold(want, pays, w)
        assert not np.signbit(total[total == 0]).any()
        if P >= 3:  # the inputs hold what the case is about
            assert all(j0 in pays[p][0] for p in range(3))
            rev = r_s.copy()
            assert ops.server_fold(rev, pays[::-1], w)[j0] != total[j0], err
        if special is not None:
            a, b = (np.float32(v) * np.float32(w) for v in (2e-38, -1e-45))
            assert 0 < a < np.finfo(np.float32).tiny and b == 0 and np.signbit(b), err
        rows = _packed_rows(pays, k, dev)
        before = rows.clone()
        tr, br = _rows(dev, r_s[None, :], True)
        tab = codec.StcFoldTable([(rows[p], w) for p in range(P)], dev)
        codec.stc_server_fold(tab, n, k, tr[0])
        np.testing.assert_array_equal(ops.u32(tr[0].cpu().numpy()), ops.u32(want), err_msg=err)
        assert (br[:, n:] == PAD).all() and torch.equal(rows, before), err
        # the plugin's two calls on the same inputs
        sr = torch.from_numpy(r_s).to(dev)
        dp = [(torch.from_numpy(i).to(dev), torch.from_numpy(v).to(dev)) for i, v in pays]
        tot = codec.decode_average(sr, dp, [w] * P, None, zero_base=True, workspace=ws)
        np.testing.assert_array_equal(ops.u32(tot.cpu().numpy()), ops.u32(total), err_msg=err)
        change = codec.decode_average(sr, [(None, tot)], [1.0], 1.0, workspace=ws)
        np.testing.assert_array_equal(ops.u32(change.cpu().numpy()), ops.u32(want), err_msg=err)


def test_server_fold_unaligned_residual_and_skipped_indices(dev):
    """r_s at an address that is no multiple of 16, and a payload whose first and last entries
    lie outside [0, n): they are skipped, the words around r_s stay untouched."""
    from decentralizepy_amd import codec
    T = codec.stc_tile_elems()
    n, k, P = T + 3, 50, 3
    pays, w, r_s, _, _ = _fold_case(n, P, k, seed=77)
    want = r_s.copy()
    inside = [(i[1:-1], v[1:-1]) for i, v in pays[:1]] + pays[1:]
    ops.server_fold(want, inside, w)
    pays[0][0][0], pays[0][0][-1] = -3, n + 2  # still ascending
    rows = _packed_rows(pays, k, dev)
    back = torch.full((n + 9,), PAD, dtype=torch.float32, device=dev)
    tr = back[5:5 + n]
    tr.copy_(torch.from_numpy(r_s))
    assert tr.data_ptr() % 16
    codec.stc_server_fold(codec.StcFoldTable([(rows[p], w) for p in range(P)], dev), n, k, tr)
    np.testing.assert_array_equal(ops.u32(tr.cpu().numpy()), ops.u32(want))
    assert (back[:5] == PAD).all() and (back[5 + n:] == PAD).all()


# ---- apply --------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "packed"])
@pytest.mark.parametrize("n", [1, 5, 4099])
def test_apply_nodes_in_place_keeps_unnamed_bits(dev, n, aligned):
    """The pinned deviation: an element the broadcast does not name keeps its bits, a -0.0 too
    (the reference's dense flat + T gives +0.0 there); a named -0.0 gets fl(-0 + val)."""
    from decentralizepy_amd import codec
    rng = np.random.default_rng(n)
    k = max(1, n // 10)
    x = rng.standard_normal((4, n)).astype(np.float32)
    idx = np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32)
    vals = rng.standard_normal(k).astype(np.float32)
    x[:, ::3] = -0.0
    if k > 1:
        x[:, idx[0]] = -0.0
        vals[0] = -0.0  # -0 + -0 = -0
    want = x.copy()
    for j in range(4):
        ops.apply(want[j], idx, vals)
    unnamed = np.setdiff1d(np.arange(n), idx)
    np.testing.assert_array_equal(ops.u32(want[:, unnamed]), ops.u32(x[:, unnamed]))
    if n > 1:
        assert np.signbit(want[:, unnamed][want[:, unnamed] == 0]).any()
    tx, bx = _rows(dev, x, aligned)
    row = _packed_rows([(idx, vals)], k, dev)
    before = row.clone()
    codec.stc_apply_nodes(codec.stc_apply_table(tx), n, k, row[0])
    np.testing.assert_array_equal(ops.u32(tx.cpu().numpy()), ops.u32(want))
    assert (bx[:, n:] == PAD).all() and torch.equal(row, before)
    if n > 1:  # indices outside [0, n) are skipped
        idx2 = idx.copy()
        idx2[0] = -1
        idx2[-1] = n if k > 1 else -1
        row2 = _packed_rows([(idx2, vals)], k, dev)
        want2 = want.copy()
        for j in range(4):
            ops.apply(want2[j], idx2[1:-1], vals[1:-1])
        codec.stc_apply_nodes(codec.stc_apply_table([tx[j] for j in range(4)]), n, k, row2[0])
        np.testing.assert_array_equal(ops.u32(tx.cpu().numpy()), ops.u32(want2))
        assert (bx[:, n:] == PAD).all()


# ---- the engine ---------------------------------------------------------------------------------
def _device_engine(dev, meta, arr, **kw):
    from decentralizepy_amd.gossip_stc import StcRound
    return StcRound(meta["clients"], torch.from_numpy(arr["x0"]).to(dev),
                    torch.from_numpy(arr["xs0"]).to(dev), meta["alpha"], **kw)


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_engine_reproduces_the_reference(dev, meta, arr):
    eng = _device_engine(dev, meta, arr)
    assert eng.x.is_cuda and eng.x[1].data_ptr() % 16 == 0 and eng.server_r.data_ptr() % 16 == 0
    drive(eng, meta, arr)


def test_step_launch_count_is_independent_of_the_client_count(dev):
    from decentralizepy_amd import codec
    seen = []
    for meta, arr in RUNS:  # 8 and 6 clients
        eng = _device_engine(dev, meta, arr)
        eng.step()  # builds the tables
        with codec.KernelTimer() as t:
            eng.step()
        seen.append({name: cnt for name, (_, cnt) in t.result.items()})
    assert seen[0] == seen[1] == {"topk_exact_hist": 6, "topk_exact_resolve": 6,
                                  "topk_exact_count": 2, "topk_exact_scan": 2,
                                  "topk_exact_write": 2, "fold": 1, "scatter_fill": 1}


@pytest.fixture
def rccl_group(dev):
    with rccl_loopback(dev) as group:
        yield group


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_engine_through_rccl_equals_the_reference(dev, rccl_group, meta, arr):
    eng = _device_engine(dev, meta, arr, rank=0, world=1, group=rccl_group)
    assert eng.coll and eng.recv is not None
    drive(eng, meta, arr, every_payload=True)


def test_engine_equals_the_plugin_objects_node_by_node(dev, tmp_path):
    """decentralizepy_amd.sharing.STC objects, one per client and one for the server, driven as
    STCClient / STCServer drive them, against the engine on the same inputs, bit for bit."""
    from decentralizepy_amd.sharing.STC import STC
    meta, arr = run_named("part6")
    nc, n = meta["clients"], meta["n"]
    kw = dict(alpha=meta["alpha"], compress=False, compression_package=None,
              compression_class=None)
    models = [scenario.make_model(meta["shape"]) for _ in range(nc + 1)]
    for u in range(nc):
        scenario.set_flat(models[u], arr["x0"][u])
    scenario.set_flat(models[nc], arr["xs0"])
    clients = [STC(u, 0, None, scenario._Mapping(nc + 1), scenario._Graph([nc]), models[u], None,
                   str(tmp_path), **kw) for u in range(nc)]
    server = STC(nc, 0, None, scenario._Mapping(nc + 1), scenario._Graph(range(nc)), models[nc],
                 None, str(tmp_path), **kw)
    eng = _device_engine(dev, meta, arr)
    for c in clients:
        c.process_received(None)
    sets = [[5, 0, 3], [1, 2, 3, 4], [2, 5], [0, 1, 2, 3, 4, 5], [4]]
    for r, workers in enumerate(sets):
        peers = OrderedDict()
        x = eng.x.cpu().numpy()
        for u in workers:
            new = (x[u] + ops.perturbation(900, r, u, n)).astype(np.float32)
            x[u] = new
            scenario.set_flat(models[u], new)
            data = clients[u].get_data_to_send()
            peers[u] = deque([dict(data, degree=1, CHANNEL="STC")])
        eng.x.copy_(torch.from_numpy(x).to(dev))
        eng.step(workers)
        for u in workers:
            idx, vals = eng.payload(u)
            msg = peers[u][0]
            np.testing.assert_array_equal(idx.cpu().numpy(), msg["indices"])
            np.testing.assert_array_equal(ops.u32(vals.cpu().numpy()), ops.u32(msg["params"]))
        server._averaging_server(peers)
        b = server.server_broadcast()
        bi, bv = eng.broadcast()
        np.testing.assert_array_equal(bi.cpu().numpy(), b["indices"])
        np.testing.assert_array_equal(ops.u32(bv.cpu().numpy()), ops.u32(b["params"]))
        for u in workers:
            clients[u].process_received({"alpha": b["alpha"], "indices": b["indices"].copy(),
                                         "params": b["params"].copy()})
        err = f"round {r}"
        np.testing.assert_array_equal(
            ops.u32(eng.x.cpu().numpy()),
            ops.u32(np.stack([scenario.get_flat(m) for m in models[:nc]])), err_msg=err)
        np.testing.assert_array_equal(ops.u32(eng.server_x.cpu().numpy()),
                                      ops.u32(scenario.get_flat(models[nc])), err_msg=err)
        np.testing.assert_array_equal(
            ops.u32(eng.r.cpu().numpy()),
            ops.u32(torch.stack([c.residuals for c in clients]).cpu().numpy()), err_msg=err)
        np.testing.assert_array_equal(
            ops.u32(eng.prev.cpu().numpy()),
            ops.u32(torch.stack([c.prev_model for c in clients]).cpu().numpy()), err_msg=err)
        np.testing.assert_array_equal(ops.u32(eng.server_r.cpu().numpy()),
                                      ops.u32(server.residuals.cpu().numpy()), err_msg=err)
