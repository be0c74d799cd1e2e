"""GPU: the whole-topology top-k round with accumulated changes.  ``dpz_topkacc_encode_nodes``
against the numpy restatement (tests/topkacc_round_ops.py) and the single-node
``codec.topk_encode`` on its exact path with the accumulator and the counter,
``dpz_topkacc_post_nodes`` against numpy, bit for bit, and the engine
(decentralizepy_amd/gossip_topkacc.py) against the runs recorded from the reference and against
``decentralizepy_amd.sharing.PartialModel`` plugin objects driven node by node.  Sizes: one
element, around a float4, the edges of the compaction chunk, several chunks with a ragged tail;
rows 16-byte aligned and 4 bytes off."""
from collections import deque

import numpy as np
import pytest
import torch

from decentralizepy_amd.gossip_round import up4
from tests import scenario
from tests import topkacc_round_ops as ops
from tests.dist_harness import rccl_loopback
from tests.test_cpu_topkacc_round import RUN_IDS, RUNS, _engine, drive, run_named

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
HEADER = 4
PAD = 7.0
SIZES = ["1", "3", "4", "5", "1025", "2047", "C-1", "C", "C+1", "3*C+37"]
# of -5 .. 5: the top magnitude holds 14 % of the elements, more than the 10 % a selection takes,
# so the k-th key ties at it wherever the elements lie
QUANT_P = np.array([0.07] + [0.86 / 9] * 9 + [0.07])


def _rows(dev, data, aligned, dtype=torch.float32, pad=PAD):
    """Device rows of the matrix ``data``, the words around them prefilled: every row 16-byte
    aligned, or every row 4 bytes past a 16-byte boundary.  Returns (view, backing)."""
    m, n = data.shape
    off = 0 if aligned else 1
    back = torch.full((m, up4(n) + 8), pad, dtype=dtype, device=dev)
    view = back[:, off:off + n]
    view.copy_(torch.from_numpy(data).to(dev))
    assert all(view[j].data_ptr() % 16 == 4 * off for j in range(m))
    return view, back


def _padding_intact(back, n, aligned, pad=PAD):
    off = 0 if aligned else 1
    return bool((back[:, :off] == pad).all() and (back[:, off + n:] == pad).all())


def _quant(rng, shape):
    return (rng.choice(np.arange(-5, 6), size=shape, p=QUANT_P) * np.float32(0.25)).astype(
        np.float32)


def _encode_data(n, C, seed):
    """3 nodes (x, x0, acc, counter).  0: 11 levels in x alone (x0 = acc = 0), +-1.25 on the two
    sides of the first chunk edge; 1: random, nothing ties; 2: 11 levels in each of x, x0 and
    acc."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((3, n)).astype(np.float32)
    x0 = (x + 0.1 * rng.standard_normal((3, n))).astype(np.float32)
    acc = (0.05 * rng.standard_normal((3, n))).astype(np.float32)
    x[0], x0[0], acc[0] = _quant(rng, n), 0.0, 0.0
    if n > C:
        x[0, C - 1], x[0, C] = 1.25, -1.25
    x[2], x0[2], acc[2] = _quant(rng, n), _quant(rng, n), _quant(rng, n)
    counter = rng.integers(0, 5, size=(3, n)).astype(np.int32)
    return x, x0, acc, counter


def _run_encode(dev, codec, x, x0, acc, counter, k, avg, aligned, with_counter=True):
    """The kernel on device copies of the inputs; returns what it left behind and checks that x,
    x0 and every word around the rows are untouched."""
    m, n = x.shape
    tx, bx = _rows(dev, x, aligned)
    t0, b0 = _rows(dev, x0, aligned)
    ta, ba = _rows(dev, acc, aligned)
    tk, bk = _rows(dev, np.full((m, n), PAD, np.float32), aligned)
    tc, bc = _rows(dev, counter, aligned, torch.int32, 77)
    cap = up4(k)
    rows = torch.from_numpy(np.full((m, HEADER + 2 * cap + 5), FILL, dtype=np.uint32)
                            .view(np.int32)).to(dev)
    tab = codec.topkacc_node_table(tx, t0, ta, rows, key=tk if avg else None,
                                   counter=tc if with_counter else None)
    mode = codec.DPZ_ACC_ADD if avg else codec.DPZ_ACC_ACCUMULATE
    codec.topkacc_encode_nodes(tab, n, k, mode)
    np.testing.assert_array_equal(ops.u32(tx.cpu().numpy()), ops.u32(x))
    np.testing.assert_array_equal(ops.u32(t0.cpu().numpy()), ops.u32(x0))
    for back, pad in ((bx, PAD), (b0, PAD), (ba, PAD), (bk, PAD), (bc, 77)):
        assert _padding_intact(back, n, aligned, pad)
    if not avg:  # the key row is acc itself: the scratch row is never touched
        assert (bk == PAD).all()
    return rows.cpu().numpy(), ta.cpu().numpy(), tc.cpu().numpy()


def _check_rows(got, pays, k, err):
    cap = up4(k)
    for j, (idx, vals) in enumerate(pays):
        e = f"{err} node {j}"
        assert got[j, :4].tolist() == [k, 0, 0, 0], e
        np.testing.assert_array_equal(got[j, HEADER:HEADER + k], idx, err_msg=e)
        np.testing.assert_array_equal(got[j, HEADER + cap:HEADER + cap + k], vals.view(np.int32),
                                      err_msg=e)
        # the rest of both slots and the words past the row: untouched
        assert (got[j, HEADER + k:HEADER + cap].view(np.uint32) == FILL).all(), e
        assert (got[j, HEADER + cap + k:].view(np.uint32) == FILL).all(), e


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset4"])
@pytest.mark.parametrize("avg", [False, True], ids=["acc", "avg"])
@pytest.mark.parametrize("which", SIZES)
def test_encode_nodes_equals_restatement_and_topk_encode(dev, which, avg, aligned):
    from decentralizepy_amd import codec
    C = codec.topkacc_chunk_elems()
    n = eval(which, {"C": C})
    ws = codec.Workspace(dev)
    mode = codec.DPZ_ACC_ADD if avg else codec.DPZ_ACC_ACCUMULATE
    for k in sorted({1, max(1, round(0.1 * n)), n}):
        err = str((n, k, avg, aligned))
        x, x0, acc, counter = _encode_data(n, C, seed=n + k)
        want_acc, want_cnt = acc.copy(), counter.copy()
        pays = [ops.encode(x[j], x0[j], want_acc[j], want_cnt[j], k, avg) for j in range(3)]
        if n > C and 1 < k < n:
            # the quantised node's input is what the tie allotment needs: the k-th key ties, the
            # run lies in at least two chunks, some of it is taken and some left
            ks = ops.keys(x[0])
            T = np.sort(ks)[n - k]
            run, taken = np.flatnonzero(ks == T), k - int((ks > T).sum())
            assert len(run) > 1 and len(np.unique(run // C)) >= 2, err
            assert 0 < taken < len(run), err
            if which == "3*C+37":  # the taken ties themselves span a chunk edge
                assert run[taken - 1] >= C and run[0] < C, err
        got, got_acc, got_cnt = _run_encode(dev, codec, x, x0, acc, counter, k, avg, aligned)
        _check_rows(got, pays, k, err)
        np.testing.assert_array_equal(ops.u32(got_acc), ops.u32(want_acc), err_msg=err)
        np.testing.assert_array_equal(got_cnt, want_cnt, err_msg=err)
        assert (want_cnt.sum(axis=1) == counter.sum(axis=1) + k).all()
        # the single-node encode on its exact path with the accumulator and the counter
        for j in range(3):
            sx, s0, sa = (torch.from_numpy(a[j].copy()).to(dev) for a in (x, x0, acc))
            sc = torch.from_numpy(counter[j].copy()).to(dev)
            si, sv = codec.topk_encode(sx, k, x0=s0, acc=sa, acc_mode=mode, counter=sc,
                                       workspace=ws, exact=True)
            e = f"{err} topk_encode node {j}"
            np.testing.assert_array_equal(si.cpu().numpy(), pays[j][0], err_msg=e)
            np.testing.assert_array_equal(ops.u32(sv.cpu().numpy()), ops.u32(pays[j][1]),
                                          err_msg=e)
            np.testing.assert_array_equal(ops.u32(sa.cpu().numpy()), ops.u32(want_acc[j]),
                                          err_msg=e)
            np.testing.assert_array_equal(sc.cpu().numpy(), want_cnt[j], err_msg=e)


@pytest.mark.parametrize("avg", [False, True], ids=["acc", "avg"])
@pytest.mark.parametrize("which", ["5", "C+1", "3*C+37"])
def test_encode_nodes_equal_keys_go_to_the_lowest_indices(dev, which, avg):
    """Node 0: every key equal and nonzero; node 1: x == x0 and acc == 0, every key zero; node 2:
    the same with a table that keeps no counter."""
    from decentralizepy_amd import codec
    C = codec.topkacc_chunk_elems()
    n = eval(which, {"C": C})
    rng = np.random.default_rng(n)
    x = rng.standard_normal((3, n)).astype(np.float32)
    x0 = x.copy()
    x0[0] = x[0] = np.float32(0.5) * rng.integers(-4, 5, size=n).astype(np.float32)
    x[0] += np.float32(0.5)  # exact: every change is 0.5
    acc = np.zeros((3, n), np.float32)
    acc[0] = 0.25
    counter = rng.integers(0, 5, size=(3, n)).astype(np.int32)
    for k in sorted({1, max(1, round(0.1 * n)), n}):
        want_acc, want_cnt = acc.copy(), counter.copy()
        pays = [ops.encode(x[j], x0[j], want_acc[j], want_cnt[j], k, avg) for j in range(3)]
        assert all((idx == np.arange(k)).all() for idx, _ in pays)
        assert not want_acc[1:].any() and (want_acc[0, :k] == 0).all()
        assert (want_acc[0, k:] == (0.25 if avg else 0.75)).all()
        for with_counter in (True, False):
            got, got_acc, got_cnt = _run_encode(dev, codec, x, x0, acc, counter, k, avg, True,
                                                with_counter)
            _check_rows(got, pays, k, str((n, k, avg)))
            np.testing.assert_array_equal(ops.u32(got_acc), ops.u32(want_acc))
            np.testing.assert_array_equal(got_cnt, want_cnt if with_counter else counter)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset4"])
def test_post_nodes_equals_numpy(dev, aligned):
    from decentralizepy_amd import codec
    C = codec.topkacc_chunk_elems()
    for which in SIZES:
        n = eval(which, {"C": C})
        rng = np.random.default_rng(n)
        x0 = rng.standard_normal((3, n)).astype(np.float32)
        x = (x0 + 0.1 * rng.standard_normal((3, n))).astype(np.float32)
        acc = (0.05 * rng.standard_normal((3, n))).astype(np.float32)
        x[2, ::3] = x0[2, ::3]  # zero changes
        acc[2, ::2] = 0.0
        want = acc.copy()
        for j in range(3):
            ops.post(want[j], x[j], x0[j])
        tx, bx = _rows(dev, x, aligned)
        t0, b0 = _rows(dev, x0, aligned)
        ta, ba = _rows(dev, acc, aligned)
        codec.topkacc_post_nodes(codec.topkacc_node_table(tx, t0, ta, None), n)
        np.testing.assert_array_equal(ops.u32(ta.cpu().numpy()), ops.u32(want), err_msg=str(n))
        np.testing.assert_array_equal(ops.u32(tx.cpu().numpy()), ops.u32(x))
        np.testing.assert_array_equal(ops.u32(t0.cpu().numpy()), ops.u32(x0))
        assert all(_padding_intact(b, n, aligned) for b in (bx, b0, ba)), n


# ---- the engine ---------------------------------------------------------------------------------
@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_engine_reproduces_the_reference(dev, meta, arr):
    eng = _engine(meta, arr, hip=True, device=dev)
    assert eng.x.is_cuda and eng.x[1].data_ptr() % 16 == 0 and eng.acc[1].data_ptr() % 16 == 0
    drive(eng, meta, arr)


@pytest.fixture
def rccl_group(dev):
    with rccl_loopback(dev) as group:
        yield group


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_engine_through_rccl_equals_the_reference(dev, rccl_group, meta, arr):
    eng = _engine(meta, arr, hip=True, device=dev, rank=0, world=1, group=rccl_group)
    assert eng.coll and eng.recv is not None
    drive(eng, meta, arr, every_payload=True)


def test_engine_with_more_than_four_neighbours_equals_the_restatement(dev):
    """A 7-node star: the hub's six payloads take the fold's node-after-node path."""
    from decentralizepy_amd.gossip_topkacc import TopKAccRound
    adj = [set(range(1, 7))] + [{0} for _ in range(6)]
    n, alpha = 2051, 0.05
    rng = np.random.default_rng(70)
    x = rng.standard_normal((7, n)).astype(np.float32)
    for avg in (False, True):
        eng = TopKAccRound(adj, torch.from_numpy(x).to(dev), alpha,
                           accumulate_averaging_changes=avg)
        hx, h0 = x.copy(), x.copy()
        hacc, hcnt = np.zeros_like(x), np.zeros(x.shape, np.int32)
        for r in range(3):
            for u in range(7):
                hx[u] = (hx[u] + ops.perturbation(71, r, u, n)).astype(np.float32)
            eng.x.copy_(torch.from_numpy(hx).to(dev))
            pays = ops.round_all(adj, hx, h0, hacc, hcnt, eng.k, avg)
            eng.step()
            for u, (idx, vals) in enumerate(pays):
                gi, gv = eng.payload(u)
                np.testing.assert_array_equal(gi.cpu().numpy(), idx)
                np.testing.assert_array_equal(ops.u32(gv.cpu().numpy()), ops.u32(vals))
            np.testing.assert_array_equal(ops.u32(eng.x.cpu().numpy()), ops.u32(hx))
            np.testing.assert_array_equal(ops.u32(eng.x0.cpu().numpy()), ops.u32(hx))
            np.testing.assert_array_equal(ops.u32(eng.acc.cpu().numpy()), ops.u32(hacc))
            np.testing.assert_array_equal(eng.counter.cpu().numpy(), hcnt)


class _TopoGraph:
    def __init__(self, adj):
        self.adj = adj

    def neighbors(self, uid):
        return self.adj[uid]


@pytest.mark.parametrize("avg", [False, True], ids=["acc", "avg"])
def test_engine_equals_the_plugin_objects_node_by_node(dev, tmp_path, avg):
    """decentralizepy_amd.sharing.PartialModel objects, one per node, driven as DPSGDNode drives
    them on fresh perturbations, against the engine on the same inputs, bit for bit."""
    from decentralizepy_amd.sharing.PartialModel import PartialModel
    meta, arr = run_named("avg_irr6" if avg else "acc_irr6")
    nn, n = meta["nodes"], meta["n"]
    adj = ops.run_adjacency(meta)
    graph = _TopoGraph(adj)
    models = [scenario.make_model(meta["shape"]) for _ in range(nn)]
    for u in range(nn):
        scenario.set_flat(models[u], arr["x0"][u])
    nodes = [PartialModel(u, 0, None, scenario._Mapping(nn), graph, models[u], None,
                          str(tmp_path), alpha=meta["alpha"], accumulation=True,
                          accumulate_averaging_changes=avg) for u in range(nn)]
    eng = _engine(meta, arr, hip=True, device=dev)
    for r in range(3):
        x = eng.x.cpu().numpy()
        msgs = []
        for u in range(nn):
            x[u] = (x[u] + ops.perturbation(910, r, u, n)).astype(np.float32)
            scenario.set_flat(models[u], x[u])
            data = nodes[u].get_data_to_send(degree=len(adj[u]))
            msgs.append(dict(data, indices=np.array(data["indices"], copy=True),
                             params=np.array(data["params"], copy=True), CHANNEL="DPSGD"))
        eng.x.copy_(torch.from_numpy(x).to(dev))
        eng.step()
        for u in range(nn):
            nodes[u]._averaging({v: deque([dict(msgs[v])]) for v in graph.neighbors(u)})
        err = f"round {r}"
        for u in range(nn):
            idx, vals = eng.payload(u)
            np.testing.assert_array_equal(idx.cpu().numpy(), msgs[u]["indices"], err_msg=err)
            np.testing.assert_array_equal(ops.u32(vals.cpu().numpy()), ops.u32(msgs[u]["params"]),
                                          err_msg=err)
        np.testing.assert_array_equal(
            ops.u32(eng.x.cpu().numpy()),
            ops.u32(np.stack([scenario.get_flat(m) for m in models])), err_msg=err)
        np.testing.assert_array_equal(
            ops.u32(eng.acc.cpu().numpy()),
            ops.u32(np.stack([m.accumulated_changes.cpu().numpy() for m in models])),
            err_msg=err)
        np.testing.assert_array_equal(
            eng.counter.cpu().numpy(),
            np.stack([np.asarray(m.shared_parameters_counter.numpy()) for m in models]),
            err_msg=err)


@pytest.mark.parametrize("avg", [False, True], ids=["acc", "avg"])
def test_step_launch_count_is_independent_of_the_node_count(dev, avg):
    from decentralizepy_amd import codec
    seen = []
    for name in ("irr6", "reg16"):  # 6 and 16 nodes
        meta, arr = run_named(("avg_" if avg else "acc_") + name)
        eng = _engine(meta, arr, hip=True, device=dev)
        eng.step()
        eng.step()  # both buffer pairs' tables are built
        with codec.KernelTimer() as t:
            eng.step()
        seen.append({name: cnt for name, (_, cnt) in t.result.items()})
    assert seen[0] == seen[1]
    enc = {"topk_exact_hist": 3, "topk_exact_resolve": 3, "topk_exact_count": 1,
           "topk_exact_scan": 1, "topk_exact_write": 1}
    assert {k: seen[0].get(k) for k in enc} == enc
    assert seen[0].get("fold", 0) >= 1 and seen[0].get("topk_accumulate", 0) == (1 if avg else 0)


@pytest.mark.parametrize("avg", [False, True], ids=["acc", "avg"])
def test_step_never_waits_for_the_device(dev, monkeypatch, avg):
    meta, arr = run_named("avg_irr6" if avg else "acc_irr6")
    eng = _engine(meta, arr, hip=True, device=dev)
    eng.step()
    eng.step()

    def no_wait(*a, **kw):
        raise AssertionError("the step waited for the device")

    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "synchronize", no_wait)
        mp.setattr(torch.cuda.Stream, "synchronize", no_wait)
        mp.setattr(torch.cuda.Event, "synchronize", no_wait)
        legs = []
        eng.step(mark=legs.append)
    assert legs == ["encode", "exchange", "fold"] + (["post"] if avg else [])
    torch.cuda.synchronize(dev)
    assert eng.round == 3 and torch.equal(eng.x, eng.x0)
