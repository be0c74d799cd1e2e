"""CPU: the whole-topology Choco round (decentralizepy_amd/gossip_choco.py).  The numpy
restatement (tests/choco_round_ops.py) against the runs recorded from the unmodified reference
(tests/golden/make_golden_choco_round.py), the engine's sharding, slots, exchange and fold order
with that restatement standing in for the HIP kernels on 1, 2 and 3 ranks (gloo), and the argument
validation of the two entry points without a device.  The device path is covered by
tests/test_gpu_choco_round.py, which shares the helpers here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests import choco_round_ops as ops
from tests.dist_harness import spawn_gloo


def np_encode(x, x_hat, k):
    idx, vals = ops.select(x.numpy(), x_hat.numpy(), k)
    return torch.from_numpy(idx), torch.from_numpy(vals)


def np_fold(x, x_hat, s, q_self, w_self, pays, step_size):
    # the rows are views of the engine's state: numpy shares their memory, updated in place
    ops.fold(x.numpy(), x_hat.numpy(), s.numpy(), (q_self[0].numpy(), q_self[1].numpy()), w_self,
             [(i.numpy(), v.numpy(), w) for i, v, w in pays], step_size)


RUNS = ops.load_runs()
RUN_IDS = [m["name"] for m, _ in RUNS]


def drive(eng, meta, arr, lo=0, every_payload=False):
    """The recorded rounds through an engine: training into ``eng.x``, a step, the comparison."""
    m = eng.hi - eng.lo
    for r in range(meta["rounds"]):
        x = eng.x.cpu().numpy()
        new = np.stack([ops.train(x[j], meta, r, lo + j) for j in range(m)]) if m else x
        eng.x.copy_(torch.from_numpy(new).to(eng.x.device))
        eng.step()
        eng.check()
        assert eng.round == r + 1
        nodes = range(meta["nodes"]) if every_payload else range(lo, lo + m)
        for q in nodes:
            idx, vals = eng.payload(q)
            assert idx.numel() == vals.numel() == int(arr["counts"][r][q]), (r, q)
            assert bool((idx[1:] > idx[:-1]).all())
        ops.check_recorded(meta, arr, r, eng.x.cpu().numpy(), None, eng.x_hat.cpu().numpy(),
                           eng.s.cpu().numpy(), lo=lo)


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_numpy_ops_reproduce_the_reference(meta, arr):
    adj = ops.run_adjacency(meta)
    nn, n, k = meta["nodes"], meta["n"], meta["k"]
    assert k == round(meta["alpha"] * n) >= 1 and arr["x0"].shape == (nn, n)
    x = arr["x0"].copy()
    x_hat, s = np.zeros_like(x), np.zeros_like(x)
    for r in range(meta["rounds"]):
        for u in range(nn):
            x[u] = ops.train(x[u], meta, r, u)
        q = [ops.select(x[u], x_hat[u], k) for u in range(nn)]
        for u in range(nn):
            nbrs, w, w_self = ops.mh(adj, u)
            ops.fold(x[u], x_hat[u], s[u], q[u], w_self,
                     [q[v] + (wv,) for v, wv in zip(nbrs, w)], meta["step_size"])
        ops.check_recorded(meta, arr, r, x, [len(i) for i, _ in q], x_hat, s)
    assert not np.signbit(x_hat[x_hat == 0]).any() and not np.signbit(s[s == 0]).any()


def test_tie_fixture_has_ties_and_zeros():
    meta, arr = RUNS[RUN_IDS.index("irr6")]
    assert meta["quantised"] and arr["counts"][0].max() > meta["k"]
    assert meta["slot_cap"] == -(-int(arr["counts"].max()) // 4) * 4
    x = ops.train(arr["x0"][0], meta, 0, 0)
    assert (x[::5] == 0).all() and len(np.unique(np.abs(x))) < 200
    assert sorted(len(a) for a in ops.run_adjacency(meta)) == [1, 1, 2, 3, 3, 4]
    assert meta["n"] % 4 == 0 and RUNS[RUN_IDS.index("regular16")][0]["n"] % 4 == 3


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_single_rank_engine_reproduces_the_reference(meta, arr):
    from decentralizepy_amd.gossip_choco import ChocoRound, slot_capacity
    eng = ChocoRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]), meta["alpha"],
                     meta["step_size"], slot_cap=meta["slot_cap"], encode=np_encode, fold=np_fold)
    assert eng.k == meta["k"] and not eng.coll and eng.recv is None
    assert eng.cap == (meta["slot_cap"] or slot_capacity(meta["n"], meta["k"]))
    assert eng.x.data_ptr() % 16 == 0 and eng.x.stride(0) % 4 == 0
    drive(eng, meta, arr)


def test_slot_capacity_and_k():
    from decentralizepy_amd.gossip_choco import ChocoRound, slot_capacity
    assert slot_capacity(2051, 103) == 168 and slot_capacity(11_000_000, 110_000) == 123_752
    assert slot_capacity(100, 90) == 100 and slot_capacity(5, 1) == 8
    adj = ops.adjacency(6, ops.EDGES_IRR6)
    x = torch.zeros(6, 40)
    kw = dict(encode=np_encode, fold=np_fold)
    with pytest.raises(ValueError, match="k = 0"):
        ChocoRound(adj, x, 0.01, 0.5, **kw)  # round(0.4) = 0
    assert ChocoRound(adj, x, 0.02, 0.5, **kw).k == 1
    assert ChocoRound(adj, x, 0.1, 0.5, slot_cap=9, **kw).cap == 12


def test_engine_rejects_what_it_does_not_implement():
    from decentralizepy_amd.gossip_choco import ChocoRound
    adj = ops.adjacency(6, ops.EDGES_IRR6)
    x = torch.zeros(6, 40)
    for bad in (dict(exchange="peer"), dict(exchange="reduce_scatter"), dict(compress=True),
                dict(compression_class="Elias"), dict(server=True)):
        with pytest.raises(ValueError, match="not implemented"):
            ChocoRound(adj, x, 0.1, 0.5, encode=np_encode, fold=np_fold, **bad)
    with pytest.raises(ValueError, match="together"):
        ChocoRound(adj, x, 0.1, 0.5, encode=np_encode)


def test_small_slot_is_reported_and_changes_no_state():
    from decentralizepy_amd.gossip_choco import ChocoRound
    meta, arr = RUNS[RUN_IDS.index("irr6")]
    x0 = np.stack([ops.train(arr["x0"][u], meta, 0, u) for u in range(6)])
    eng = ChocoRound(ops.run_adjacency(meta), torch.from_numpy(x0), meta["alpha"],
                     meta["step_size"], slot_cap=meta["k"], encode=np_encode, fold=np_fold)
    eng.step()
    over = [u for u in range(6) if arr["counts"][0][u] > eng.cap]
    assert over
    with pytest.raises(RuntimeError, match=re.escape(str(over))):
        eng.check()
    np.testing.assert_array_equal(ops.u32(eng.x.numpy()), ops.u32(x0))
    assert not eng.x_hat.any() and not eng.s.any()


def test_step_is_one_encode_one_collective_one_fold(monkeypatch):
    """The call sequence of a step with stubs for the two library calls and the collective: the
    same three calls for 6 and for 16 nodes, and no read of a device value in between."""
    from decentralizepy_amd import codec
    from decentralizepy_amd.gossip_choco import ChocoRound
    calls = []
    monkeypatch.setattr(codec, "choco_node_table", lambda *a: "enc")
    monkeypatch.setattr(codec, "ChocoTable", lambda recvs, dev: ("fold", len(recvs)))
    monkeypatch.setattr(codec, "choco_encode_nodes",
                        lambda tab, n, k, cap, ws: calls.append(("encode", tab, n, k, cap)))
    monkeypatch.setattr(codec, "choco_fold_nodes",
                        lambda tab, n, step, guard=None: calls.append(("fold", tab[1], n, step)))
    monkeypatch.setattr(dist, "all_gather_into_tensor",
                        lambda out, inp, group=None: calls.append(("all_gather", tuple(out.shape),
                                                                   tuple(inp.shape), group)))
    monkeypatch.setattr(torch.Tensor, "item", lambda self: pytest.fail("a device value was read"))
    for meta, arr in RUNS:
        nn, n = meta["nodes"], meta["n"]
        eng = ChocoRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]), meta["alpha"],
                         meta["step_size"], group="g")  # the HIP path, a group: the collective
        legs = []
        del calls[:]
        eng.step(mark=legs.append)
        eng.step()
        W = 4 + 2 * eng.cap
        want = [("encode", "enc", n, meta["k"], eng.cap),
                ("all_gather", (nn, W), (nn, W), "g"), ("fold", nn, n, meta["step_size"])]
        assert calls == want + want and legs == ["encode", "exchange", "fold"]
        assert eng.round == 2


# ---- 2 and 3 ranks over gloo --------------------------------------------------------------------
def _worker(rank, world, name):
    from decentralizepy_amd.gossip import shard
    from decentralizepy_amd.gossip_choco import ChocoRound
    meta, arr = RUNS[RUN_IDS.index(name)]
    lo, hi, per = shard(meta["nodes"], world, rank)
    eng = ChocoRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"][lo:hi]),
                     meta["alpha"], meta["step_size"], rank=rank, world=world,
                     slot_cap=meta["slot_cap"], encode=np_encode, fold=np_fold)
    assert eng.coll and eng.recv.shape[0] == per * world
    drive(eng, meta, arr, lo=lo, every_payload=True)
    return lo, hi


@pytest.mark.parametrize("name,world", [("irr6", 2), ("regular16", 3), ("irr6", 3)])
def test_gloo_worlds_reproduce_the_reference(name, world):
    from decentralizepy_amd.gossip import shard
    nn = RUNS[RUN_IDS.index(name)][0]["nodes"]
    if (name, world) == ("regular16", 3):
        assert shard(nn, 3, 2) == (12, 16, 6)  # 6 + 6 + 4: the last rank's block is padded
    got = spawn_gloo(_worker, world, name)  # one result per rank; a failed drive() fails here
    assert len(got) == world and sum(hi - lo for lo, hi in got) == nn


# ---- the C entry points: every check is made on the host, before any device call ---------------
def _fold_words(recvs):
    """The fold table's words as codec.ChocoTable lays them out, from plain integers."""
    m = len(recvs)
    n_ent = sum(len(r[6]) for r in recvs)
    words = np.zeros(max(1, 6 * m + 2 * n_ent), dtype=np.uint64)
    halves = words.view(np.uint32)
    pos = 0
    for j, (x, xh, s, row, cap, w_self, pays) in enumerate(recvs):
        b = 6 * j
        words[b:b + 4] = (x, xh, s, row)
        halves[2 * b + 8] = np.float32(w_self).view(np.uint32)
        halves[2 * b + 9] = np.int32(cap).view(np.uint32)
        halves[2 * b + 10], halves[2 * b + 11] = pos, len(pays)
        for prow, pcap, w in pays:
            e = 6 * m + 2 * pos
            words[e] = prow
            halves[2 * e + 2] = np.float32(w).view(np.uint32)
            halves[2 * e + 3] = np.int32(pcap).view(np.uint32)
            pos += 1
    return words, n_ent


def test_table_builder_lays_out_the_documented_words():
    from decentralizepy_amd import codec
    row = 1 << 36
    recvs = [(row, 2 * row, 3 * row, 4 * row, 8, 0.5, [(5 * row, 8, 0.25), (4 * row, 12, 0.125)]),
             (6 * row, 7 * row, 8 * row, 5 * row, 8, 1.0, [])]
    tab = codec.ChocoTable(recvs, "cpu")
    words, n_ent = _fold_words(recvs)
    assert (tab.m, tab.n_entries) == (2, n_ent) and n_ent == 2
    np.testing.assert_array_equal(tab.host, words)
    np.testing.assert_array_equal(tab.dev.numpy().view(np.uint64), words)


def test_argument_validation_without_gpu():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    ARG, WS, UNSUP = _lib.DPZ_ERR_ARG, _lib.DPZ_ERR_WORKSPACE, _lib.DPZ_ERR_UNSUPPORTED
    d, n, big = 4096, 100, 1 << 31  # d is never dereferenced: the checks come first
    assert L.dpz_choco_chunk_elems() > 0 and L.dpz_choco_tile_elems() > 0
    assert L.dpz_choco_chunk_elems() % 1024 == 0 and L.dpz_choco_tile_elems() % 1024 == 0
    need = L.dpz_choco_encode_workspace_bytes(3, n)
    assert need >= 3 * 256 and L.dpz_choco_encode_workspace_bytes(0, n) == 0
    assert L.dpz_choco_encode_workspace_bytes(3, 0) == 0
    assert L.dpz_choco_encode_workspace_bytes(6, n) == 2 * need

    def enc(m=3, tab=d, n=n, k=5, cap=8, ws=d, wsb=need):
        return L.dpz_choco_encode_nodes(m, tab, n, k, cap, ws, wsb, None)

    for bad in (dict(m=0), dict(n=0), dict(k=0), dict(k=-1), dict(k=n + 1), dict(cap=0),
                dict(tab=None), dict(ws=None)):
        assert enc(**bad) == ARG, bad
    assert enc(n=big, k=5, wsb=1 << 40) == UNSUP and enc(m=65536, wsb=1 << 40) == UNSUP
    assert enc(wsb=need - 1) == WS and enc(wsb=0) == WS

    row = 1 << 36  # addresses that are never dereferenced (rows of 2^31 floats stay apart)
    x, xh, s, own, other = (row * i for i in range(1, 6))
    good = [(x, xh, s, own, 8, 0.5, [(other, 8, 0.25), (own, 8, 0.25)]),
            (x + row // 2, xh + row // 2, s + row // 2, other, 8, 1.0, [])]

    def fold(recvs=good, m=None, n=n, dev=row, host=True, n_ent=None, step=0.5, guard=None,
             guard_n=0):
        words, ne = _fold_words(recvs)
        return L.dpz_choco_fold_nodes(
            len(recvs) if m is None else m, dev,
            ctypes.c_void_p(words.ctypes.data) if host else None,
            ne if n_ent is None else n_ent, n, step, guard, guard_n, None)

    # every call here must stop at a check: nothing may reach a launch on this machine
    assert fold(n=big) == UNSUP
    assert fold(m=0) == ARG and fold(n=0) == ARG and fold(dev=None) == ARG
    assert fold(host=False) == ARG and fold(n_ent=-1) == ARG and fold(n_ent=1) == ARG
    assert fold(guard_n=3) == ARG and fold(guard_n=-1) == ARG  # words, no guard
    assert fold(step=float("nan")) == ARG and fold(step=float("inf")) == ARG

    def one(**kw):
        base = dict(x=x, xh=xh, s=s, row=own, cap=8, w_self=0.5, pays=[(other, 8, 0.5)])
        base.update(kw)
        return fold(recvs=[tuple(base[f] for f in ("x", "xh", "s", "row", "cap", "w_self",
                                                   "pays"))])

    for bad in (dict(x=0), dict(xh=0), dict(s=0), dict(row=0), dict(cap=0),
                dict(w_self=float("nan")), dict(pays=[(0, 8, 0.5)]), dict(pays=[(other, 0, 0.5)]),
                dict(pays=[(other, 8, float("inf"))]), dict(x=x + 2), dict(row=own + 1),
                dict(pays=[(other + 2, 8, 0.5)])):
        assert one(**bad) == ARG, bad
    # a written row that equals or overlaps another written row or a payload row, either side
    for bad in (dict(xh=x), dict(s=x + 4 * (n - 1)), dict(s=x - 4 * (n - 1)),
                dict(row=x + 4 * (n - 1)), dict(row=x - 4 * 19), dict(pays=[(s, 8, 0.5)])):
        assert one(**bad) == ARG, bad
    assert fold(recvs=[good[0], (x + 4, xh + row // 2, s + row // 2, other, 8, 1.0, [])]) == ARG
    assert L.dpz_abi_version() == 2  # symbols were added, nothing changed


def test_header_library_and_ctypes_table_agree():
    from decentralizepy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "dpz_codec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dpz_[a-z0-9_]+)\s*\(", text))
    new = {"dpz_choco_encode_nodes": 8, "dpz_choco_fold_nodes": 9, "dpz_choco_chunk_elems": 0,
           "dpz_choco_tile_elems": 0, "dpz_choco_encode_workspace_bytes": 2}
    assert set(new) <= declared and set(_lib.SIGNATURES) == declared
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in new.items():
        assert hasattr(handle, name) and len(_lib.SIGNATURES[name][1]) == nargs
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    assert all(name in doc for name in new)
