"""CPU: the whole-topology top-k round with accumulated changes
(decentralizepy_amd/gossip_topkacc.py).  The numpy restatement (tests/topkacc_round_ops.py) against
the runs recorded from the unmodified reference (tests/golden/make_golden_topkacc_round.py), the
engine's sharding, rows, exchange and call order with that restatement standing in for the HIP
kernels on 1, 2 and 3 ranks (gloo), and the argument validation of the entry points without a
device.  The device path is covered by tests/test_gpu_topkacc_round.py, which shares the helpers
here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests import topkacc_round_ops as ops
from tests.dist_harness import spawn_gloo


def np_encode(x, x0, acc, counter, k, avg):
    # the rows are views of the engine's state: numpy shares their memory, updated in place
    idx, vals = ops.encode(x.numpy(), x0.numpy(), acc.numpy(), counter.numpy(), k, avg)
    return torch.from_numpy(idx), torch.from_numpy(vals)


def np_fold(local, payloads, weights, w_self, out):
    out.copy_(torch.from_numpy(ops.fold(local.numpy(), [(i.numpy(), v.numpy())
                                                        for i, v in payloads], weights, w_self)))


def np_post(acc, x_new, x_old):
    ops.post(acc.numpy(), x_new.numpy(), x_old.numpy())


NP = dict(encode=np_encode, fold=np_fold, post=np_post)
RUNS = ops.load_runs()
RUN_IDS = [m["name"] for m, _ in RUNS]


def run_named(name):
    return RUNS[RUN_IDS.index(name)]


def drive(eng, meta, arr, lo=0, every_payload=False):
    """The recorded rounds through an engine: training into ``eng.x`` in place, a step, the
    comparison of payloads, models and, at the end, the accumulators and counters."""
    m = eng.hi - eng.lo
    x_ptr = eng.x.data_ptr()
    for r in range(meta["rounds"]):
        x = eng.x.cpu().numpy()
        for j in range(m):
            x[j] = ops.train(x[j], meta, r, lo + j)
        eng.x.copy_(torch.from_numpy(x).to(eng.x.device))
        eng.step()
        assert eng.round == r + 1 and eng.x.data_ptr() == x_ptr
        for u in (range(meta["nodes"]) if every_payload else range(lo, lo + m)):
            idx, vals = eng.payload(u)
            ops.check_payload(arr, r, u, idx.cpu().numpy(), vals.cpu().numpy())
        assert torch.equal(eng.x, eng.x0)
        ops.check_state(meta, arr, r, eng.x.cpu().numpy(), eng.acc.cpu().numpy(),
                        eng.counter.cpu().numpy(), lo=lo)


def _engine(meta, arr, lo=0, hi=None, **kw):
    from decentralizepy_amd.gossip_topkacc import TopKAccRound
    ops_kw = {} if kw.pop("hip", False) else NP
    x = torch.from_numpy(arr["x0"][lo:hi])
    if "device" in kw:
        x = x.to(kw["device"])
    return TopKAccRound(ops.run_adjacency(meta), x, meta["alpha"],
                        accumulate_averaging_changes=meta["avg"], **ops_kw, **kw)


def test_fixtures_are_the_four_runs():
    assert sorted(RUN_IDS) == ["acc_irr6", "acc_reg16", "avg_irr6", "avg_reg16"]
    for meta, arr in RUNS:
        big = meta["name"].endswith("reg16")
        assert (meta["nodes"], meta["n"], meta["alpha"], meta["rounds"]) == (
            (16, 2051, 0.05, 3) if big else (6, 4100, 0.1, 4))
        assert meta["avg"] == meta["name"].startswith("avg")
        assert meta["k"] == round(meta["alpha"] * meta["n"]) >= 1
        assert arr["x0"].shape == (meta["nodes"], meta["n"]) and arr["counter"].dtype == np.int32
        for name, a in arr.items():
            if a.dtype == np.float32:
                assert not np.signbit(a[a == 0]).any(), name
    assert run_named("acc_reg16")[0]["n"] % 4 == 3  # rows that are no multiple of 4
    adj = ops.run_adjacency(run_named("acc_irr6")[0])
    assert sorted(len(a) for a in adj) == [1, 1, 2, 3, 3, 4]


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_numpy_ops_reproduce_the_reference(meta, arr):
    adj, k = ops.run_adjacency(meta), meta["k"]
    x = arr["x0"].copy()
    x0, acc = x.copy(), np.zeros_like(x)
    counter = np.zeros(x.shape, np.int32)
    for r in range(meta["rounds"]):
        for u in range(meta["nodes"]):
            x[u] = ops.train(x[u], meta, r, u)
            change = (x[u] - x0[u]).astype(np.float32)
            assert not ops.kth_has_tie(change + acc[u], k)  # the key of either mode
        pays = ops.round_all(adj, x, x0, acc, counter, k, meta["avg"])
        for u, (idx, vals) in enumerate(pays):
            ops.check_payload(arr, r, u, idx, vals)
        ops.check_state(meta, arr, r, x, acc, counter)
    assert counter.sum() == meta["rounds"] * meta["nodes"] * k


def test_the_two_modes_differ_from_each_other_and_from_plain_topk():
    """The accumulator matters from round 1 on: the recorded selections of the two modes and a
    plain top-k of x - x0 on the recorded models all differ."""
    (ma, aa), (mv, av) = run_named("acc_irr6"), run_named("avg_irr6")
    np.testing.assert_array_equal(aa["r0_idx"], av["r0_idx"])  # acc = 0 in round 0
    assert not np.array_equal(aa["r1_idx"], av["r1_idx"])
    x1 = np.stack([ops.train(aa["r0_x"][u], ma, 1, u) for u in range(6)])
    plain = np.stack([ops.select(x1[u] - aa["r0_x"][u], ma["k"]) for u in range(6)])
    assert not np.array_equal(plain, aa["r1_idx"])


def test_select_sends_ties_to_the_lowest_indices():
    c = np.array([1, -2, 2, 0, 2, -1, 2], np.float32)
    assert ops.select(c, 2).tolist() == [1, 2] and ops.select(c, 3).tolist() == [1, 2, 4]
    assert ops.select(c, 5).tolist() == [0, 1, 2, 4, 6] and ops.kth_has_tie(c, 2)
    assert not ops.kth_has_tie(c, 4) and ops.kth_has_tie(c, 5) and not ops.kth_has_tie(c, 6)


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_single_rank_engine_reproduces_the_reference(meta, arr):
    eng = _engine(meta, arr)
    assert eng.k == meta["k"] and not eng.coll and eng.recv is None
    assert eng.x.data_ptr() % 16 == 0 and eng.x.stride(0) % 4 == 0
    assert eng.row_words == 4 + 2 * (-(-meta["k"] // 4) * 4)
    assert torch.equal(eng.x0, eng.x) and not eng.acc.any() and not eng.counter.any()
    assert eng.counter.dtype == torch.int32 and eng.avg == meta["avg"]
    drive(eng, meta, arr)


def test_engine_rejects_what_it_does_not_implement():
    from decentralizepy_amd.gossip_topkacc import TopKAccRound
    adj = ops.adjacency(6, ops.EDGES_IRR6)
    x = torch.zeros(6, 40)
    for bad in (dict(exchange="peer"), dict(exchange="reduce_scatter"), dict(compress=True),
                dict(compression_class="Elias")):
        with pytest.raises(ValueError, match="GossipRound"):
            TopKAccRound(adj, x, 0.1, **NP, **bad)
    with pytest.raises(ValueError, match="FullShareRound"):
        TopKAccRound(adj, x, 1.0, **NP)
    with pytest.raises(ValueError, match="FullShareRound"):
        TopKAccRound(adj, x, 0.5, metadata_cap=0.5, **NP)
    with pytest.raises(ValueError, match="k = round.*SubSamplingRound"):
        TopKAccRound(adj, x, 0.01, **NP)  # round(0.4) = 0
    with pytest.raises(ValueError, match="together"):
        TopKAccRound(adj, x, 0.1, encode=np_encode)
    with pytest.raises(ValueError, match="together"):
        TopKAccRound(adj, x, 0.1, encode=np_encode, fold=np_fold)
    with pytest.raises(ValueError, match="rows"):
        TopKAccRound(adj, x[:5], 0.1, **NP)
    assert TopKAccRound(adj, x, 0.02, **NP).k == 1
    assert TopKAccRound(adj, x, 0.6, metadata_cap=0.7, **NP).k == 24


@pytest.mark.parametrize("avg", [False, True], ids=["acc", "avg"])
def test_step_is_one_call_per_leg_whatever_the_node_count(monkeypatch, avg):
    """The call sequence of a step with stubs for the library calls and the collective: encode,
    one all-gather, the guarded fold, the post-step in mode "avg" only, then the swap; the same
    calls for 6 and for 16 nodes, the tables built once per buffer pair, no read of a device
    value in between."""
    from decentralizepy_amd import _lib, codec
    from decentralizepy_amd.gossip_topkacc import TopKAccRound
    calls, built = [], []

    class Lib:
        @staticmethod
        def dpz_decode_average_batch_guarded(m, local, out, n, counts, idx, val, k, w, w_self,
                                             flags, guard, guard_n, stream):
            calls.append(("fold", m, n, [counts[j] for j in range(m)], flags, guard_n,
                          local[0], out[0]))
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: Lib)
    monkeypatch.setattr(codec, "topkacc_node_table",
                        lambda x, x0, acc, rows, key=None, counter=None: built.append(
                            (x.data_ptr(), x0.data_ptr(), key.data_ptr())) or ("tab", len(built)))
    monkeypatch.setattr(codec, "topkacc_encode_nodes",
                        lambda tab, n, k, mode, ws: calls.append(("encode", tab, n, k, mode)))
    monkeypatch.setattr(codec, "topkacc_post_nodes",
                        lambda tab, n: calls.append(("post", tab, n)))
    monkeypatch.setattr(dist, "all_gather_into_tensor",
                        lambda out, inp, group=None: calls.append(("all_gather", tuple(out.shape),
                                                                   tuple(inp.shape), group)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type(
        "S", (), {"cuda_stream": 0})())
    monkeypatch.setattr(torch.Tensor, "item", lambda self: pytest.fail("a device value was read"))
    names = []
    for name in ("avg_irr6" if avg else "acc_irr6", "avg_reg16" if avg else "acc_reg16"):
        meta, arr = run_named(name)
        nn, n, k = meta["nodes"], meta["n"], meta["k"]
        eng = TopKAccRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]), meta["alpha"],
                           accumulate_averaging_changes=avg, group="g")  # the HIP path
        x, a, b = eng.x.data_ptr(), eng.x0.data_ptr(), eng.out.data_ptr()
        legs = []
        del calls[:], built[:]
        for _ in range(4):
            eng.step(mark=legs.append)
        W = eng.row_words
        mode = codec.DPZ_ACC_ADD if avg else codec.DPZ_ACC_ACCUMULATE
        flags = _lib.DPZ_FOLD_SELF | _lib.DPZ_FOLD_ALSO_LOCAL
        degs = [len(s) for s in ops.run_adjacency(meta)]

        def want(tab, x0, out):
            return ([("encode", tab, n, k, mode), ("all_gather", (nn, W), (nn, W), "g"),
                     ("fold", nn, n, degs, flags, nn, x, out)]
                    + ([("post", tab, n)] if avg else []))

        t1, t2 = ("tab", 1), ("tab", 2)
        assert calls == want(t1, a, b) + want(t2, b, a) + want(t1, a, b) + want(t2, b, a)
        assert built == [(x, a, b), (x, b, a)]  # one table per buffer pair, built once
        assert legs == (["encode", "exchange", "fold"] + (["post"] if avg else [])) * 4
        assert eng.round == 4 and eng.x0.data_ptr() == a
        names.append([c[0] for c in calls])
    assert names[0] == names[1]


def test_fold_falls_back_to_the_batch_when_a_node_has_more_than_four_neighbours(monkeypatch):
    from decentralizepy_amd import _lib, codec
    from decentralizepy_amd.gossip_topkacc import TopKAccRound
    calls = []

    class Lib:
        @staticmethod
        def dpz_decode_average_batch_guarded(*a):
            calls.append("guarded")
            return _lib.DPZ_ERR_UNSUPPORTED

        @staticmethod
        def dpz_decode_average_batch(m, local, out, n, counts, idx, val, k, w, w_self, flags, ws,
                                     ws_bytes, n_streams, streams):
            calls.append(("batch", m, n, flags, n_streams))
            return 0

        @staticmethod
        def dpz_decode_workspace_bytes(n, p):
            return 256

    monkeypatch.setattr(_lib, "lib", lambda: Lib)
    monkeypatch.setattr(_lib, "check", lambda rc, what: None if rc == 0 else pytest.fail(what))
    monkeypatch.setattr(codec, "topkacc_node_table", lambda *a, **kw: "tab")
    monkeypatch.setattr(codec, "topkacc_encode_nodes", lambda *a: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type(
        "S", (), {"cuda_stream": 0})())
    star = [set(range(1, 7))] + [{0} for _ in range(6)]
    eng = TopKAccRound(star, torch.zeros(7, 40), 0.1)
    eng.step()
    assert calls == ["guarded", ("batch", 7, 40, _lib.DPZ_FOLD_SELF | _lib.DPZ_FOLD_ALSO_LOCAL,
                                 1)]


# ---- 1, 2 and 3 ranks over gloo -----------------------------------------------------------------
def _worker(rank, world, name):
    from decentralizepy_amd.gossip_round import shard
    meta, arr = run_named(name)
    lo, hi, per = shard(meta["nodes"], world, rank)
    gathers = []
    real = dist.all_gather_into_tensor

    def counted(out, inp, group=None):
        gathers.append(tuple(inp.shape))
        return real(out, inp, group=group)

    dist.all_gather_into_tensor = counted
    try:
        eng = _engine(meta, arr, lo, hi, rank=rank, world=world)
        assert eng.coll and eng.recv.shape[0] == per * world
        drive(eng, meta, arr, lo=lo, every_payload=True)
    finally:
        dist.all_gather_into_tensor = real
    return lo, hi, gathers == [(per, eng.row_words)] * meta["rounds"]


@pytest.mark.parametrize("name,world", [("acc_irr6", 1), ("avg_irr6", 2), ("acc_reg16", 3),
                                        ("avg_reg16", 3), ("acc_irr6", 3), ("avg_reg16", 2)])
def test_gloo_worlds_reproduce_the_reference(name, world):
    from decentralizepy_amd.gossip_round import shard
    nn = run_named(name)[0]["nodes"]
    if (nn, world) == (16, 3):
        assert shard(nn, 3, 2) == (12, 16, 6)  # 6 + 6 + 4: the last rank's block is padded
    if world == 1:  # one rank with a group: the collective path as a loopback
        got = spawn_gloo(_worker_group, 1, name)
    else:
        got = spawn_gloo(_worker, world, name)
    assert len(got) == world and sum(hi - lo for lo, hi, _ in got) == nn
    assert all(one_gather_per_step for _, _, one_gather_per_step in got)


def _worker_group(rank, world, name):
    meta, arr = run_named(name)
    gathers = []
    real = dist.all_gather_into_tensor

    def counted(out, inp, group=None):
        gathers.append(tuple(inp.shape))
        return real(out, inp, group=group)

    dist.all_gather_into_tensor = counted
    try:
        eng = _engine(meta, arr, group=dist.group.WORLD)
        assert eng.coll and eng.recv is not None
        drive(eng, meta, arr, every_payload=True)
    finally:
        dist.all_gather_into_tensor = real
    return 0, meta["nodes"], len(gathers) == meta["rounds"]


# ---- the C entry points: every check is made on the host, before any device call ---------------
def test_table_builder_lays_out_the_documented_words():
    from decentralizepy_amd import codec
    x = torch.zeros(3, 8)
    x0, acc, key = torch.zeros(3, 8), torch.zeros(3, 8), torch.zeros(3, 8)
    counter = torch.zeros(3, 8, dtype=torch.int32)
    rows = torch.zeros(3, 12, dtype=torch.int32)
    tab = codec.topkacc_node_table(x, x0, acc, rows, key=key, counter=counter).numpy()
    assert tab.shape == (3, 6) and tab.dtype == np.int64
    for j in range(3):
        assert tab[j].tolist() == [x[j].data_ptr(), x0[j].data_ptr(), acc[j].data_ptr(),
                                   key[j].data_ptr(), counter[j].data_ptr(), rows[j].data_ptr()]
    bare = codec.topkacc_node_table([x[1]], [x0[1]], [acc[1]], None).numpy()
    assert bare.tolist() == [[x[1].data_ptr(), x0[1].data_ptr(), acc[1].data_ptr(), 0, 0, 0]]
    assert codec.topkacc_row_words(5) == 20 and codec.topkacc_row_words(8) == 20
    assert codec.topkacc_row_words(9) == 28


def test_argument_validation_without_gpu():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    ARG, UNSUP = _lib.DPZ_ERR_ARG, _lib.DPZ_ERR_UNSUPPORTED
    ACC, ADD, NONE = _lib.DPZ_ACC_ACCUMULATE, _lib.DPZ_ACC_ADD, _lib.DPZ_ACC_NONE
    d, n, big = 4096, 100, 1 << 31  # d is never dereferenced: the checks come first
    assert L.dpz_topkacc_chunk_elems() > 0 and L.dpz_topkacc_chunk_elems() % 1024 == 0
    need = L.dpz_topkacc_encode_workspace_bytes(3, n)
    assert need >= 3 * 256 and L.dpz_topkacc_encode_workspace_bytes(0, n) == 0
    assert L.dpz_topkacc_encode_workspace_bytes(3, 0) == 0
    assert L.dpz_topkacc_encode_workspace_bytes(6, n) == 2 * need

    # every call here must stop at a check: nothing may reach a launch on this machine
    def enc(m=3, tab=d, n=n, k=5, mode=ACC, ws=d, wsb=need):
        return L.dpz_topkacc_encode_nodes(m, tab, n, k, mode, ws, wsb, None)

    for bad in (dict(m=0), dict(m=-1), dict(tab=None), dict(ws=None), dict(n=0), dict(n=-5),
                dict(n=big, k=5, wsb=1 << 40), dict(n=big + 7, k=5, wsb=1 << 40), dict(k=0),
                dict(k=-1), dict(k=n + 1), dict(mode=NONE), dict(mode=3), dict(mode=-1),
                dict(wsb=need - 1), dict(wsb=0), dict(tab=d + 4), dict(ws=d + 2)):
        assert enc(**bad) == ARG, bad
        assert enc(**dict(bad, mode=bad.get("mode", ADD))) == ARG, bad
    assert enc(m=65536, wsb=1 << 40) == UNSUP

    def post(m=3, tab=d, n=n):
        return L.dpz_topkacc_post_nodes(m, tab, n, None)

    for bad in (dict(m=0), dict(m=-1), dict(tab=None), dict(n=0), dict(n=big), dict(tab=d + 4)):
        assert post(**bad) == ARG, bad
    assert post(m=65536) == UNSUP
    assert L.dpz_abi_version() == 2  # symbols were added, nothing changed


def test_header_library_and_ctypes_table_agree():
    from decentralizepy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "dpz_codec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dpz_[a-z0-9_]+)\s*\(", text))
    new = {"dpz_topkacc_encode_nodes": 8, "dpz_topkacc_post_nodes": 4,
           "dpz_topkacc_chunk_elems": 0, "dpz_topkacc_encode_workspace_bytes": 2}
    assert set(new) <= declared and set(_lib.SIGNATURES) == declared
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in new.items():
        assert hasattr(handle, name) and len(_lib.SIGNATURES[name][1]) == nargs
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    assert all(name in doc for name in new)
