"""CPU: the batched JWINS round (decentralizepy_amd/gossip_jwins_batch.py) with the numpy oracle
(tests/jwins_ops.OracleJwinsOps) standing in for the HIP kernels: the runs recorded from the
unmodified reference ``JWINS`` class over two topologies
(tests/golden/make_golden_jwins_round.py) on 1, 2 and 3 ranks (gloo), equality with
``JwinsRound`` round by round, the argument errors of the engine and of the new entry points
without a device.  The device path is covered by tests/test_gpu_jwins_batch_round.py."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests import jwins_round_ops as ops
from tests.dist_harness import spawn_gloo
from tests.jwins_ops import OracleJwinsOps, coeff_len

RUNS = ops.load_runs()
RUN_IDS = [m["name"] for m, _ in RUNS]
CPU = torch.device("cpu")


def run_named(name):
    return RUNS[RUN_IDS.index(name)]


def _engine(meta, arr, lo=0, hi=None, **kw):
    from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound
    return JwinsBatchRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"][lo:hi]),
                           meta["alpha_list"], wavelet=meta["wavelet"], level=meta["level"],
                           metadata_cap=meta["metadata_cap"], device=CPU,
                           ops=OracleJwinsOps(meta["wavelet"], meta["level"]), **kw)


def test_fixtures_are_the_two_runs():
    assert sorted(RUN_IDS) == ["irr6", "reg16"]
    for meta, arr in RUNS:
        big = meta["name"] == "reg16"
        assert (meta["nodes"], meta["n"], meta["rounds"]) == ((16, 1030, 3) if big
                                                              else (6, 4100, 4))
        assert meta["alpha_list"] == ops.TUTORIAL_ALPHAS and meta["metadata_cap"] == 0.5
        assert (meta["wavelet"], meta["level"]) == ("sym2", 4)
        assert meta["m_len"] == coeff_len(meta["n"]) == (1040 if big else 4111)
        assert arr["x0"].shape == (meta["nodes"], meta["n"]) and arr["counter"].dtype == np.int32
        rngs = [random.Random(u) for u in range(meta["nodes"])]
        partial = set()
        for r in range(meta["rounds"]):
            draws = [g.choice(meta["alpha_list"]) for g in rngs]
            assert draws == arr[f"r{r}_alpha"].tolist()
            full = [u for u, a in enumerate(draws) if a >= 0.5]
            assert full == meta["full_shares"][r] and full  # a full share in every round
            for u, a in enumerate(draws):
                assert (f"r{r}_n{u}_idx" in arr) == (a < 0.5)
                if a < 0.5:
                    partial.add(a)
                    assert arr[f"r{r}_n{u}_idx"].size == round(a * meta["m_len"])
                    assert np.all(np.diff(arr[f"r{r}_n{u}_idx"]) > 0)
        assert len(partial) >= 4
        for name, a in arr.items():
            if a.dtype == np.float32:
                assert not np.signbit(a[a == 0]).any(), name
    assert run_named("irr6")[0]["full_shares"] == [[0, 2], [2], [0, 1], [1]]
    adj = ops.run_adjacency(run_named("irr6")[0])
    assert sorted(len(a) for a in adj) == [1, 1, 2, 3, 3, 4]


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_single_rank_engine_reproduces_the_reference(meta, arr):
    eng = _engine(meta, arr)
    assert eng.M == meta["m_len"] and not eng.coll and eng.recv is None
    for rows in (eng.x, eng.x0, eng.acc, eng.wx, eng.wc, eng.counter):
        # a row every 256 bytes from the buffer's start (which the host allocator aligns to 64)
        assert rows.data_ptr() % 64 == 0 and rows.stride(0) % 64 == 0
    assert torch.equal(eng.x0, eng.x) and not eng.acc.any() and not eng.counter.any()
    assert eng.counter.dtype == torch.int32
    legs = []
    eng.step(mark=legs.append)
    assert legs == ["encode", "exchange", "fold", "post"]
    ops.drive(_engine(meta, arr), meta, arr)


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_engine_equals_jwins_round_round_by_round(meta, arr):
    from decentralizepy_amd.gossip_jwins import JwinsRound
    adj = ops.run_adjacency(meta)
    x = torch.from_numpy(arr["x0"])
    new = _engine(meta, arr)
    old = JwinsRound(adj, x, meta["alpha_list"], ops=OracleJwinsOps(), device=CPU,
                     metadata_cap=meta["metadata_cap"], m_len=meta["m_len"])
    for r in range(meta["rounds"] + 2):  # two rounds past the recording
        for u in range(meta["nodes"]):
            step = torch.from_numpy(ops.perturbation(meta["seed"] + 1, r, u, meta["n"]))
            new.x[u] += step
            old.x[u] += step
        new.step()
        old.step()
        assert new.alphas == old.alphas
        lay, s_idx, s_val = old._layout(old.alphas)
        for u in range(meta["nodes"]):
            (ni, nv), (oi, ov) = new.payload(u), old._payload(u, lay, s_idx, s_val)
            assert (ni is None) == (oi is None) and (ni is None or torch.equal(ni, oi))
            assert torch.equal(nv.view(torch.int32), ov.view(torch.int32))
        for a, b in ((new.x, old.x), (new.x0, old.x0), (new.acc, old.acc)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(new.counter, old.counter)


def test_engine_rejects_what_it_does_not_implement():
    from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound, sym2_coeff_len
    adj = ops.adjacency(6, ops.EDGES_IRR6)
    x = torch.zeros(6, 40)
    kw = dict(device=CPU, ops=OracleJwinsOps())
    for bad in (dict(exchange="peer"), dict(compress=True), dict(compression_class="Elias"),
                dict(m_len=50), dict(streams=3)):
        with pytest.raises(ValueError, match="unknown arguments"):
            JwinsBatchRound(adj, x, [0.1, 1.0], **kw, **bad)
    for bad in (dict(wavelet="haar"), dict(wavelet="db4"), dict(level=5), dict(level=0),
                dict(level=8)):
        with pytest.raises(ValueError, match="JwinsRound"):
            JwinsBatchRound(adj, x, [0.1, 1.0], **kw, **bad)
    with pytest.raises(ValueError, match="k = round"):
        JwinsBatchRound(adj, x, [0.01, 1.0], **kw)  # round(0.01 * 50) = 0
    with pytest.raises(ValueError, match="too short"):
        JwinsBatchRound(adj, x[:, :10], [0.5, 1.0], **kw)  # level 4 needs 11 values
    with pytest.raises(ValueError, match="rows"):
        JwinsBatchRound(adj, x[:5], [0.1, 1.0], **kw)
    with pytest.raises(ValueError, match="rank"):
        JwinsBatchRound(adj, x, [0.1, 1.0], rank=2, world=2, **kw)
    # an alpha at or above the cap is a full share whatever round(alpha M) is
    assert JwinsBatchRound(adj, x, [0.01], metadata_cap=0.01, **kw).M == 50
    assert JwinsBatchRound(adj, x, "[0.02, 1.0]", **kw).alpha_list == [0.02, 1.0]  # k = 1
    for n in (11, 12, 100, 101, 1030, 4100, 89834):
        for level in (1, 2, 3, 4):
            assert sym2_coeff_len(n, level) == coeff_len(n, level)
    assert sym2_coeff_len(10, 4) is None and sym2_coeff_len(11, 4) == 22


# ---- 2 and 3 ranks over gloo ---------------------------------------------------------------------
def _worker(rank, world, name, group_only=False):
    from decentralizepy_amd.gossip_round import shard
    meta, arr = run_named(name)
    lo, hi, per = (0, meta["nodes"], meta["nodes"]) if group_only else shard(meta["nodes"], world,
                                                                             rank)
    gathers = []
    real = dist.all_gather_into_tensor

    def counted(out, inp, group=None):
        gathers.append((out.numel(), inp.numel()))
        return real(out, inp, group=group)

    dist.all_gather_into_tensor = counted
    try:
        kw = dict(group=dist.group.WORLD) if group_only else dict(rank=rank, world=world)
        eng = _engine(meta, arr, lo, hi, **kw)
        assert eng.coll and eng.recv.numel() == world * eng.send.numel()
        ops.drive(eng, meta, arr, lo=lo, every_payload=True)
    finally:
        dist.all_gather_into_tensor = real
    one_buffer_per_round = (len(gathers) == meta["rounds"]
                            and all(o == world * i and i % 64 == 0 for o, i in gathers))
    return lo, hi, one_buffer_per_round


@pytest.mark.parametrize("name,world", [("irr6", 2), ("reg16", 3), ("irr6", 3), ("reg16", 2)])
def test_gloo_worlds_reproduce_the_reference(name, world):
    from decentralizepy_amd.gossip_round import shard
    nn = run_named(name)[0]["nodes"]
    if (nn, world) == (16, 3):
        assert shard(nn, 3, 2) == (12, 16, 6)  # 6 + 6 + 4: the last rank's block is padded
    got = spawn_gloo(_worker, world, name)
    assert len(got) == world and sum(hi - lo for lo, hi, _ in got) == nn
    assert all(ok for _, _, ok in got)


def test_one_rank_with_a_group_gathers_as_a_loopback():
    got = spawn_gloo(_worker, 1, "irr6", True)
    assert got == [(0, 6, True)]


# ---- the round's calls with stubs for the library -------------------------------------------------
def test_step_is_one_call_per_leg_whatever_the_node_count(monkeypatch):
    """The call sequence of a step with stubs for the codec wrappers, the fold and the
    collective: the table's upload first, one pair transform, one encode, one all-gather, the
    guarded fold (here refused: the batch fold on the same stream), one inverse, one
    accumulating transform; the same calls for 6 and for 16 nodes, no device value read."""
    from decentralizepy_amd import _lib, codec
    from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound
    calls = []

    class Tab:
        def __init__(self, kind, *cols):
            self.kind, self.m = kind, len(cols[0])
            self.sets = {}

        def set(self, j, k, idx_out, val_out):
            self.sets[j] = (k, idx_out, val_out)

        def upload(self):
            calls.append(("upload", dict(self.sets)))

    class Lib:
        @staticmethod
        def dpz_jwins_encode_workspace_bytes(m, n):
            return 256

        @staticmethod
        def dpz_decode_workspace_bytes(n, p):
            return 256

        @staticmethod
        def dpz_decode_average_batch_guarded(m, local, out, n, counts, idx, val, k, w, w_self,
                                             flags, guard, guard_n, stream):
            dense = any(idx[i] is None for i in range(sum(counts[j] for j in range(m))))
            calls.append(("guarded", m, n, flags, guard_n))
            return _lib.DPZ_ERR_UNSUPPORTED if dense or max(counts[j] for j in range(m)) > 4 \
                else 0

        @staticmethod
        def dpz_decode_average_batch(m, local, out, n, counts, idx, val, k, w, w_self, flags, ws,
                                     ws_bytes, n_streams, streams):
            calls.append(("batch", m, n, flags, n_streams,
                          [k[i] for i in range(sum(counts[j] for j in range(m)))]))
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: Lib)
    monkeypatch.setattr(_lib, "check", lambda rc, what: None if rc == 0 else pytest.fail(what))
    monkeypatch.setattr(codec, "DwtNodesTable", lambda *c: Tab("dwt", c[0]))
    monkeypatch.setattr(codec, "IdwtNodesTable", lambda *c: Tab("idwt", c[0]))
    monkeypatch.setattr(codec, "JwinsEncodeTable", lambda *c: Tab("enc", c[0]))
    monkeypatch.setattr(codec, "dwt_sym2_nodes", lambda tab, n, level, accumulate=False:
                        calls.append(("dwt", tab.kind, n, level, accumulate)))
    monkeypatch.setattr(codec, "idwt_sym2_nodes", lambda tab, n, level:
                        calls.append(("idwt", tab.kind, n, level)))
    monkeypatch.setattr(codec, "jwins_encode_nodes", lambda tab, n, ws:
                        calls.append(("encode", tab.kind, n)))
    monkeypatch.setattr(dist, "all_gather_into_tensor", lambda out, inp, group=None:
                        calls.append(("all_gather", out.numel(), inp.numel(), group)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type(
        "S", (), {"cuda_stream": 0})())
    monkeypatch.setattr(torch.Tensor, "item", lambda self: pytest.fail("a device value was read"))
    names = []
    for name in RUN_IDS:
        meta, arr = run_named(name)
        nn, n, M = meta["nodes"], meta["n"], meta["m_len"]
        eng = JwinsBatchRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]),
                              meta["alpha_list"], group="g", device=CPU)  # the HIP path
        del calls[:]
        for r in range(meta["rounds"]):
            eng.step()
        per_round = len(calls) // meta["rounds"]
        assert per_round * meta["rounds"] == len(calls)
        for r in range(meta["rounds"]):
            c = calls[r * per_round:(r + 1) * per_round]
            assert [x[0] for x in c] == ["upload", "dwt", "encode", "all_gather", "guarded",
                                         "batch", "idwt", "dwt"]
            sets = c[0][1]
            assert sorted(sets) == list(range(nn))
            for u in range(nn):
                a = arr[f"r{r}_alpha"][u]
                k, idx_out, val_out = sets[u]
                base = eng.send.data_ptr()  # slots start on 256-byte steps of the buffer
                assert k == (round(a * M) if a < 0.5 else 0) and (val_out - base) % 256 == 0
                assert (idx_out == 0) == (a >= 0.5)
                assert idx_out == 0 or (idx_out - base) % 256 == 0
            assert c[1] == ("dwt", "dwt", n, 4, False) and c[2] == ("encode", "enc", M)
            assert c[3][1] == c[3][2] and c[3][3] == "g"  # one rank: the gather is a loopback
            assert c[4] == ("guarded", nn, M, _lib.DPZ_FOLD_SELF, 1)
            assert c[5][:5] == ("batch", nn, M, _lib.DPZ_FOLD_SELF, 1)
            want_k = [M if arr[f"r{r}_alpha"][q] >= 0.5 else round(arr[f"r{r}_alpha"][q] * M)
                      for u in range(nn) for q in ops.run_adjacency(meta)[u]]
            assert c[5][5] == want_k
            assert c[6] == ("idwt", "idwt", n, 4) and c[7] == ("dwt", "dwt", n, 4, True)
        names.append([x[0] for x in calls[:per_round]])
    assert names[0] == names[1]


# ---- the C entry points: every check is made on the host, before any device call ----------------
def test_argument_validation_without_gpu():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    ARG, UNSUP = _lib.DPZ_ERR_ARG, _lib.DPZ_ERR_UNSUPPORTED
    d, n, big = 4096, 100, 1 << 31  # d is never dereferenced: the checks come first
    assert L.dpz_jwins_chunk_elems() > 0 and L.dpz_jwins_chunk_elems() % 1024 == 0
    need = L.dpz_jwins_encode_workspace_bytes(3, n)
    assert need >= 3 * 256 and L.dpz_jwins_encode_workspace_bytes(0, n) == 0
    assert L.dpz_jwins_encode_workspace_bytes(3, 0) == 0
    assert L.dpz_jwins_encode_workspace_bytes(6, n) == 2 * need

    # every call here must stop at a check: nothing may reach a launch on this machine
    def enc(m=3, tab=d, n=n, ws=d, wsb=need):
        return L.dpz_jwins_encode_nodes(m, tab, n, ws, wsb, None)

    for bad in (dict(m=0), dict(m=-1), dict(tab=None), dict(ws=None), dict(n=0), dict(n=-5),
                dict(n=big, wsb=1 << 40), dict(n=big + 7, wsb=1 << 40), dict(wsb=need - 1),
                dict(wsb=0), dict(tab=d + 4), dict(ws=d + 2)):
        assert enc(**bad) == ARG, bad
    assert enc(m=65536, wsb=1 << 40) == UNSUP

    def table(rows, words):
        host = np.array(rows, dtype=np.uint64).reshape(-1, words)
        return host, ctypes.c_void_p(host.ctypes.data)

    def dwt(rows, m=None, tab=d, n=n, level=4, accumulate=0, host=True):
        h, p = table(rows, 4)
        return L.dpz_dwt_sym2_nodes(len(h) if m is None else m, tab, p if host else None, n,
                                    level, accumulate, None)

    ok = [256, 512, 1024, 2048]
    both = [ok, [4096, 8192, 16384, 32768]]
    assert dwt(both, m=0) == ARG and dwt(both, m=-1) == ARG
    assert dwt(both, tab=None) == ARG and dwt(both, host=False) == ARG
    assert dwt(both, tab=d + 4) == ARG and dwt(both, n=0) == ARG and dwt(both, n=-3) == ARG
    assert dwt([ok, [0, 8192, 16384, 32768]]) == ARG          # no x
    assert dwt([ok, [4096, 0, 16384, 32768]]) == ARG          # coeffs_diff without x0
    for col in range(4):                                      # a row that is not 16-byte aligned
        for off in (4, 8, 12):
            row = list(both[1])
            row[col] += off
            assert dwt([ok, row]) == ARG, (col, off)
    assert dwt([ok, [4096, 8192, 0, 32768]]) == ARG           # mixed output sets
    assert dwt([ok, [4096, 8192, 16384, 0]]) == ARG
    assert dwt([[256, 0, 1024, 0], [4096, 0, 16384, 0]], accumulate=1) == ARG
    for level in (0, 5, 8, -1):
        assert dwt(both, level=level) == UNSUP, level
    assert dwt(both, n=10) == UNSUP and dwt(both, n=3, level=1) == UNSUP
    assert dwt([ok] * 65536) == UNSUP
    assert dwt([[256, 512, 0, 0]] * 2) == 0                   # no output: nothing to do

    def idwt(rows, m=None, tab=d, n=n, level=4, host=True):
        h, p = table(rows, 2)
        return L.dpz_idwt_sym2_nodes(len(h) if m is None else m, tab, p if host else None, n,
                                     level, None)

    two = [[256, 512], [1024, 2048]]
    assert idwt(two, m=0) == ARG and idwt(two, tab=None) == ARG and idwt(two, host=False) == ARG
    assert idwt(two, tab=d + 4) == ARG and idwt(two, n=0) == ARG
    assert idwt([[256, 512], [0, 2048]]) == ARG and idwt([[256, 512], [1024, 0]]) == ARG
    assert idwt([[256, 512], [1028, 2048]]) == ARG and idwt([[256, 512], [1024, 2056]]) == ARG
    for level in (0, 5, 8):
        assert idwt(two, level=level) == UNSUP, level
    assert idwt(two, n=10) == UNSUP and idwt([[256, 512]] * 65536) == UNSUP
    assert L.dpz_abi_version() == 2  # symbols were added, nothing changed


def test_header_library_and_ctypes_table_agree():
    from decentralizepy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "dpz_codec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dpz_[a-z0-9_]+)\s*\(", text))
    new = {"dpz_dwt_sym2_nodes": 7, "dpz_idwt_sym2_nodes": 6, "dpz_jwins_chunk_elems": 0,
           "dpz_jwins_encode_workspace_bytes": 2, "dpz_jwins_encode_nodes": 6}
    assert set(new) <= declared and set(_lib.SIGNATURES) == declared
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in new.items():
        assert hasattr(handle, name) and len(_lib.SIGNATURES[name][1]) == nargs
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    assert all(name in doc for name in new)


def test_encode_table_lays_out_the_documented_words():
    from decentralizepy_amd import codec
    c, acc, wx = torch.zeros(3, 8), torch.zeros(3, 8), torch.zeros(3, 8)
    counter = torch.zeros(3, 8, dtype=torch.int32)
    tab = codec.JwinsEncodeTable(c, acc, wx, counter, CPU)
    send = torch.zeros(64, dtype=torch.int32)
    tab.set(0, 3, send[0:3], send[32:35])
    tab.set(1, 0, None, None)
    tab.set(2, 0, 0, send.data_ptr() + 4 * 40)
    tab.upload()
    p = send.data_ptr()
    want = [[c[j].data_ptr(), acc[j].data_ptr(), wx[j].data_ptr(), counter[j].data_ptr()]
            for j in range(3)]
    want[0] += [p, p + 128, 3, 0]
    want[1] += [0, 0, 0, 0]
    want[2] += [0, p + 160, 0, 0]
    assert tab.dev.tolist() == want and tab.dev.dtype == torch.int64 and tab.m == 3
    bare = codec.JwinsEncodeTable([c[1]], [acc[1]], [wx[1]], None, CPU)
    assert bare.host.tolist() == [[c[1].data_ptr(), acc[1].data_ptr(), wx[1].data_ptr(), 0, 0,
                                   0, 0, 0]]
    dt = codec.DwtNodesTable(c, acc, None, wx, CPU)
    assert dt.host.tolist() == [v for j in range(3)
                                for v in (c[j].data_ptr(), acc[j].data_ptr(), 0,
                                          wx[j].data_ptr())]
    it = codec.IdwtNodesTable(c, wx, CPU)
    assert it.dev.tolist() == [v for j in range(3) for v in (c[j].data_ptr(), wx[j].data_ptr())]
