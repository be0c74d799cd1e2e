"""CPU: the whole-topology FFT round (decentralizepy_amd/gossip_fft.py) with the numpy oracle
(tests/fft_round_ops.OracleFftOps) standing in for the HIP kernels: the three runs recorded from
the unmodified reference ``FFT`` class (tests/golden/make_golden_fft_round.py) on 1, 2 and 3 ranks
(gloo), the ranks' agreement bit for bit, the constructor's refusals, the call sequence of a step
and the argument errors of the new entry points without a device.  The device path is covered by
tests/test_gpu_fft_round.py.

The bound of round r (0-based) is ``scenario.fft_tol(what, n, max|x0|) * (r + 1)``
(fft_round_ops.tol): the float64 oracle measured here stays below 0.060 of it for the models and
below 0.036 for the frequency-domain arrays (printed by the single-rank test)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests import fft_round_ops as ops
from tests.dist_harness import spawn_gloo

RUNS = ops.load_runs()
RUN_IDS = [m["name"] for m, _ in RUNS]
CPU = torch.device("cpu")


def run_named(name):
    return RUNS[RUN_IDS.index(name)]


def _engine(meta, arr, lo=0, hi=None, **kw):
    from decentralizepy_amd.gossip_fft import FftRound
    return FftRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"][lo:hi]), device=CPU,
                    ops=ops.OracleFftOps(), **ops.engine_kwargs(meta), **kw)


def test_fixtures_are_the_three_runs():
    assert RUN_IDS == ["reg16", "irr6", "plain6"]
    want = {"reg16": (16, 1030, 3, 52, True, False), "irr6": (6, 4100, 3, 205, True, True),
            "plain6": (6, 1024, 2, 51, False, False)}
    for meta, arr in RUNS:
        nn, n, rounds, k, acc, aac = want[meta["name"]]
        assert (meta["nodes"], meta["n"], meta["rounds"], meta["k"]) == (nn, n, rounds, k)
        assert (meta["accumulation"], meta["accumulate_averaging_changes"]) == (acc, aac)
        M = n // 2 + 1
        assert meta["m_len"] == M and k == round(meta["alpha"] * M) and meta["alpha"] == 0.1
        assert meta["min_gap"] >= ops.MIN_GAP == 1e-4
        assert arr["x0"].shape == (nn, n) and arr["x0"].dtype == np.float32
        for r in range(rounds):
            assert arr[f"r{r}_idx"].shape == (nn, k) and arr[f"r{r}_idx"].dtype == np.int32
            assert np.all(np.diff(arr[f"r{r}_idx"], axis=1) > 0)
            assert arr[f"r{r}_idx"].min() >= 0 and arr[f"r{r}_idx"].max() < M
            assert arr[f"r{r}_params"].shape == (nn, k)
            assert arr[f"r{r}_params"].dtype == np.complex64
            assert arr[f"r{r}_counter"].shape == (nn, M) and arr[f"r{r}_counter"].dtype == np.int32
            assert arr[f"r{r}_counter"].sum() == nn * k * (r + 1)
            assert arr[f"r{r}_x"].shape == (nn, n)
            for name in ("acc_enc", "acc_avg"):
                assert (f"r{r}_{name}" in arr) == acc
                if acc:
                    a = arr[f"r{r}_{name}"]
                    assert a.shape == (nn, M) and a.dtype == np.complex64
            if acc:  # the rewind: nothing is owed at what was just sent
                rows = np.arange(nn)[:, None]
                assert not arr[f"r{r}_acc_enc"][rows, arr[f"r{r}_idx"]].any()
                if not aac:  # no post-step bookkeeping in this mode
                    assert np.array_equal(arr[f"r{r}_acc_enc"], arr[f"r{r}_acc_avg"])
        for name, a in arr.items():
            if a.dtype in (np.float32, np.complex64):
                f = a.view(np.float32)
                assert np.isfinite(f).all() and not np.signbit(f[f == 0]).any(), name
    adj = ops.run_adjacency(run_named("irr6")[0])
    assert sorted(len(a) for a in adj) == [1, 1, 2, 3, 3, 4]
    assert ops.run_adjacency(run_named("plain6")[0]) == adj


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_single_rank_engine_reproduces_the_reference(meta, arr):
    eng = _engine(meta, arr)
    assert eng.M == meta["m_len"] and eng.k == meta["k"] and not eng.coll and eng.recv is None
    rows = [eng.x, eng.x0, eng.fx, eng.ch, eng.key, eng.counter]
    rows += [eng.acc] if meta["accumulation"] else []
    assert (eng.acc is None) == (not meta["accumulation"])
    for t in rows:
        # a row every 256 bytes from the buffer's start (which the host allocator aligns to 64)
        assert t.data_ptr() % 64 == 0 and (t.stride(0) * t.element_size()) % 256 == 0
    assert eng.fx.dtype == eng.ch.dtype == torch.complex64 and eng.counter.dtype == torch.int32
    assert torch.equal(eng.x0, eng.x) and not eng.counter.any()
    assert eng.send.numel() == 2 * eng.per * eng._slot and eng._slot % 64 == 0 \
        and eng._slot >= 2 * eng.k  # 4 k words per node, padded to 256-byte slots
    legs = []
    eng.step(mark=legs.append)
    assert legs == ["encode", "exchange", "fold", "post"]
    errs = {}
    ops.drive(_engine(meta, arr), meta, arr, errs=errs)
    print(meta["name"], {w: round(max(v), 4) for w, v in errs.items()})


def test_engine_rejects_what_it_does_not_implement():
    from decentralizepy_amd.gossip_fft import FftRound
    adj = ops.adjacency(6, ops.EDGES_IRR6)
    x = torch.zeros(6, 40)
    kw = dict(device=CPU, ops=ops.OracleFftOps())
    for bad in (dict(exchange="peer"), dict(compress=True), dict(compression_class="Elias"),
                dict(streams=3), dict(wavelet="sym2")):
        with pytest.raises(ValueError, match="unknown arguments"):
            FftRound(adj, x, 0.1, **kw, **bad)
    for n in (41, 39, 5):
        with pytest.raises(ValueError, match="reshape"):
            FftRound(adj, torch.zeros(6, n), 0.1, **kw)
    for n in (2, 3):
        with pytest.raises(ValueError, match="even N >= 4"):
            FftRound(adj, torch.zeros(6, n), 0.5, **kw)
    with pytest.raises(ValueError, match="KeyError"):
        FftRound(adj, x, 1.0, **kw)  # the default metadata_cap is 1.0
    with pytest.raises(ValueError, match="KeyError"):
        FftRound(adj, x, 0.5, metadata_cap=0.5, **kw)
    with pytest.raises(ValueError, match="k = round"):
        FftRound(adj, x, 0.01, **kw)  # round(0.01 * 21) = 0
    with pytest.raises(ValueError, match="change_based_selection"):
        FftRound(adj, x, 0.1, change_based_selection=False, **kw)
    with pytest.raises(ValueError, match="rows"):
        FftRound(adj, x[:5], 0.1, **kw)
    with pytest.raises(ValueError, match="rank"):
        FftRound(adj, x, 0.1, rank=2, world=2, **kw)
    eng = FftRound(adj, torch.zeros(6, 4), 0.4, **kw)  # the smallest model: M = 3, k = 1
    assert (eng.M, eng.k, eng.acc_mode) == (3, 1, 0)
    assert FftRound(adj, x, 0.1, accumulation=True, **kw).acc_mode == 1
    assert FftRound(adj, x, 0.1, accumulation=True, accumulate_averaging_changes=True,
                    **kw).acc_mode == 2
    # the reference ignores accumulate_averaging_changes without accumulation
    plain = FftRound(adj, x, 0.1, accumulate_averaging_changes=True, **kw)
    assert plain.acc_mode == 0 and plain.acc is None and not plain.aac


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
        got = ops.drive(eng, meta, arr, lo=lo, every_payload=True)
    finally:
        dist.all_gather_into_tensor = real
    one_buffer_per_round = (len(gathers) == meta["rounds"]
                            and all(o == world * i and i % 64 == 0 for o, i in gathers))
    return lo, hi, one_buffer_per_round, got


@pytest.mark.parametrize("name,world", [("irr6", 2), ("reg16", 3), ("plain6", 3), ("reg16", 2)])
def test_gloo_worlds_reproduce_the_reference_and_agree_bit_for_bit(name, world):
    meta, arr = run_named(name)
    nn = meta["nodes"]
    res = spawn_gloo(_worker, world, name)
    assert len(res) == world and sum(hi - lo for lo, hi, _, _ in res) == nn
    assert all(ok for _, _, ok, _ in res)
    one = ops.drive(_engine(meta, arr), meta, arr)
    for lo, hi, _, got in res:
        mine = []
        for rnd in one:  # the one-rank run's rows [lo, hi) and every payload
            d = {key: v for key, v in rnd.items() if key.startswith(("idx", "vals"))}
            d.update({key: rnd[key][lo:hi] for key in ("x", "counter", "acc", "acc_enc")
                      if key in rnd})
            mine.append(d)
        ops.same_bits(got, mine)
        assert all(f"vals{u}" in rnd for rnd in got for u in range(nn))


def test_one_rank_with_a_group_gathers_as_a_loopback():
    lo, hi, ok, got = spawn_gloo(_worker, 1, "irr6", True)[0]
    assert (lo, hi, ok) == (0, 6, True)
    meta, arr = run_named("irr6")
    ops.same_bits(got, ops.drive(_engine(meta, arr), meta, arr))


# ---- the round's calls with stubs for the library -------------------------------------------------
def test_step_is_one_call_per_leg_whatever_the_node_count(monkeypatch):
    """The call sequence of a step with stubs for the codec wrappers, the fold and the
    collective: one pair transform of 2 m jobs, one encode, one all-gather, the guarded fold, one
    inverse and, with accumulate_averaging_changes, one accumulating transform of m jobs; the same
    calls for 6 and for 16 nodes, no device value read."""
    from decentralizepy_amd import _lib, codec
    from decentralizepy_amd.gossip_fft import FftRound
    calls = []

    class Tab:
        def __init__(self, kind, m, flag=None):
            self.kind, self.m, self.flag = kind, m, flag

    class Lib:
        @staticmethod
        def dpz_cplx_encode_workspace_bytes(m, n):
            return 256

        @staticmethod
        def dpz_decode_workspace_bytes(n, p):
            return 256

        @staticmethod
        def dpz_decode_average_batch_guarded(m, local, out, n, counts, idx, val, k, w, w_self,
                                             flags, guard, guard_n, stream):
            calls.append(("guarded", m, n, flags, guard_n,
                          [k[i] for i in range(sum(counts[j] for j in range(m)))]))
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: Lib)
    monkeypatch.setattr(_lib, "check", lambda rc, what: None if rc == 0 else pytest.fail(what))
    monkeypatch.setattr(codec, "fft_native", lambda n: True)
    monkeypatch.setattr(codec, "FftNodesTable", lambda x, x0, out, acc, dev:
                        Tab("fft", len(x), acc))
    monkeypatch.setattr(codec, "IfftNodesTable", lambda c, out, dev: Tab("ifft", len(c)))
    monkeypatch.setattr(codec, "CplxEncodeTable", lambda *c: Tab("enc", len(c[0])))
    monkeypatch.setattr(codec, "fft_nodes_workspace", lambda jobs, n, dev: ("ws", jobs, n))
    monkeypatch.setattr(codec, "rfft_nodes", lambda tab, n, ws:
                        calls.append(("rfft", tab.kind, tab.m, tab.flag, n, ws)))
    monkeypatch.setattr(codec, "irfft_nodes", lambda tab, n, ws:
                        calls.append(("irfft", tab.kind, tab.m, n)))
    monkeypatch.setattr(codec, "cplx_encode_nodes", lambda tab, n, k, mode, ws:
                        calls.append(("encode", tab.kind, tab.m, n, k, mode)))
    monkeypatch.setattr(dist, "all_gather_into_tensor", lambda out, inp, group=None:
                        calls.append(("all_gather", out.numel(), inp.numel(), group)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type(
        "S", (), {"cuda_stream": 0})())
    monkeypatch.setattr(torch.Tensor, "item", lambda self: pytest.fail("a device value was read"))
    names = {}
    for name in RUN_IDS:
        meta, arr = run_named(name)
        nn, n, M, k = meta["nodes"], meta["n"], meta["m_len"], meta["k"]
        eng = FftRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]), group="g",
                       device=CPU, **ops.engine_kwargs(meta))  # the HIP path
        del calls[:]
        eng.step()
        eng.step()
        per_round = len(calls) // 2
        assert calls[:per_round] == calls[per_round:]
        c = calls[:per_round]
        want = ["rfft", "encode", "all_gather", "guarded", "irfft"]
        want += ["rfft"] if meta["accumulate_averaging_changes"] else []
        assert [x[0] for x in c] == want
        assert c[0] == ("rfft", "fft", 2 * nn, False, n, ("ws", 2 * nn, n))
        assert c[1] == ("encode", "enc", nn, M, k, eng.acc_mode)
        assert c[2][1] == c[2][2] == 2 * nn * eng._slot and c[2][3] == "g"
        n_pay = sum(len(a) for a in ops.run_adjacency(meta))
        assert c[3] == ("guarded", nn, 2 * M, _lib.DPZ_FOLD_SELF, 1, [2 * k] * n_pay)
        assert c[4] == ("irfft", "ifft", nn, n)
        if meta["accumulate_averaging_changes"]:
            assert c[5] == ("rfft", "fft", nn, True, n, ("ws", 2 * nn, n))
        names[name] = [x[0] for x in c]
    assert names["reg16"] == names["plain6"]  # 16 nodes and 6 nodes: the same calls


# ---- the C entry points: every check is made on the host, before any device call ----------------
def test_argument_validation_without_gpu():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    ARG, UNSUP, WS = _lib.DPZ_ERR_ARG, _lib.DPZ_ERR_UNSUPPORTED, _lib.DPZ_ERR_WORKSPACE
    d, big = 4096, 1 << 40  # d is never dereferenced: the checks come first

    def table(rows, words):
        host = np.array(rows, dtype=np.uint64).reshape(-1, words)
        return host, ctypes.c_void_p(host.ctypes.data)

    def fwd(rows, jobs=None, tab=d, n=1030, ws=d, wsb=big, host=True):
        h, p = table(rows, 4)
        return L.dpz_rfft_nodes(len(h) if jobs is None else jobs, tab, p if host else None, n, ws,
                                wsb, None)

    def inv(rows, jobs=None, tab=d, n=1030, ws=d, wsb=big, host=True):
        h, p = table(rows, 2)
        return L.dpz_irfft_nodes(len(h) if jobs is None else jobs, tab, p if host else None, n,
                                 ws, wsb, None)

    # the workspace: one M-complex row per job, a second where the plan has two passes or more
    assert L.dpz_fft_nodes_workspace_bytes(3, 514) == 3 * 2304 + 256       # 257: one pass
    assert L.dpz_fft_nodes_workspace_bytes(3, 1030) == 2 * 3 * 4352 + 256  # 515 = 103 * 5: two
    assert L.dpz_fft_nodes_workspace_bytes(3, 131584) == 2 * 3 * 526336 + 256
    for jobs, n in ((0, 1030), (-1, 1030), (3, 1031), (3, 2), (3, 0), (3, -4), (3, 8198),
                    (3, 89834)):
        assert L.dpz_fft_nodes_workspace_bytes(jobs, n) == -1, (jobs, n)
    assert L.dpz_fft_native(8198) == 0 and L.dpz_fft_native(1030) == 1

    two = [[256, 512, 1024, 0], [2048, 0, 4096, 1]]
    pair = [[256, 512], [1024, 2048]]
    for call, rows in ((fwd, two), (inv, pair)):
        assert call(rows, jobs=0) == ARG and call(rows, jobs=-2) == ARG
        assert call(rows, tab=None) == ARG and call(rows, host=False) == ARG
        assert call(rows, tab=d + 4) == ARG
        for n in (1031, 3, 2, 0, -6, 8198, 89834):  # odd, too short, a hipFFT size
            assert call(rows, n=n) == UNSUP, n
        assert call(rows, ws=None) == WS and call(rows, wsb=100) == WS
        assert call(rows, wsb=L.dpz_fft_nodes_workspace_bytes(2, 1030) - 1) == WS
        assert call([rows[0]] * 65536) == UNSUP
        for col in range(len(rows[0]) - (call is fwd)):  # a row that is not 8-byte aligned
            row = list(rows[0])
            row[col] += 4
            assert call([row, rows[1]]) == ARG, col
    assert fwd([[0, 0, 1024, 0]]) == ARG and fwd([[256, 0, 0, 0]]) == ARG  # no x, no out
    assert fwd([[256, 0, 1024, 2]]) == ARG                                # a flag above 1
    assert inv([[0, 512]]) == ARG and inv([[256, 0]]) == ARG
    # a refusal by the size comes before the rows are looked at
    assert fwd([[0, 0, 0, 0]], n=8198) == UNSUP

    C = L.dpz_cplx_chunk_elems()
    assert C > 0 and C % 1024 == 0
    M = 2051
    need = L.dpz_cplx_encode_workspace_bytes(3, M)
    assert need >= 3 * 256 and L.dpz_cplx_encode_workspace_bytes(6, M) == 2 * need
    assert L.dpz_cplx_encode_workspace_bytes(0, M) == 0
    assert L.dpz_cplx_encode_workspace_bytes(3, 0) == 0

    def enc(m=3, tab=d, n=M, k=205, mode=0, ws=d, wsb=need):
        return L.dpz_cplx_encode_nodes(m, tab, n, k, mode, ws, wsb, None)

    for bad in (dict(m=0), dict(m=-1), dict(tab=None), dict(ws=None), dict(n=0), dict(n=-5),
                dict(n=1 << 30, wsb=big), dict(k=0), dict(k=-1), dict(k=M + 1), dict(mode=3),
                dict(mode=-1), dict(wsb=need - 1), dict(wsb=0), dict(tab=d + 4), dict(ws=d + 2)):
        assert enc(**bad) == ARG, bad
    assert enc(m=65536, wsb=big) == UNSUP
    assert L.dpz_abi_version() == 2  # symbols were added, nothing changed


def test_header_library_and_ctypes_table_agree():
    from decentralizepy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "dpz_codec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dpz_[a-z0-9_]+)\s*\(", text))
    new = {"dpz_fft_nodes_workspace_bytes": 2, "dpz_rfft_nodes": 7, "dpz_irfft_nodes": 7,
           "dpz_cplx_chunk_elems": 0, "dpz_cplx_encode_workspace_bytes": 2,
           "dpz_cplx_encode_nodes": 8}
    assert set(new) <= declared and set(_lib.SIGNATURES) == declared
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in new.items():
        assert hasattr(handle, name) and len(_lib.SIGNATURES[name][1]) == nargs
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    assert all(name in doc for name in new)


def test_tables_lay_out_the_documented_words():
    from decentralizepy_amd import codec
    x, x0 = torch.zeros(3, 8), torch.zeros(3, 8)
    fx, ch = torch.zeros(3, 5, dtype=torch.complex64), torch.zeros(3, 5, dtype=torch.complex64)
    acc = torch.zeros(3, 5, dtype=torch.complex64)
    key, counter = torch.zeros(3, 5), torch.zeros(3, 5, dtype=torch.int32)
    send = torch.zeros(3, 16, dtype=torch.int32)
    p = lambda t: [t[j].data_ptr() for j in range(3)]  # noqa: E731
    pre = codec.FftNodesTable(list(x) + list(x), [None] * 3 + list(x0), list(fx) + list(ch),
                              False, CPU)
    want = [[a, 0, o, 0] for a, o in zip(p(x), p(fx))]
    want += [[a, b, o, 0] for a, b, o in zip(p(x), p(x0), p(ch))]
    assert pre.m == 6 and pre.dev.dtype == torch.int64
    assert pre.dev.tolist() == pre.host.tolist() == [v for row in want for v in row]
    post = codec.FftNodesTable(x, x0, acc, True, CPU)
    assert post.host.tolist() == [v for a, b, o in zip(p(x), p(x0), p(acc)) for v in (a, b, o, 1)]
    mixed = codec.FftNodesTable(x, None, acc, [0, 1, 0], CPU)
    assert mixed.host.reshape(3, 4)[:, 3].tolist() == [0, 1, 0]
    assert not mixed.host.reshape(3, 4)[:, 1].any()
    it = codec.IfftNodesTable(ch, x, CPU)
    assert it.dev.tolist() == [v for c, o in zip(p(ch), p(x)) for v in (c, o)]
    enc = codec.CplxEncodeTable(ch, acc, fx, key, counter, send[:, :4], send[:, 8:12], CPU)
    rows = zip(p(ch), p(acc), p(fx), p(key), p(counter), p(send))
    assert enc.dev.tolist() == [v for c, a, f, k_, n_, s in rows
                                for v in (c, a, f, k_, n_, s, s + 32, 0)]
    bare = codec.CplxEncodeTable([ch[1]], None, [fx[1]], [key[1]], None, [send[1, :4]],
                                 [send[1, 8:12]], CPU)
    assert bare.host.tolist() == [ch[1].data_ptr(), 0, fx[1].data_ptr(), key[1].data_ptr(), 0,
                                  send[1].data_ptr(), send[1].data_ptr() + 32, 0]
    for bad_k in (0, 6):
        with pytest.raises(ValueError, match="outside"):
            codec.cplx_encode_nodes(enc, 5, bad_k)
    with pytest.raises(ValueError, match="null row"):
        codec.cplx_encode_nodes(bare, 5, 2, codec.DPZ_ACC_ADD)
