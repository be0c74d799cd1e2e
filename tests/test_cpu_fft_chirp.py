"""CPU: the chirp-z real FFTs' host side (dpz_fft_chirp_length, the workspace, every argument
check of dpz_rfft_chirp_nodes / dpz_irfft_chirp_nodes without a device), the FFT round with
``chirp=True`` over the recorded reference run of a size without a native plan (N = 8,198; the numpy
oracle standing in for the kernels) and the library calls of a ``chirp=True`` step.  The kernels
are covered by tests/test_gpu_fft_chirp.py."""
import ctypes

import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests import fft_chirp_ops as cops
from tests import fft_round_ops as ops

CPU = torch.device("cpu")
NO_PLAN = (8198, 24_594, 89_834)


def test_chirp_length_follows_its_rule():
    from decentralizepy_amd import _lib, codec
    L = _lib.lib()
    for n in (5, 7, 1031, 3, 2, 1, 0, -6, -4, (1 << 30) + 2, (1 << 30) + 1, 1 << 31, 1 << 40):
        assert L.dpz_fft_chirp_length(n) == 0 == cops.chirp_length(n), n
    assert cops.is_prime(4099) and cops.is_prime(44_917)
    assert NO_PLAN == (2 * 4099, 6 * 4099, 2 * 44_917)
    for n in list(range(4, 4201, 2)) + list(NO_PLAN):
        P = L.dpz_fft_chirp_length(n)
        assert P == cops.chirp_length(n) == codec.fft_chirp_length(n), n
        assert P >= n - 1 and L.dpz_fft_native(2 * P) == 1, (n, P)
    for n in NO_PLAN:
        assert L.dpz_fft_native(n) == 0, n
    assert [L.dpz_fft_chirp_length(n) for n in (4, 6, 8, 10, 12, 66, 8198, 89_834)] == \
        [3, 5, 7, 9, 12, 70, 8232, 90_000]
    assert L.dpz_fft_chirp_length(1 << 30) == 1 << 30  # 2^30 - 1 has the prime factor 331


def test_argument_validation_without_gpu():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    ARG, UNSUP, WS = _lib.DPZ_ERR_ARG, _lib.DPZ_ERR_UNSUPPORTED, _lib.DPZ_ERR_WORKSPACE
    d, big = 4096, 1 << 40  # d is never dereferenced: the checks come first

    def table(rows, words):
        host = np.array(rows, dtype=np.uint64).reshape(-1, words)
        return host, ctypes.c_void_p(host.ctypes.data)

    def fwd(rows, jobs=None, tab=d, n=8198, ws=d, wsb=big, host=True):
        h, p = table(rows, 4)
        return L.dpz_rfft_chirp_nodes(len(h) if jobs is None else jobs, tab, p if host else None,
                                      n, ws, wsb, None)

    def inv(rows, jobs=None, tab=d, n=8198, ws=d, wsb=big, host=True):
        h, p = table(rows, 2)
        return L.dpz_irfft_chirp_nodes(len(h) if jobs is None else jobs, tab, p if host else None,
                                       n, ws, wsb, None)

    # the workspace: two rows of P complex per job on 256 bytes, and 256 bytes of alignment slack
    need = L.dpz_fft_chirp_nodes_workspace_bytes
    assert need(3, 8198) == 2 * 3 * 66_048 + 256  # P = 8,232: 65,856 bytes, 66,048 on 256
    assert need(1, 4) == 2 * 256 + 256 and need(7, 4) == 7 * 2 * 256 + 256
    for n in (10, 1030, 8198, 89_834):
        one = need(1, n) - 256
        assert one > 0 and one % 512 == 0 and one >= 2 * 8 * cops.chirp_length(n)
        for jobs in (2, 5, 96, 65_535):
            assert need(jobs, n) == jobs * one + 256, (jobs, n)
    for jobs, n in ((0, 8198), (-1, 8198), (3, 1031), (3, 3), (3, 2), (3, 0), (3, -6),
                    (3, (1 << 30) + 2)):
        assert need(jobs, n) == -1, (jobs, n)

    two = [[256, 512, 1024, 0], [2048, 0, 4096, 1]]
    pair = [[256, 512], [1024, 2048]]
    for call, rows in ((fwd, two), (inv, pair)):
        assert call(rows, jobs=0) == ARG and call(rows, jobs=-2) == ARG
        assert call(rows, tab=None) == ARG and call(rows, host=False) == ARG
        assert call(rows, tab=d + 4) == ARG
        for n in (1031, 3, 2, 0, -6, (1 << 30) + 2):  # odd, too short, too long
            assert call(rows, n=n) == UNSUP, n
        assert call(rows, ws=None) == WS and call(rows, wsb=100) == WS
        assert call(rows, wsb=need(2, 8198) - 1) == WS
        assert call(rows, n=1030, wsb=need(2, 1030) - 1) == WS  # a native size is taken too
        assert call([rows[0]] * 65_536) == UNSUP
        for col in range(len(rows[0]) - (call is fwd)):  # a row that is not 8-byte aligned
            row = list(rows[0])
            row[col] += 4
            assert call([row, rows[1]]) == ARG, col
    assert fwd([[0, 0, 1024, 0]]) == ARG and fwd([[256, 0, 0, 0]]) == ARG  # no x, no out
    assert fwd([[256, 0, 1024, 2]]) == ARG                                # a flag above 1
    assert inv([[0, 512]]) == ARG and inv([[256, 0]]) == ARG
    # a refusal by the size comes before the rows are looked at
    assert fwd([[0, 0, 0, 0]], n=1031) == UNSUP and inv([[0, 0]], n=2) == UNSUP
    assert L.dpz_abi_version() == 2  # symbols were added, nothing changed


def test_header_library_and_ctypes_table_agree_on_the_new_entry_points():
    from decentralizepy_amd import _lib
    new = {"dpz_fft_chirp_length": 1, "dpz_fft_chirp_nodes_workspace_bytes": 2,
           "dpz_rfft_chirp_nodes": 7, "dpz_irfft_chirp_nodes": 7}
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in new.items():
        assert hasattr(handle, name) and len(_lib.SIGNATURES[name][1]) == nargs


# ---- the engine over the recorded run of N = 8,198 --------------------------------------------------
RUN = cops.load_run()


def _engine(meta, arr, **kw):
    from decentralizepy_amd.gossip_fft import FftRound
    return FftRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]), device=CPU,
                    **ops.engine_kwargs(meta), **kw)


def test_fixture_is_the_recorded_run():
    meta, arr = RUN
    assert (meta["name"], meta["nodes"], meta["n"], meta["rounds"], meta["k"]) == \
        ("chirp4", 4, 8198, 2, 410)
    assert meta["shape"] == [90, 90, 98] and meta["seed"] >= 74 and meta["alpha"] == 0.1
    assert meta["accumulation"] and meta["accumulate_averaging_changes"]
    assert meta["min_gap"] >= ops.MIN_GAP and meta["m_len"] == 4100
    assert [len(a) for a in ops.run_adjacency(meta)] == [1, 3, 2, 2]
    assert arr["x0"].shape == (4, 8198) and arr["x0"].dtype == np.float32
    for r in range(2):
        assert arr[f"r{r}_idx"].shape == (4, 410) and arr[f"r{r}_idx"].dtype == np.int32
        assert np.all(np.diff(arr[f"r{r}_idx"], axis=1) > 0)
        assert arr[f"r{r}_params"].shape == (4, 410) and arr[f"r{r}_params"].dtype == np.complex64
        assert arr[f"r{r}_counter"].sum() == 4 * 410 * (r + 1)
        assert arr[f"r{r}_x"].shape == (4, 8198)
        for name in ("acc_enc", "acc_avg"):
            assert arr[f"r{r}_{name}"].shape == (4, 4100)
        rows = np.arange(4)[:, None]
        assert not arr[f"r{r}_acc_enc"][rows, arr[f"r{r}_idx"]].any()
    for name, a in arr.items():
        if a.dtype in (np.float32, np.complex64):
            f = a.view(np.float32)
            assert np.isfinite(f).all() and not np.signbit(f[f == 0]).any(), name


def test_engine_with_injected_ops_accepts_chirp_and_reproduces_the_reference():
    from decentralizepy_amd.gossip_fft import FftRound
    meta, arr = RUN
    errs = {}
    eng = _engine(meta, arr, ops=ops.OracleFftOps(), chirp=True)
    assert eng.chirp is True and eng.M == 4100 and eng.k == 410
    got = ops.drive(eng, meta, arr, errs=errs)
    print({w: round(max(v), 4) for w, v in errs.items()})
    ops.same_bits(got, ops.drive(_engine(meta, arr, ops=ops.OracleFftOps()), meta, arr))
    adj, x = ops.run_adjacency(meta), torch.zeros(4, 40)
    kw = dict(device=CPU, ops=ops.OracleFftOps())
    for bad in (1, 0, "yes", None, np.bool_(True)):
        with pytest.raises(ValueError, match="chirp"):
            FftRound(adj, x, 0.1, chirp=bad, **kw)
    for bad in (dict(bluestein=True), dict(chirp_z=True), dict(exchange="peer")):
        with pytest.raises(ValueError, match="unknown arguments"):
            FftRound(adj, x, 0.1, chirp=True, **kw, **bad)
    assert FftRound(adj, x, 0.1, **kw).chirp is False


# ---- the round's calls with stubs for the library -------------------------------------------------
def _stubbed(monkeypatch, calls):
    from decentralizepy_amd import _lib, codec

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
        def dpz_decode_average_batch_guarded(m, *a):
            calls.append(("guarded", m))
            return 0

    native = _lib.lib().dpz_fft_native  # the library's own answer: 8,198 has no native plan
    monkeypatch.setattr(_lib, "lib", lambda: Lib)
    monkeypatch.setattr(_lib, "check", lambda rc, what: None if rc == 0 else pytest.fail(what))
    monkeypatch.setattr(codec, "fft_native", lambda n: bool(native(n)))
    monkeypatch.setattr(codec, "FftNodesTable", lambda x, x0, out, acc, dev:
                        Tab("fft", len(x), acc))
    monkeypatch.setattr(codec, "IfftNodesTable", lambda c, out, dev: Tab("ifft", len(c)))
    monkeypatch.setattr(codec, "CplxEncodeTable", lambda *c: Tab("enc", len(c[0])))
    monkeypatch.setattr(codec, "fft_nodes_workspace", lambda jobs, n, dev:
                        pytest.fail("the native workspace at a size without a plan"))
    monkeypatch.setattr(codec, "fft_chirp_nodes_workspace", lambda jobs, n, dev:
                        ("chirp_ws", jobs, n))
    for name in ("rfft_nodes", "irfft_nodes"):
        monkeypatch.setattr(codec, name, lambda *a, _n=name: pytest.fail(_n))
    monkeypatch.setattr(codec, "rfft_chirp_nodes", lambda tab, n, ws:
                        calls.append(("rfft_chirp", tab.kind, tab.m, tab.flag, n, ws)))
    monkeypatch.setattr(codec, "irfft_chirp_nodes", lambda tab, n, ws:
                        calls.append(("irfft_chirp", tab.kind, tab.m, n, ws)))
    monkeypatch.setattr(codec, "rfft", lambda x, out=None, workspace=None:
                        calls.append(("rfft",)))
    monkeypatch.setattr(codec, "irfft", lambda c, n, out=None, workspace=None:
                        calls.append(("irfft",)))
    monkeypatch.setattr(codec, "elementwise", lambda *a, **k: calls.append(("ew",)))
    monkeypatch.setattr(codec, "cplx_encode_nodes", lambda tab, n, k, mode, ws:
                        calls.append(("encode", tab.m)))
    monkeypatch.setattr(dist, "all_gather_into_tensor", lambda out, inp, group=None:
                        calls.append(("all_gather",)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type(
        "S", (), {"cuda_stream": 0})())
    monkeypatch.setattr(torch.Tensor, "item", lambda self: pytest.fail("a device value was read"))


def test_chirp_step_is_one_call_per_transform_leg_whatever_the_node_count(monkeypatch):
    """At N = 8,198 (no native plan) a ``chirp=True`` step's three transform legs are one
    ``*_chirp_nodes`` call each, for 6 nodes as for 1; a default engine makes per-node ``rfft``
    calls."""
    from decentralizepy_amd.gossip_fft import FftRound
    calls = []
    _stubbed(monkeypatch, calls)
    N, names = 8198, {}
    g = torch.Generator().manual_seed(3)
    for nn in (1, 6):
        adj = ops.adjacency(nn, ops.EDGES_IRR6 if nn == 6 else [])
        x = torch.randn(nn, N, generator=g)
        kw = dict(group="g", device=CPU, accumulation=True, accumulate_averaging_changes=True)
        eng = FftRound(adj, x, 0.1, chirp=True, **kw)  # the HIP path
        assert eng.batched and not eng.native and eng.chirp
        del calls[:]
        eng.step()
        c = list(calls)
        assert [v[0] for v in c] == ["rfft_chirp", "encode", "all_gather", "guarded",
                                     "irfft_chirp", "rfft_chirp"]
        ws = ("chirp_ws", 2 * nn, N)
        assert c[0] == ("rfft_chirp", "fft", 2 * nn, False, N, ws)
        assert c[4] == ("irfft_chirp", "ifft", nn, N, ws)
        assert c[5] == ("rfft_chirp", "fft", nn, True, N, ws)
        names[nn] = [v[0] for v in c]
        plain = FftRound(adj, x, 0.1, **kw)
        assert not plain.batched and not plain.native and not plain.chirp
        del calls[:]
        plain.step()
        kinds = [v[0] for v in calls]
        assert kinds.count("rfft") == 3 * nn and kinds.count("irfft") == nn
        assert not any(k.endswith("_chirp") for k in kinds)
    assert names[1] == names[6]
