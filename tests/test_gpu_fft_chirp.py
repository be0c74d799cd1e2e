"""GPU: the chirp-z real FFTs (csrc/dpz_fft.hip, dpz_rfft_chirp_nodes / dpz_irfft_chirp_nodes) and
the FFT round with ``chirp=True`` at sizes without a native plan.

Accuracy.  E(y) = ||y - ref||_2 / ||ref||_2 against numpy's float64 transform of the same fp32
input, held to E <= 4 max(E_ref, E_emu, eps): E_ref is the figure of torch's CPU fp32 transform at
that n, E_emu that of the fp32 restatement of this algorithm in tests/fft_chirp_ops.py (both
computed here on the CPU).  Measured on an MI355X: DESIGN.md section 3.7.

The launch-count test compares what the library's own timing counters see.  hipFFT's kernels and
the elementwise calls are not among them, so a default engine has no "fft" count to compare: its
per-node legs show as one "fft_scale" launch per node (the 1 / n after each hipFFT inverse),
where the ``chirp=True`` engine's counts are the same for 1 and 3 nodes."""
import numpy as np
import pytest
import torch

from tests import fft_chirp_ops as cops
from tests import fft_round_ops as ops
from tests.dist_harness import rccl_loopback
from tests.test_gpu_fft_conformance import bound as native_bound

pytestmark = pytest.mark.gpu

EPS, rel, c64 = cops.EPS, cops.rel, np.complex64
PAD = 7.0


def dev_rfft(a, dev):
    from decentralizepy_amd import codec
    return codec.rfft(torch.tensor(a).to(dev), chirp=True).cpu().numpy()


def dev_irfft(a, n, dev):
    from decentralizepy_amd import codec
    return codec.irfft(torch.tensor(a).to(dev), n, chirp=True).cpu().numpy()


def test_sizes_reach_the_edges_of_the_padding():
    from decentralizepy_amd import codec
    P = {n: codec.fft_chirp_length(n) for n in cops.SIZES}
    assert all(P[n] == cops.chirp_length(n) for n in cops.SIZES)
    assert (P[4], P[6]) == (3, 5)                                    # L = 2 and 3
    assert any(P[n] == n - 1 for n in cops.SWEEP) and any(P[n] == n for n in cops.SWEEP)
    assert max(P[n] for n in cops.SWEEP) <= 256                      # one-pass P
    assert [codec.fft_native(n) for n in cops.FORCED] == [True] * 3
    assert [codec.fft_native(n) for n in cops.NO_PLAN] == [False] * 4
    assert (P[8198], P[89_834]) == (8232, 90_000)


@pytest.mark.parametrize("n", cops.SIZES)
def test_random_accuracy(dev, n):
    """rfft, irfft of an arbitrary spectrum and the round trip: E <= 4 max(E_ref, E_emu, eps)."""
    c = cops.random_case(n)
    f = dev_rfft(c["x"], dev)
    errs = {"fwd": rel(f, c["fwd"]), "inv": rel(dev_irfft(c["spec"], n, dev), c["inv"]),
            "rt": rel(dev_irfft(f, n, dev), c["x64"])}
    print(n, {k: (round(e / EPS, 2), round(c["ref"][k] / EPS, 2), round(c["emu"][k] / EPS, 2))
              for k, e in errs.items()})
    for what, e in errs.items():
        b = cops.bound(c["ref"][what], c["emu"][what])
        assert e <= b, (what, n, e / EPS, b / EPS)


@pytest.mark.parametrize("n", cops.STRUCTURED)
def test_structured_inputs(dev, n):
    """Unit impulses and tones, each with its own E_ref and E_emu: a chirp exponent reduced in
    floating point loses these at the far indices."""
    P = cops.chirp_length(n)
    for name, x in cops.structured(n):
        ref = np.fft.rfft(x.astype(np.float64))
        e_ref = rel(torch.fft.rfft(torch.from_numpy(x)).numpy(), ref)
        e_emu = rel(cops.emu_rfft(x, P), ref)
        e = rel(dev_rfft(x, dev), ref)
        print(n, name, round(e / EPS, 2), round(e_ref / EPS, 2), round(e_emu / EPS, 2))
        assert e <= cops.bound(e_ref, e_emu), (n, name, e / EPS, e_ref / EPS, e_emu / EPS)


@pytest.mark.parametrize("n", cops.STRUCTURED)
def test_constant_vector(dev, n):
    """The DC bin within the random-input bound of n * c; every other bin within
    4 max(E_rand, r / ||x||, eps) ||x||, r the largest other-bin error of the reference's and
    of the restatement's transform of the same vector."""
    c = cops.random_case(n)
    x32 = np.full(n, cops.FLAT_C, np.float32)
    ref = np.zeros(n // 2 + 1, np.complex128)
    ref[0] = n * cops.FLAT_C
    nx = float(np.linalg.norm(x32.astype(np.float64)))
    e_peak, e_rest = cops.flat_errors(dev_rfft(x32, dev), ref)
    r_ref = cops.flat_errors(torch.fft.rfft(torch.from_numpy(x32)).numpy(), ref)[1]
    r_emu = cops.flat_errors(cops.emu_rfft(x32, cops.chirp_length(n)), ref)[1]
    b_rand = cops.bound(c["ref"]["fwd"], c["emu"]["fwd"])
    b_peak = b_rand * n * cops.FLAT_C
    b_rest = cops.bound(c["ref"]["fwd"], c["emu"]["fwd"], r_ref / nx, r_emu / nx) * nx
    print(n, e_peak / b_peak, e_rest / b_rest, r_ref / nx / EPS, r_emu / nx / EPS)
    assert e_peak <= b_peak, (n, e_peak, b_peak)
    assert e_rest <= b_rest, (n, e_rest, b_rest)


# ---- jobs and rows --------------------------------------------------------------------------------
def _rows(dev, data, off, pad=PAD):
    """Device rows of ``data``, each ``off`` elements into a prefilled backing row."""
    m, n = data.shape
    back = torch.full((m, -(-(n + 8) // 32) * 32), pad, dtype=torch.from_numpy(data).dtype,
                      device=dev)
    view = back[:, off:off + n]
    view.copy_(torch.from_numpy(data).to(dev))
    return view, back


def _intact(back, n, off, pad=PAD):
    return bool((back[:, :off] == pad).all() and (back[:, off + n:] == pad).all())


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _exact_ws(codec, jobs, n, dev):
    """A workspace of exactly the stated bytes inside guard bytes."""
    need = int(codec._lib.lib().dpz_fft_chirp_nodes_workspace_bytes(jobs, n))
    back = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device=dev)
    return back[128:128 + need], back, need


@pytest.mark.parametrize("n", [10, 8198])
def test_jobs_and_rows(dev, n):
    from decentralizepy_amd import codec
    M, J = n // 2 + 1, 5
    rng = np.random.default_rng(n)
    x = rng.standard_normal((J, n)).astype(np.float32)
    x0 = (x + 0.1 * rng.standard_normal((J, n))).astype(np.float32)
    acc = (rng.standard_normal((J, M)) + 1j * rng.standard_normal((J, M))).astype(c64)
    with_x0 = [False, True, True, False, True]
    accum = [False, False, True, True, True]
    tx, bx = _rows(dev, x, 2)
    t0, b0 = _rows(dev, x0, 2)
    init = np.where(np.array(accum)[:, None], acc, np.full((J, M), PAD, c64))
    out, bout = _rows(dev, init, 1)
    ws, wback, need = _exact_ws(codec, J, n, dev)
    entry = lambda j, o: ([tx[j]], [t0[j] if with_x0[j] else None], [o], [accum[j]])  # noqa: E731
    tab = codec.FftNodesTable(list(tx), [t0[j] if with_x0[j] else None for j in range(J)],
                              list(out), accum, dev)
    assert codec.rfft_chirp_nodes(tab, n, ws) == 0
    ws1, wback1, _ = _exact_ws(codec, 1, n, dev)
    for j in range(J):
        # the same entry alone as one job
        alone, balone = _rows(dev, init[j:j + 1], 1)
        codec.rfft_chirp_nodes(codec.FftNodesTable(*entry(j, alone[0]), dev), n, ws1)
        assert np.array_equal(_bits(out[j]), _bits(alone[0])), (n, j)
        assert _intact(balone, M, 1)
        # the plain transform of SUB(x, x0), ADDed into the prior output
        src = tx[j].contiguous()
        if with_x0[j]:
            src = codec.elementwise(codec.DPZ_EW_SUB, src, t0[j].contiguous())
        want = codec.rfft(src, chirp=True)
        if accum[j]:
            a = torch.view_as_real(torch.from_numpy(acc[j]).to(dev)).reshape(-1).clone()
            codec.elementwise(codec.DPZ_EW_ADD, a, torch.view_as_real(want).reshape(-1), out=a)
            want = torch.view_as_complex(a.view(-1, 2))
        assert np.array_equal(_bits(out[j]), _bits(want)), (n, j, with_x0[j], accum[j])
    assert _intact(bout, M, 1) and _intact(bx, n, 2) and _intact(b0, n, 2)
    assert np.array_equal(_bits(tx), x.view(np.uint32))
    assert np.array_equal(_bits(t0), x0.view(np.uint32))
    # the inverse of arbitrary coefficients, which are only read
    co, bco = _rows(dev, acc, 1)
    back, bback = _rows(dev, np.full((J, n), PAD, np.float32), 2)
    assert codec.irfft_chirp_nodes(codec.IfftNodesTable(list(co), list(back), dev), n, ws) == 0
    for j in range(J):
        alone, balone = _rows(dev, np.full((1, n), PAD, np.float32), 2)
        codec.irfft_chirp_nodes(codec.IfftNodesTable([co[j]], [alone[0]], dev), n, ws1)
        assert np.array_equal(_bits(back[j]), _bits(alone[0])), (n, j)
        assert _intact(balone, n, 2)
        want = codec.irfft(torch.from_numpy(acc[j].copy()).to(dev), n, chirp=True)
        assert np.array_equal(_bits(back[j]), _bits(want)), (n, j)
    assert np.array_equal(_bits(co), acc.view(np.uint32))
    assert _intact(bco, M, 1) and _intact(bback, n, 2)
    for wb, nb in ((wback, need), (wback1, wback1.numel() - 512)):
        assert bool((wb[:128] == 0x5A).all() and (wb[128 + nb:] == 0x5A).all())
    # one byte less is refused before anything is written
    before = _bits(out).copy()
    rc = codec.rfft_chirp_nodes(tab, n, ws[:need - 1], check_rc=False)
    assert rc == codec._lib.DPZ_ERR_WORKSPACE and np.array_equal(_bits(out), before)


@pytest.mark.parametrize("n", [1030, 4100])
def test_against_the_native_kernels(dev, n):
    """rfft(chirp=True) against rfft() at sizes with a native plan: within the sum of both
    bounds."""
    from decentralizepy_amd import codec
    c = cops.random_case(n)
    x = torch.tensor(c["x"]).to(dev)
    a, b = codec.rfft(x, chirp=True).cpu().numpy(), codec.rfft(x).cpu().numpy()
    both = cops.bound(c["ref"]["fwd"], c["emu"]["fwd"]) + native_bound(c["ref"]["fwd"], n)
    d = float(np.linalg.norm(a.astype(np.complex128) - b) / np.linalg.norm(c["fwd"]))
    print(n, d / EPS, both / EPS)
    assert d <= both
    ia = codec.irfft(torch.tensor(c["spec"]).to(dev), n, chirp=True).cpu().numpy()
    ib = codec.irfft(torch.tensor(c["spec"]).to(dev), n).cpu().numpy()
    both = cops.bound(c["ref"]["inv"], c["emu"]["inv"]) + native_bound(c["ref"]["inv"], n)
    assert float(np.linalg.norm(ia.astype(np.float64) - ib) / np.linalg.norm(c["inv"])) <= both


# ---- the engine -----------------------------------------------------------------------------------
RUN = cops.load_run()


def _engine(dev, **kw):
    from decentralizepy_amd.gossip_fft import FftRound
    meta, arr = RUN
    return FftRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]).to(dev), device=dev,
                    **ops.engine_kwargs(meta), **kw)


def test_engine_reproduces_the_reference_at_a_size_without_a_plan(dev):
    meta, arr = RUN
    eng = _engine(dev, chirp=True)
    assert eng.batched and not eng.native and eng.x.is_cuda
    errs = {}
    got = ops.drive(eng, meta, arr, errs=errs)
    print("chirp", {w: round(max(v), 4) for w, v in errs.items()})
    plain = _engine(dev)
    assert not plain.batched and not plain.native and not plain.chirp
    errs = {}
    ref = ops.drive(plain, meta, arr, errs=errs)
    print("default", {w: round(max(v), 4) for w, v in errs.items()})
    for a, b in zip(got, ref):
        for name in a:
            if name.startswith("idx") or name == "counter":
                assert np.array_equal(a[name], b[name]), name


def test_chirp_changes_nothing_at_a_native_size(dev):
    from decentralizepy_amd.gossip_fft import FftRound
    adj = ops.adjacency(6, ops.EDGES_IRR6)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((6, 1030))
                         .astype(np.float32)).to(dev)
    kw = dict(accumulation=True, accumulate_averaging_changes=True, device=dev)
    a, b = FftRound(adj, x, 0.1, chirp=True, **kw), FftRound(adj, x, 0.1, **kw)
    assert a.native and a.batched and b.native and b.batched
    for e in (a, b):
        for _ in range(2):
            e.x += 0.01
            e.step()
    for name in ("x", "fx", "ch", "acc", "counter"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_chirp_step_launch_count_is_independent_of_the_node_count(dev):
    """A ``chirp=True`` step at N = 8,198 with m = 1 and m = 3 from the library's timing counters:
    equal, kernel by kernel (P = 8,232 = 98 * 84: two passes, so 2 * 2 + 3 launches per transform
    set and three sets).  The default engine's per-node legs grow with the node count."""
    from decentralizepy_amd import codec
    from decentralizepy_amd.gossip_fft import FftRound
    n = 8198
    seen = {}
    for chirp in (True, False):
        for adj in ([set()], [{1, 2}, {0}, {0}]):
            x = torch.from_numpy(np.random.default_rng(3).standard_normal((len(adj), n))
                                 .astype(np.float32)).to(dev)
            eng = FftRound(adj, x, 0.1, accumulation=True, accumulate_averaging_changes=True,
                           device=dev, chirp=chirp)
            eng.x += 0.01
            eng.step()
            eng.x += 0.01
            with codec.KernelTimer() as t:
                eng.step()
            seen[chirp, len(adj)] = {name: cnt for name, (_, cnt) in t.result.items()}
    one, three = seen[True, 1], seen[True, 3]
    pick = lambda d: {k: v for k, v in d.items()  # noqa: E731
                      if k.startswith(("fft", "topk_exact", "cplx"))}
    assert pick(one) == pick(three)
    for counts in (one, three):
        assert counts["fft"] == 3 * (2 * 2 + 3)
        assert "fft_scale" not in counts and "cplx" not in counts
    d1, d3 = seen[False, 1], seen[False, 3]
    # hipFFT's kernels (and the elementwise ones) are not among the library's counters: of the
    # default engine's per-node transform legs they see the 1 / n scaling after each hipFFT inverse
    assert "fft" not in d1 and "fft" not in d3
    assert (d1["fft_scale"], d3["fft_scale"]) == (1, 3)
    assert pick(d1) != pick(d3)


def test_chirp_step_never_waits_for_the_device(dev, monkeypatch):
    eng = _engine(dev, chirp=True)
    eng.step()

    def no_wait(*a, **kw):
        raise AssertionError("the step waited for the device")

    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "synchronize", no_wait)
        mp.setattr(torch.cuda.Stream, "synchronize", no_wait)
        mp.setattr(torch.cuda.Event, "synchronize", no_wait)
        mp.setattr(torch.Tensor, "item", no_wait)
        mp.setattr(torch.Tensor, "cpu", no_wait)
        eng.step()
    torch.cuda.synchronize(dev)
    assert eng.round == 2 and torch.equal(eng.x, eng.x0)


def test_chirp_engine_through_rccl_loopback_equals_the_in_place_engine(dev):
    meta, arr = RUN
    with rccl_loopback(dev) as group:
        eng = _engine(dev, chirp=True, rank=0, world=1, group=group)
        assert eng.coll and eng.recv is not None and eng.batched and not eng.native
        got = ops.drive(eng, meta, arr, every_payload=True)
    ops.same_bits(got, ops.drive(_engine(dev, chirp=True), meta, arr, every_payload=True))
