"""GPU: the fused chirp-z real FFTs (csrc/dpz_fft.hip, dpz_rfft_chirp_fused_nodes /
dpz_irfft_chirp_fused_nodes) and the FFT round with ``chirp="fused"``.

Where the padded length and the plan are the unfused call's (8,198 and 16,396: P = 8,232 and
16,464, two passes without a runt) the fused result is the unfused one bit for bit.  Where the plan
differs (1,642: 42 * 40 for 210 * 8; 89,834: 50 * 45 * 40 for 250 * 180 * 2) it is held to the
unfused path's bound, E <= 4 max(E_ref, E_emu, eps) against numpy's float64 transform
(tests/fft_chirp_ops.py), E_emu at ``fft_chirp_fused_length(n)``."""
import numpy as np
import pytest
import torch

from tests import fft_chirp_ops as cops
from tests import fft_round_ops as ops

pytestmark = pytest.mark.gpu

c64 = np.complex64
TABLE = {8198: 8232, 16_396: 16_464, 24_594: 24_696, 1642: 1680, 89_834: 90_000}


def test_plan_rule():
    from decentralizepy_amd import codec
    assert {n: codec.fft_chirp_fused_length(n) for n in TABLE} == TABLE
    assert [codec.fft_chirp_fused_length(n) for n in (2, 3, 7, 2 ** 30 + 2)] == [0] * 4
    for n in (8198, 16_396, 24_594):
        assert codec.fft_chirp_fused_length(n) == codec.fft_chirp_length(n)


def _jobs(dev, n):
    """Three forward jobs (one with an x0, one accumulating onto a non-zero row, one plain) and
    three inverse jobs, as device rows."""
    rng = np.random.default_rng(n)
    M = n // 2 + 1
    x, x0 = (torch.from_numpy(rng.standard_normal((3, n)).astype(np.float32)).to(dev)
             for _ in range(2))
    spec = torch.from_numpy((rng.standard_normal((2, 3, M)) + 1j * rng.standard_normal((2, 3, M)))
                            .astype(c64)).to(dev)
    return x, x0, spec[0], spec[1]


@pytest.mark.parametrize("n", [8198, 16_396])
def test_bit_for_bit_against_the_unfused_calls(dev, n):
    from decentralizepy_amd import codec
    x, x0, prior, coeffs = _jobs(dev, n)
    got = {}
    for fused in (False, True):
        out = prior.clone()
        tab = codec.FftNodesTable(list(x), [x0[0], None, None], list(out), [False, True, False],
                                  dev)
        assert codec.rfft_chirp_nodes(tab, n, fused=fused) == 0
        co, back = coeffs.clone(), torch.full((3, n), 7.0, device=dev)
        assert codec.irfft_chirp_nodes(codec.IfftNodesTable(list(co), list(back), dev), n,
                                       fused=fused) == 0
        assert torch.equal(co, coeffs)
        got[fused] = (out, back)
    assert torch.equal(torch.view_as_real(got[True][0]), torch.view_as_real(got[False][0]))
    assert torch.equal(got[True][1], got[False][1])
    assert not torch.equal(got[True][0][1], prior[1])


@pytest.mark.parametrize("n", [4, 6, 10, 66, 200, 1642, 89_834])
def test_accuracy_where_the_plan_differs(dev, n):
    """rfft, irfft and the round trip.  Measured on an MI355X (E / eps): see DESIGN.md 3.7."""
    from decentralizepy_amd import codec
    c = cops.random_case(n)
    P = codec.fft_chirp_fused_length(n)
    e_fwd = cops.emu_rfft(c["x"], P)
    emu = {"fwd": cops.rel(e_fwd, c["fwd"]),
           "inv": cops.rel(cops.emu_irfft(c["spec"], n, P), c["inv"]),
           "rt": cops.rel(cops.emu_irfft(e_fwd, n, P), c["x64"])}
    f = codec.rfft(torch.tensor(c["x"]).to(dev), chirp="fused")
    inv = codec.irfft(torch.tensor(c["spec"]).to(dev), n, chirp="fused")
    errs = {"fwd": cops.rel(f.cpu().numpy(), c["fwd"]),
            "inv": cops.rel(inv.cpu().numpy(), c["inv"]),
            "rt": cops.rel(codec.irfft(f, n, chirp="fused").cpu().numpy(), c["x64"])}
    print(n, P, {k: tuple(round(v / cops.EPS, 2) for v in (e, c["ref"][k], emu[k]))
                 for k, e in errs.items()})
    for what, e in errs.items():
        b = cops.bound(c["ref"][what], emu[what])
        assert e <= b, (what, n, e / cops.EPS, b / cops.EPS)


@pytest.mark.parametrize("n,npass", [(8198, 2), (1642, 2)])
def test_launch_counts(dev, n, npass):
    """2 npass + 1 launches forward, 2 npass inverse, for 1 job and for 5 (the library's timing
    counters, as test_gpu_fft_chirp's launch-count test reads them)."""
    from decentralizepy_amd import codec
    for jobs in (1, 5):
        x = torch.randn(jobs, n, device=dev)
        out = torch.zeros(jobs, n // 2 + 1, dtype=torch.complex64, device=dev)
        fwd = codec.FftNodesTable(list(x), None, list(out), False, dev)
        inv = codec.IfftNodesTable(list(out), list(x), dev)
        ws = codec.fft_chirp_nodes_workspace(jobs, n, dev, fused=True)
        for call, tab, want in ((codec.rfft_chirp_nodes, fwd, 2 * npass + 1),
                                (codec.irfft_chirp_nodes, inv, 2 * npass)):
            call(tab, n, ws, fused=True)
            with codec.KernelTimer() as t:
                call(tab, n, ws, fused=True)
            assert {k: cnt for k, (_, cnt) in t.result.items()} == {"fft": want}, (jobs, call)


@pytest.mark.parametrize("accumulation,aac", [(False, False), (True, False), (True, True)])
def test_engine_equals_the_unfused_engine(dev, accumulation, aac):
    from decentralizepy_amd.gossip_fft import FftRound
    meta, arr = cops.load_run()
    kw = dict(alpha=meta["alpha"], accumulation=accumulation, accumulate_averaging_changes=aac,
              device=dev)
    adj, x = ops.run_adjacency(meta), torch.from_numpy(arr["x0"]).to(dev)
    with pytest.raises(ValueError):
        FftRound(adj, x, chirp="yes", **kw)
    a, b = FftRound(adj, x, chirp="fused", **kw), FftRound(adj, x, chirp=True, **kw)
    assert a.batched and not a.native and a.N == 8198
    # at a size with a native plan the keyword changes nothing
    nat = [FftRound(adj, x[:, :1030].contiguous(), chirp=c, **kw) for c in ("fused", False)]
    for e in nat:
        assert e.native
        e.x += 0.01
        e.step()
    assert torch.equal(nat[0].x, nat[1].x) and torch.equal(nat[0].send, nat[1].send)
    for _ in range(3):
        for e in (a, b):
            e.x += 0.01 * torch.sin(e.x0 * 50.0)
            e.step()
        for name in ("x", "x0", "acc", "counter", "send"):
            if getattr(b, name) is not None:
                assert torch.equal(getattr(a, name), getattr(b, name)), name
