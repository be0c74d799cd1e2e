"""GPU: the batched generic-filter transforms (``dpz_dwt_generic_nodes`` /
``dpz_idwt_generic_nodes``) bit for bit against the numpy restatement pinned to pywt 1.1.1
(oracle/wavelet.py) and against the single-node ``codec.wavedec`` / ``codec.waverec``, at the
level rule's smallest length, at odd level lengths and around the tile edges; their refusals;
and ``JwinsWaveletBatchRound`` against ``JwinsRound`` on the HIP ops."""
import numpy as np
import pytest
import torch

from decentralizepy_amd.gossip_jwins_batch import wavelet_coeff_len
from oracle import topk as otopk
from oracle import wavelet as owav
from tests import jwins_round_ops as ops
from tests.test_gpu_jwins_batch_round import PAD, _bits, _padding_intact, _rows, run_named

pytestmark = pytest.mark.gpu

CASES = [(w, lv) for w in ("db1", "bior2.2", "db4", "db10", "dmey") for lv in (1, 3, 8)]
CASES += [("sym2", 5), ("sym2", 8)]  # sym2 to level 4 runs the fused kernels
FLEN = {"db1": 2, "sym2": 4, "bior2.2": 6, "db4": 8, "db10": 20, "dmey": 62}


def _sizes(T, level, F):
    """the level rule's smallest n, one whose levels read an odd length twice (once at level 1),
    and the tile edges"""
    def odd_inputs(n):
        lens = [n]
        for _ in range(level - 1):
            lens.append((lens[-1] + F - 1) // 2)
        return sum(v % 2 for v in lens)
    lo = next(n for n in range(1, 1 << 16) if wavelet_coeff_len(n, level, F))
    odd = next(n for n in range(max(lo, 301), 1 << 16) if odd_inputs(n) >= min(2, level))
    return [lo, odd, 2 * T - 1, 2 * T, 2 * T + 1, 6 * T + 37]


@pytest.mark.parametrize("wavelet,level", CASES)
def test_transforms_of_nodes_equal_the_oracle_and_the_single_calls(dev, wavelet, level):
    from decentralizepy_amd import codec
    F, T = FLEN[wavelet], codec.wavelet_nodes_tile_width()
    assert codec.filter_len(wavelet) == F and not codec._fused(wavelet, level)
    sizes = _sizes(T, level, F)
    assert sizes[0] < 2 * T and wavelet_coeff_len(sizes[0] - 1, level, F) is None
    for n in sizes:
        M = owav.coeff_len(n, level, wavelet)
        rng = np.random.default_rng([n, level, F])
        x = rng.standard_normal((3, n)).astype(np.float32)
        x0 = (x + 0.1 * rng.standard_normal((3, n))).astype(np.float32)
        acc = rng.standard_normal((3, M)).astype(np.float32)
        want_x = np.stack([owav.wavedec_array(x[j], level, wavelet) for j in range(3)])
        want_d = np.stack([owav.wavedec_array(x[j] - x0[j], level, wavelet) for j in range(3)])
        want_a = acc + want_d
        want_o = np.stack([owav.waverec_array(want_a[j], n, level, wavelet) for j in range(3)])
        tx, bx = _rows(dev, x, 4)
        t0, b0 = _rows(dev, x0, 4)
        for j in range(3):  # the single-node calls give the oracle's bits
            sx, sc = codec.wavedec(tx[j].contiguous(), level, x0=t0[j].contiguous(),
                                   wavelet=wavelet)
            so = codec.waverec(torch.from_numpy(want_a[j]).to(dev), n, level, wavelet=wavelet)
            for got, want in ((sx, want_x[j]), (sc, want_d[j]), (so, want_o[j])):
                assert np.array_equal(_bits(got), want.view(np.uint32)), (n, j)
        ws = codec.wavelet_nodes_workspace(3, n, level, wavelet, dev)
        for m in (3, 1):
            def fresh(data):
                return _rows(dev, data[:m], 4)

            def dwt(x0_, cx, cd, **kw):
                codec.dwt_generic_nodes(codec.DwtNodesTable(tx[:m], x0_, cx, cd, dev), n, level,
                                        wavelet, workspace=ws, **kw)

            blank = np.full((m, M), PAD, np.float32)
            (wx, bwx), (wc, bwc), (ox, box), (od, bod) = (fresh(blank) for _ in range(4))
            dwt(t0[:m], wx, wc)                                  # pair mode
            dwt(None, ox, None)                                  # W(x) alone
            dwt(t0[:m], None, od)                                # W(x - x0) alone
            ta, ba = fresh(acc)
            dwt(t0[:m], None, ta, accumulate=True)               # onto random accumulators
            out, bout = fresh(np.full((m, n), PAD, np.float32))  # the inverse of the accumulators
            codec.idwt_generic_nodes(codec.IdwtNodesTable(ta, out, dev), n, level, wavelet,
                                     workspace=ws)
            for got, want in ((wx, want_x), (wc, want_d), (ox, want_x), (od, want_d),
                              (ta, want_a), (out, want_o)):
                assert np.array_equal(_bits(got), want[:m].view(np.uint32)), (n, m)
            for back, ln in ((bx, n), (b0, n), (bwx, M), (bwc, M), (box, M), (bod, M), (ba, M),
                             (bout, n)):
                assert _padding_intact(back, ln, 4), (n, m)
        assert np.array_equal(_bits(tx), x.view(np.uint32))
        assert np.array_equal(_bits(t0), x0.view(np.uint32))


def test_generic_transforms_of_nodes_refuse_bad_calls_before_writing(dev):
    from decentralizepy_amd import _lib, codec
    n, level, w = 101, 3, "db4"
    M = codec.wavedec_len(n, level, w)
    x = np.random.default_rng(5).standard_normal((3, n)).astype(np.float32)
    blank = np.full((3, M), PAD, np.float32)
    short = codec.wavelet_nodes_workspace(3, n, level, w, dev)[:-4]

    def dwt(tab, n=n, **kw):
        return codec.dwt_generic_nodes(tab, n, level, w, check_rc=False, **kw)

    def idwt(tab, n=n, **kw):
        return codec.idwt_generic_nodes(tab, n, level, w, check_rc=False, **kw)

    outs = []
    for col in range(4):  # a row 4 bytes off in x, x0, coeffs_x, coeffs_diff
        cols = [_rows(dev, x if c < 2 else blank, 5 if c == col else 4) for c in range(4)]
        assert dwt(codec.DwtNodesTable(*(v for v, _ in cols), dev)) == _lib.DPZ_ERR_ARG
        outs += [back for _, back in cols[2:]]
    tx, t0 = _rows(dev, x, 4)[0], _rows(dev, x, 4)[0]
    (wx, bwx), (wc, bwc) = _rows(dev, blank, 4), _rows(dev, blank, 4)
    for word in (2, 3):  # mixed output sets: node 2 without coeffs_x, then without coeffs_diff
        tab = codec.DwtNodesTable(tx, t0, wx, wc, dev)
        tab.host[4 * 2 + word] = 0
        tab._upload(dev)
        assert dwt(tab) == _lib.DPZ_ERR_ARG
    tab = codec.DwtNodesTable(tx, t0, wx, wc, dev)
    assert dwt(tab, workspace=short) == _lib.DPZ_ERR_WORKSPACE
    assert dwt(tab, n=7) == _lib.DPZ_ERR_UNSUPPORTED  # 7 values, 8 taps
    assert dwt(tab, n=9) == _lib.DPZ_ERR_UNSUPPORTED  # level 3 reads 7 values: 9, then 8, then 7
    # the inverse: a misaligned coefficient row, a misaligned output row, then the same refusals
    for off_c, off_o in ((5, 4), (4, 5), (4, 4)):
        (co, _), (out, bout) = _rows(dev, blank, off_c), _rows(dev, x, off_o, pad=PAD)
        tab = codec.IdwtNodesTable(co, out, dev)
        if (off_c, off_o) == (4, 4):
            assert idwt(tab, workspace=short) == _lib.DPZ_ERR_WORKSPACE
            assert idwt(tab, n=7) == _lib.DPZ_ERR_UNSUPPORTED
        else:
            assert idwt(tab) == _lib.DPZ_ERR_ARG
        assert np.array_equal(_bits(out), x.view(np.uint32))
    torch.cuda.synchronize(dev)
    assert all((b == PAD).all() for b in outs + [bwx, bwc])  # nothing was written


# ---- the engine -----------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha_list", [ops.TUTORIAL_ALPHAS, [0.1, 0.25, 0.4]],
                         ids=["tutorial", "partial_only"])
@pytest.mark.parametrize("wavelet,level", [("db4", 4), ("coif2", 3)])
def test_engine_equals_jwins_round_on_the_hip_ops(dev, wavelet, level, alpha_list):
    """regular_16 at N = 4,100 over 3 rounds: bit for bit, on inputs whose selections do not tie
    at the k-th key (seeds 81 / 82: checked with the oracle round on the CPU)."""
    from decentralizepy_amd import codec
    from decentralizepy_amd.gossip_jwins import JwinsRound
    from decentralizepy_amd.gossip_jwins_batch import JwinsWaveletBatchRound
    adj = ops.run_adjacency(run_named("reg16")[0])
    n, nn = 4100, 16
    x = torch.from_numpy(np.random.default_rng(81).standard_normal((nn, n)).astype(np.float32))
    kw = dict(wavelet=wavelet, level=level, metadata_cap=0.5, device=dev)
    new = JwinsWaveletBatchRound(adj, x.to(dev), alpha_list, **kw)
    old = JwinsRound(adj, x.to(dev), str(alpha_list), **kw)
    assert new.M == old.M == owav.coeff_len(n, level, wavelet)
    for r in range(3):
        for u in range(nn):
            step = torch.from_numpy(ops.perturbation(82, r, u, n)).to(dev)
            new.x[u] += step
            old.x[u] += step
        keys = [(codec.wavedec(new.x[u].contiguous(), level, x0=new.x0[u].contiguous(),
                               wavelet=wavelet)[1] + new.acc[u]).cpu().numpy()
                for u in range(nn)]
        new.step()
        old.step()
        assert new.alphas == old.alphas
        lay, s_idx, s_val = old._layout(old.alphas)
        for u in range(nn):
            a = new.alphas[u]
            if a < 0.5:
                assert not otopk.kth_has_tie(otopk.keys_u32(keys[u]), round(a * new.M)), (r, u)
            (ni, nv), (oi, ov) = new.payload(u), old._payload(u, lay, s_idx, s_val)
            assert (ni is None) == (oi is None) == (a >= 0.5)
            assert ni is None or torch.equal(ni, oi), (r, u)
            assert torch.equal(nv.view(torch.int32), ov.view(torch.int32)), (r, u)
        for a, b in ((new.x, old.x), (new.x0, old.x0), (new.acc, old.acc)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), r
        assert torch.equal(new.counter, old.counter), r


def test_transform_launch_count_is_independent_of_the_node_count(dev):
    """db4 at level 4: the pair and the accumulating pass are 4 "dwt" launches each, the inverse
    4 "idwt" launches, for 6 nodes as for 16."""
    from decentralizepy_amd import codec
    from decentralizepy_amd.gossip_jwins_batch import JwinsWaveletBatchRound
    seen = []
    for name in ("irr6", "reg16"):
        meta, arr = run_named(name)
        eng = JwinsWaveletBatchRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]).to(dev),
                                     meta["alpha_list"], wavelet="db4", level=4, device=dev)
        eng.step()
        with codec.KernelTimer() as t:
            eng.step()
        seen.append({name: cnt for name, (_, cnt) in t.result.items()})
    for counts in seen:
        assert (counts.get("dwt"), counts.get("idwt")) == (8, 4)
