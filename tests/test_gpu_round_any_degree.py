"""GPU: the whole-topology engines on topologies with more than four neighbours per node and on
rounds with full shares.  Their folds take dpz_decode_average_batch's any-degree one-launch path
(dpz_fold_walk.hip fold_walk_any_kernel): every engine bit for bit against what it is compared
with on small degrees (the restatement written out node by node, ``JwinsRound`` on the HIP ops,
the per-node plugin objects), and the ``fold`` launches of a step against
dpz_debug_fold_batch_plan: a launch per table of nodes, not per node.

The 7-node star folds in one launch.  fullyConnected_16 takes the plan's two: its 16 nodes and
240 payload entries are 256 slots of 24 bytes, and a launch's kernel arguments hold 146."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import jwins_round_ops as jops
from tests import scenario
from tests import topkacc_round_ops as tops
from tests.test_cpu_gossip import _oracle_encode, _oracle_fold

pytestmark = pytest.mark.gpu

FC16 = os.path.join(scenario.GOLDEN, "fullyConnected_16.edges")
REG16 = os.path.join(scenario.GOLDEN, "regular_16.edges")
SMALLWORLD = os.path.join(scenario.GOLDEN, "96_nodes_smallworld.edges")
STAR = [set(range(1, 7))] + [{0} for _ in range(6)]


def _adj(name):
    from decentralizepy_amd.gossip import read_edges
    return STAR if name == "star" else read_edges(FC16)


def _plan(adj, n, k_of, dense_of, flags):
    """The plan of a round's fold: node u folds one payload per neighbour v, of k_of(v) entries."""
    from decentralizepy_amd import _lib
    counts = [len(a) for a in adj]
    ks = [k_of(v) for a in adj for v in a]
    dn = [1 if dense_of(v) else 0 for a in adj for v in a]
    out = (ctypes.c_int * 4)()
    assert _lib.lib().dpz_debug_fold_batch_plan(
        len(adj), n, (ctypes.c_int * len(adj))(*counts), (ctypes.c_int64 * len(ks))(*ks),
        (ctypes.c_int * len(dn))(*dn), flags, 1, out) == 0
    return dict(zip(("path", "launches", "first", "passes"), out))


def _folds(t):
    assert "fold_offsets" not in t.result
    return t.result["fold"][1]


@pytest.mark.parametrize("avg", [False, True], ids=["acc", "avg"])
@pytest.mark.parametrize("topo", ["star", "fc16"])
def test_topkacc_round(dev, topo, avg):
    """Payloads, models, x0, accumulators and counters equal the restatement's; a step's folds
    are the plan's launches (before: one per node at least)."""
    from decentralizepy_amd import _lib, codec
    from decentralizepy_amd.gossip_topkacc import TopKAccRound
    adj = _adj(topo)
    nn, n, alpha = len(adj), 2051, 0.05
    x = np.random.default_rng(70).standard_normal((nn, n)).astype(np.float32)
    eng = TopKAccRound(adj, torch.from_numpy(x).to(dev), alpha, accumulate_averaging_changes=avg)
    pl = _plan(adj, n, lambda v: eng.k, lambda v: False,
               _lib.DPZ_FOLD_SELF | _lib.DPZ_FOLD_ALSO_LOCAL)
    assert (pl["path"], pl["launches"]) == (2, 1 if topo == "star" else 2)
    hx, h0 = x.copy(), x.copy()
    hacc, hcnt = np.zeros_like(x), np.zeros(x.shape, np.int32)
    for r in range(3):
        for u in range(nn):
            hx[u] = (hx[u] + tops.perturbation(71, r, u, n)).astype(np.float32)
        eng.x.copy_(torch.from_numpy(hx).to(dev))
        pays = tops.round_all(adj, hx, h0, hacc, hcnt, eng.k, avg)
        with codec.KernelTimer() as t:
            eng.step()
        assert _folds(t) == pl["launches"] < nn
        for u, (idx, vals) in enumerate(pays):
            gi, gv = eng.payload(u)
            np.testing.assert_array_equal(gi.cpu().numpy(), idx)
            np.testing.assert_array_equal(tops.u32(gv.cpu().numpy()), tops.u32(vals))
        np.testing.assert_array_equal(tops.u32(eng.x.cpu().numpy()), tops.u32(hx))
        np.testing.assert_array_equal(tops.u32(eng.x0.cpu().numpy()), tops.u32(hx))
        np.testing.assert_array_equal(tops.u32(eng.acc.cpu().numpy()), tops.u32(hacc))
        np.testing.assert_array_equal(eng.counter.cpu().numpy(), hcnt)


@pytest.mark.parametrize("topo", ["star", "fc16"])
def test_gossip_round(dev, topo, monkeypatch):
    """GossipRound against the same engine on the oracle's encode and fold; its guarded fold
    applies (no host check between encode and fold) and is the plan's launches."""
    from decentralizepy_amd import _lib, codec
    from decentralizepy_amd.gossip import GossipRound
    adj = _adj(topo)
    nn, n, alpha = len(adj), 2051, 0.05
    x = torch.from_numpy(np.random.default_rng(72).standard_normal((nn, n)).astype(np.float32))
    ref = GossipRound(adj, x, alpha, encode=_oracle_encode, fold=_oracle_fold)
    eng = GossipRound(adj, x.to(dev), alpha)
    assert all(eng.x[j].data_ptr() % 16 == 0 and eng.out[j].data_ptr() % 16 == 0 for j in range(nn))
    pl = _plan(adj, n, lambda v: eng.k, lambda v: False,
               _lib.DPZ_FOLD_SELF | _lib.DPZ_FOLD_ALSO_LOCAL)
    assert (pl["path"], pl["launches"]) == (2, 1 if topo == "star" else 2)
    guarded = []
    fold_all = eng.fold_all

    def spy(guard=None):
        res = fold_all(guard=guard)
        if guard is not None:
            guarded.append(res)
        return res

    monkeypatch.setattr(eng, "fold_all", spy)
    for r in range(2):
        step = 0.01 * torch.randn(nn, n, generator=torch.Generator().manual_seed(100 + r))
        ref.x += step
        eng.x += step.to(dev)
        ref.step()
        with codec.KernelTimer() as t:
            eng.step()
        torch.cuda.synchronize()
        assert _folds(t) == pl["launches"] < nn
        for a, b in ((eng.x, ref.x), (eng.x0, ref.x0)):
            np.testing.assert_array_equal(a.cpu().numpy().view(np.uint32),
                                          b.numpy().view(np.uint32))
        np.testing.assert_array_equal(eng.counter.cpu().numpy(), ref.counter.numpy())
    assert guarded == [True, True]


def _jwins_pair(dev, adj, n, rounds, seed):
    """JwinsBatchRound against JwinsRound on the HIP ops over ``rounds`` rounds with the
    tutorial's alpha list: payloads, models, accumulators and counters bit for bit.  Returns per
    round (fold launches of the step, the plan of its fold)."""
    from decentralizepy_amd import _lib, codec
    from decentralizepy_amd.gossip_jwins import JwinsRound
    from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound
    nn = len(adj)
    x = torch.from_numpy(np.random.default_rng(seed).standard_normal((nn, n)).astype(np.float32))
    new = JwinsBatchRound(adj, x.to(dev), jops.TUTORIAL_ALPHAS, device=dev)
    old = JwinsRound(adj, x.to(dev), str(jops.TUTORIAL_ALPHAS), metadata_cap=0.5, device=dev)
    assert new.M == old.M == codec.wavedec_len(n, 4) >= 1024
    seen = []
    for r in range(rounds):
        for u in range(nn):
            step = torch.from_numpy(jops.perturbation(seed + 1, r, u, n)).to(dev)
            new.x[u] += step
            old.x[u] += step
        with codec.KernelTimer() as t:
            new.step()
        old.step()
        assert new.alphas == old.alphas
        lay, s_idx, s_val = old._layout(old.alphas)
        ks = []
        for u in range(nn):
            (ni, nv), (oi, ov) = new.payload(u), old._payload(u, lay, s_idx, s_val)
            assert (ni is None) == (oi is None) == (new.alphas[u] >= 0.5)
            assert ni is None or torch.equal(ni, oi), (r, u)
            assert torch.equal(nv.view(torch.int32), ov.view(torch.int32)), (r, u)
            ks.append(nv.numel())
        for a, b in ((new.x, old.x), (new.x0, old.x0), (new.acc, old.acc)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), r
        assert torch.equal(new.counter, old.counter), r
        pl = _plan(adj, new.M, lambda v: ks[v], lambda v: new.alphas[v] >= 0.5, _lib.DPZ_FOLD_SELF)
        seen.append((_folds(t), pl, sum(a >= 0.5 for a in new.alphas)))
    return seen


def test_jwins_batch_round_with_full_shares(dev):
    """regular_16 at N = 4,100: every round holds full shares, which the fold took node after
    node (16 launches and more); now the plan's one."""
    from decentralizepy_amd.gossip import read_edges
    seen = _jwins_pair(dev, read_edges(REG16), 4100, 4, seed=81)
    assert sum(full > 0 for _, _, full in seen) >= 3
    for folds, pl, full in seen:
        assert pl["path"] == (2 if full else 1) and pl["launches"] == 1
        assert folds <= pl["launches"]


@pytest.mark.parametrize("nn", [32, 96])
def test_jwins_batch_round_on_the_smallworld_graph(dev, nn):
    """Degrees 3..10 and full shares, the first 32 nodes' induced subgraph and all 96: three times
    the nodes, the launches of three times the tables."""
    from decentralizepy_amd.gossip import read_edges
    adj = [{v for v in a if v < nn} for a in read_edges(SMALLWORLD)[:nn]]
    assert min(len(a) for a in adj) >= 1 and max(len(a) for a in adj) > 4
    for folds, pl, _ in _jwins_pair(dev, adj, 1030, 2, seed=83 + nn):
        assert pl["path"] == 2 and pl["passes"] == 1
        assert folds == pl["launches"] < nn / 4


def test_fft_round_fully_connected(dev, tmp_path):
    """fullyConnected_16 at N = 1,030 against the per-node plugin objects; the fold over the
    float view (n = 1,032) takes the any-degree path."""
    from decentralizepy_amd import _lib, codec
    from decentralizepy_amd.gossip import read_edges
    from decentralizepy_amd.gossip_fft import FftRound
    from tests import fft_round_ops as fops
    from tests.test_gpu_fft_round import _engine_rounds, _plugin_rounds
    adj = read_edges(FC16)
    shape, kwargs = (30, 33, 40), dict(accumulation=True, accumulate_averaging_changes=True)
    x0 = np.random.default_rng(70).standard_normal((16, 1030)).astype(np.float32)
    eng = FftRound(adj, torch.from_numpy(x0).to(dev), 0.1, device=dev, **kwargs)
    pl = _plan(adj, 2 * eng.M, lambda v: 2 * eng.k, lambda v: False, _lib.DPZ_FOLD_SELF)
    assert (pl["path"], pl["launches"]) == (2, 2)
    with codec.KernelTimer() as t:
        got = _engine_rounds(eng, 2, seed=92)
    assert _folds(t) == 2 * pl["launches"]
    fops.same_bits(got, _plugin_rounds(adj, x0, shape, 2, 92, dict(alpha=0.1, **kwargs), tmp_path))
