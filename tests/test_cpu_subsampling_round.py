"""CPU: the whole-topology SubSampling round (decentralizepy_amd/gossip_subsampling.py) — argument
validation of its three batched entry points without a device, and the engine's sharding, slots,
exchange and fold order with the numpy restatement (tests/subsampling_ops.py) standing in for the
HIP kernels, against a direct node-by-node simulation with ``OracleNode`` (one node per uid).  The
device path is covered by tests/test_gpu_subsampling_round.py, which shares the helpers here."""
import ctypes
import math

import numpy as np
import torch

from tests import subsampling_ops as sops
from tests.dist_harness import spawn_gloo

# 6 nodes, degrees 3 3 2 3 3 2: a ring with two chords
EDGES6 = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 3), (1, 4)]
# 5 nodes over 2 ranks: 3 + 2, the second rank's block of the all-gather is padded
EDGES5 = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (0, 2)]
SEEDS = [91, 2 ** 32 + 17, 5, 123456789, 77, 4242, 31337, 8]


def adjacency(n, edges):
    """Adjacency sets filled like ``gossip.read_edges`` fills them (same insertion order)."""
    adj = [set() for _ in range(n)]
    for a, b in edges:
        adj[a].add(b)
        adj[b].add(a)
    return adj


def star(n):
    return adjacency(n, [(0, j) for j in range(1, n)])


def models(n_nodes, n, seed=3):
    return torch.randn(n_nodes, n, generator=torch.Generator().manual_seed(seed))


def np_encode(x, seed, alpha, counter):
    c = counter.numpy() if counter is not None else None  # shares memory: updated in place
    return torch.from_numpy(sops.encode(x.numpy(), seed, alpha, c))


def np_fold(local, payloads, weights, w_self, out):
    pays = [(s, a, v.numpy()) for s, a, v in payloads]
    out.copy_(torch.from_numpy(sops.fold(local.numpy(), pays, weights, w_self)))


def oracle_rounds(adj, x, alpha, seeds, rounds, layerwise=False):
    """The reference written out node by node: per round (models, payload dicts, counters)."""
    nodes = [sops.OracleNode(x[i], seeds[i], alpha, layerwise) for i in range(len(adj))]
    for _ in range(rounds):
        data = [nd.get_data_to_send() for nd in nodes]
        for i, nd in enumerate(nodes):
            nd.averaging([dict(data[j], degree=len(adj[j])) for j in list(adj[i])])
        yield (np.stack([nd.model for nd in nodes]), data,
               np.stack([nd.counter for nd in nodes]))


def check_round(eng, want, lo=0, every_payload=True):
    """An engine's state after a step against the simulation's (models, data, counters)."""
    model, data, counter = want
    m = eng.hi - eng.lo
    np.testing.assert_array_equal(eng.x.cpu().numpy().view(np.uint32),
                                  model[lo:lo + m].view(np.uint32))
    np.testing.assert_array_equal(eng.counter.cpu().numpy(), counter[lo:lo + m])
    for q in (range(len(data)) if every_payload else range(lo, lo + m)):
        seed, alpha, vals = eng.payload(q)
        assert seed == data[q]["seed"] and alpha == data[q]["alpha"]
        assert vals.numel() == len(data[q]["params"])
        np.testing.assert_array_equal(vals.cpu().numpy().view(np.uint32),
                                      data[q]["params"].view(np.uint32))


def test_argument_validation_without_gpu():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    ARG, WS, UNSUP = _lib.DPZ_ERR_ARG, _lib.DPZ_ERR_WORKSPACE, _lib.DPZ_ERR_UNSUPPORTED
    d = 4096  # never dereferenced: the checks come first
    seeds, alphas = (ctypes.c_uint32 * 2)(1, 2), (ctypes.c_float * 2)(0.1, 0.2)
    n = 100
    mw, re = 4, L.dpz_mt_rank_entries(n)
    big = 1 << 31

    def mask(m=2, s=seeds, a=alphas, n=n, mk=d, ms=mw, rt=d, rs=re, cnt=d, ws=d, wsb=1 << 20):
        return L.dpz_mt_mask_batch(m, s, a, n, mk, ms, rt, rs, cnt, ws, wsb, None)

    assert L.dpz_mt_mask_batch_workspace_bytes(2, n) >= 256
    assert L.dpz_mt_mask_batch_workspace_bytes(0, n) == 0
    assert (L.dpz_mt_mask_batch_workspace_bytes(3, (1 << 24) + 65)
            >= 3 * (L.dpz_mt_mask_workspace_bytes((1 << 24) + 65) - 256))
    for bad in (dict(m=0), dict(n=0), dict(s=None), dict(a=None), dict(mk=None), dict(rt=None),
                dict(cnt=None), dict(ws=None), dict(ms=mw - 1), dict(ms=mw + 2), dict(rs=re - 1)):
        assert mask(**bad) == ARG, bad
    assert mask(n=big, ms=big // 32, rs=big) == UNSUP
    assert mask(wsb=0) == WS
    n2 = (1 << 24) + 65  # needs coarse states: the single mask's workspace is too small for two
    assert mask(n=n2, ms=-(-n2 // 128) * 4, rs=L.dpz_mt_rank_entries(n2),
                wsb=L.dpz_mt_mask_workspace_bytes(n2)) == WS

    assert L.dpz_mask_gather_nodes(0, d, n, 8, None) == ARG
    assert L.dpz_mask_gather_nodes(1, d, 0, 8, None) == ARG
    assert L.dpz_mask_gather_nodes(1, None, n, 8, None) == ARG
    assert L.dpz_mask_gather_nodes(1, d, n, 0, None) == ARG
    assert L.dpz_mask_gather_nodes(1, d, big, 8, None) == UNSUP

    np2 = (ctypes.c_int * 2)(3, 16)
    assert L.dpz_mask_decode_average_nodes(0, d, np2, n, 1, None, 0, None) == ARG
    assert L.dpz_mask_decode_average_nodes(2, d, np2, 0, 1, None, 0, None) == ARG
    assert L.dpz_mask_decode_average_nodes(2, None, np2, n, 1, None, 0, None) == ARG
    assert L.dpz_mask_decode_average_nodes(2, d, None, n, 1, None, 0, None) == ARG
    assert L.dpz_mask_decode_average_nodes(2, d, np2, n, 0x10, None, 0, None) == ARG  # ACCUMULATE
    assert L.dpz_mask_decode_average_nodes(2, d, np2, n, 1, None, 3, None) == ARG  # words, no guard
    assert L.dpz_mask_decode_average_nodes(2, d, (ctypes.c_int * 2)(3, 0), n, 1, None, 0,
                                           None) == ARG
    assert L.dpz_mask_decode_average_nodes(2, d, np2, big, 1, None, 0, None) == UNSUP
    assert L.dpz_mask_decode_average_nodes(2, d, (ctypes.c_int * 2)(3, 17), n, 1, None, 0,
                                           None) == UNSUP
    assert L.dpz_abi_version() == 2  # symbols were added, nothing changed


def test_engine_rejects_what_it_does_not_implement():
    import pytest

    from decentralizepy_amd.gossip_subsampling import SubSamplingRound
    adj = adjacency(6, EDGES6)
    x = models(6, 50)
    kw = dict(encode=np_encode, fold=np_fold)
    for bad in (dict(exchange="peer"), dict(exchange="reduce_scatter"), dict(metadata_cap=0.5),
                dict(compress=True)):
        with pytest.raises(ValueError):
            SubSamplingRound(adj, x, 0.1, SEEDS[:6], **kw, **bad)
    with pytest.raises(ValueError):
        SubSamplingRound(adj, x, 0.1, SEEDS[:5], **kw)


def test_single_rank_round_matches_oracle_nodes():
    from decentralizepy_amd.gossip_subsampling import SubSamplingRound
    adj = adjacency(6, EDGES6)
    assert sorted(len(a) for a in adj) == [2, 2, 3, 3, 3, 3]
    n, alpha = 3001, 0.1
    x = models(6, n)
    eng = SubSamplingRound(adj, x, alpha, SEEDS[:6], encode=np_encode, fold=np_fold)
    assert eng.round == 0 and not eng.coll
    for r, want in enumerate(oracle_rounds(adj, x.numpy(), alpha, SEEDS[:6], 3)):
        eng.step()
        assert eng.round == r + 1
        check_round(eng, want)
    assert eng.counter.max() >= 1


def test_layerwise_leaves_the_counters_zero():
    from decentralizepy_amd.gossip_subsampling import SubSamplingRound
    adj = adjacency(6, EDGES6)
    x = models(6, 997)
    eng = SubSamplingRound(adj, x, 0.2, SEEDS[:6], layerwise=True, encode=np_encode,
                           fold=np_fold)
    for want in oracle_rounds(adj, x.numpy(), 0.2, SEEDS[:6], 2, layerwise=True):
        eng.step()
        check_round(eng, want)
    assert not eng.counter.any()


def test_small_slot_raises_and_keeps_the_models():
    import pytest

    from decentralizepy_amd.gossip_subsampling import SubSamplingRound
    adj = adjacency(6, EDGES6)
    x = models(6, 3001)
    eng = SubSamplingRound(adj, x, 0.1, SEEDS[:6], slot_cap=200, encode=np_encode, fold=np_fold)
    assert eng.cap == 200
    with pytest.raises(RuntimeError, match="slot"):
        eng.step()
    assert eng.round == 0
    np.testing.assert_array_equal(eng.x.numpy().view(np.uint32), x.numpy().view(np.uint32))


def _worker(rank, world, n, alpha):
    from decentralizepy_amd.gossip import shard
    from decentralizepy_amd.gossip_subsampling import SubSamplingRound
    adj = adjacency(5, EDGES5)
    x = models(5, n)
    lo, hi, _ = shard(5, world, rank)
    eng = SubSamplingRound(adj, x[lo:hi], alpha, SEEDS[:5], rank=rank, world=world,
                           encode=np_encode, fold=np_fold)
    res = []
    for _ in range(3):
        eng.step()
        res.append((eng.x.numpy().copy(), eng.counter.numpy().copy(),
                    [eng.payload(p)[2].numpy().copy() for p in range(5)]))
    return lo, res


def test_two_rank_round_equals_single_rank():
    from decentralizepy_amd.gossip import shard
    from decentralizepy_amd.gossip_subsampling import SubSamplingRound
    n, alpha = 2003, 0.1
    adj = adjacency(5, EDGES5)
    assert shard(5, 2, 1) == (3, 5, 3)  # 3 + 2 nodes: the all-gather is padded
    x = models(5, n)
    single = SubSamplingRound(adj, x, alpha, SEEDS[:5], encode=np_encode, fold=np_fold)
    want = []
    for ref in oracle_rounds(adj, x.numpy(), alpha, SEEDS[:5], 3):
        single.step()
        check_round(single, ref)
        want.append((single.x.numpy().copy(), single.counter.numpy().copy(),
                     [single.payload(p)[2].numpy().copy() for p in range(5)]))
    for lo, res in spawn_gloo(_worker, 2, n, alpha):
        for (xs, cs, pays), (wx, wc, wpays) in zip(res, want):
            m = xs.shape[0]
            np.testing.assert_array_equal(xs.view(np.uint32), wx[lo:lo + m].view(np.uint32))
            np.testing.assert_array_equal(cs, wc[lo:lo + m])
            for a, b in zip(pays, wpays):  # every node's payload crossed the all-gather
                np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_slot_cap():
    from decentralizepy_amd.gossip_subsampling import SubSamplingRound, slot_capacity
    n = 131_109
    for alpha in (0.01, 0.1, 0.5, 1.0):
        raw = min(n, math.ceil(alpha * n + 8 * math.sqrt(alpha * n * (1 - alpha))))
        cap = slot_capacity(n, alpha)
        assert cap % 4 == 0 and raw <= cap < raw + 4
    assert slot_capacity(n, 0.1) == 13_980 and slot_capacity(n, 1.0) == 131_112
    cap = slot_capacity(n, 0.1)
    counts = [int(sops.mask(seed, 0.1, n).sum()) for seed in range(1, 9)]
    assert max(counts) <= cap and min(counts) > 0.09 * n
    adj = adjacency(6, EDGES6)
    x = models(6, 64)
    eng = SubSamplingRound(adj, x, 0.1, SEEDS[:6], encode=np_encode, fold=np_fold)
    assert eng.cap == slot_capacity(64, 0.1)
    assert SubSamplingRound(adj, x, 0.1, SEEDS[:6], slot_cap=9, encode=np_encode,
                            fold=np_fold).cap == 12
