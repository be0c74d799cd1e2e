"""GPU: the whole-topology SubSampling round.  The batched kernels against the single-payload
entry points they batch (codec.mt_mask / boolean indexing / codec.mask_decode_average), bit for
bit, and the engine (decentralizepy_amd/gossip_subsampling.py) against the node-by-node
``OracleNode`` simulation of tests/test_cpu_subsampling_round.py.  Sizes: one element, one state
block, the chunk edges (65536 elements a chunk), several chunks with a ragged tail, and one past
256 chunks (the coarse launch)."""
import numpy as np
import pytest
import torch

from tests import subsampling_ops as ops
from tests.dist_harness import rccl_loopback
from tests.test_cpu_subsampling_round import (EDGES6, SEEDS, adjacency, check_round, models,
                                              oracle_rounds, star)

pytestmark = pytest.mark.gpu

S = 65536
# a negative alpha selects nothing, 1.0 everything; the rest differ from mask to mask
ALPHAS = [0.1, -0.25, 1.0, 0.5, 1e-8, 0.3, 0.02, 0.75, 0.9, 0.05, 0.25, 0.6, 0.01]
MASK_SEEDS = [7, 2 ** 32 + 5, 0xFFFFFFFF, 0, 12345, 99, 2 ** 63 + 3, 31, 32, 33, 34, 35, 36]
FILL = 0x5A5A5A5A


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _check_batch(dev, n, m, off=0):
    from decentralizepy_amd import codec
    seeds = [MASK_SEEDS[(i + off) % 13] for i in range(m)]
    alphas = [ALPHAS[(i + off) % 13] for i in range(m)]
    mw, re = codec.mask_words(n), codec.mt_rank_entries(n)
    # rows wider than needed, prefilled: the padding must come back untouched
    mask = torch.full((m, -(-mw // 4) * 4 + 4), FILL, dtype=torch.int32, device=dev)
    rank = torch.full((m, re + 3), FILL, dtype=torch.int32, device=dev)
    count = torch.full((m,), -1, dtype=torch.int64, device=dev)
    got = codec.mt_mask_batch(seeds, alphas, n, dev, mask=mask, rank_tab=rank, count=count)
    assert got[0] is mask and got[1] is rank and got[2] is count
    ws = codec.Workspace(dev)
    for i in range(m):
        m1, r1, c1 = codec.mt_mask(seeds[i], alphas[i], n, dev, workspace=ws)
        err = str((n, m, i, seeds[i], alphas[i]))
        assert int(count[i].item()) == int(c1.item()), err
        np.testing.assert_array_equal(_u32(mask[i, :mw]), _u32(m1), err_msg=err)
        np.testing.assert_array_equal(_u32(rank[i, :re]), _u32(r1), err_msg=err)
    assert (_u32(mask[:, mw:]) == FILL).all() and (_u32(rank[:, re:]) == FILL).all()
    return seeds, alphas, mask, count


@pytest.mark.parametrize("m", [1, 5, 13])
@pytest.mark.parametrize("n", [1, 33, S - 1, S + 1, 3 * S + 37])
def test_mask_batch_equals_single_masks(dev, n, m):
    seeds, alphas, _, count = _check_batch(dev, n, m, off=n % 5 if m == 1 else 0)
    if m > 1:
        assert min(alphas) < 0 and max(alphas) == 1.0 and max(seeds) >= 2 ** 32
        c = count.cpu().numpy()
        assert c[alphas.index(min(alphas))] == 0 and c[alphas.index(1.0)] == n


def test_mask_batch_of_more_than_one_launch_group(dev):
    """Seeds and alphas travel by value, 64 masks per launch: 70 masks take a second group."""
    _check_batch(dev, S + 1, 70)


def test_mask_batch_coarse_launch(dev):
    from decentralizepy_amd import _lib
    n = 2 ** 24 + 65
    assert -(-n // S) > _lib.lib().dpz_mt_coarse_chunks() > 0
    _check_batch(dev, n, 3)


def test_mask_batch_against_the_restatement(dev):
    from decentralizepy_amd import codec
    n = S + 1
    seeds, alphas = [2 ** 32 + 5, 77], [0.1, 0.5]
    mask, _, count = codec.mt_mask_batch(seeds, alphas, n, dev)
    for i in range(2):
        ref = ops.mask(seeds[i], alphas[i], n)
        assert int(count[i].item()) == int(ref.sum())
        np.testing.assert_array_equal(_u32(mask[i, :codec.mask_words(n)]), ops.pack(ref))


@pytest.mark.parametrize("n", [3 * S + 37, S])
def test_gather_nodes_matches_boolean_index(dev, n):
    from decentralizepy_amd import codec
    m, alphas, seeds = 3, [0.1, 0.5, 0.02], [11, 12, 2 ** 32 + 13]
    x = np.stack([ops.recipe(100 + j, n) for j in range(m)])
    tx = torch.from_numpy(x).to(dev)  # packed rows: with n % 4 == 1 rows 1 and 2 are unaligned
    assert n % 4 == 0 or tx[1].data_ptr() % 16
    mask, rank, count = codec.mt_mask_batch(seeds, alphas, n, dev)
    sel = [ops.mask(seeds[j], alphas[j], n) for j in range(m)]
    ks = [int(s.sum()) for s in sel]
    assert count.cpu().tolist() == ks
    counter = torch.zeros(m, n, dtype=torch.int32, device=dev)
    want = np.zeros((m, n), np.int32)
    for cap, with_counter in ((max(ks), True), (max(ks) + 5, False), (ks[0] + 3, True)):
        # the last cap holds nodes 0 and 2 but not node 1 (alpha 0.5)
        assert ks[2] <= ks[0] < cap <= max(ks) + 5
        vals = torch.full((m, cap + 1), 7.0, dtype=torch.float32, device=dev)
        status = torch.full((m,), 9, dtype=torch.int32, device=dev)
        tab = codec.gather_node_table(tx, mask, rank, vals, count, status,
                                      counter if with_counter else None)
        codec.mask_gather_nodes(tab, n, cap)
        got = vals.cpu().numpy()
        assert status.cpu().tolist() == [int(k > cap) for k in ks]
        for j in range(m):
            k = min(ks[j], cap)
            np.testing.assert_array_equal(got[j, :k].view(np.uint32),
                                          x[j][sel[j]][:k].view(np.uint32))
            assert (got[j, k:] == 7.0).all()  # the rest of the slot and the guard element
            if with_counter:
                want[j] += sel[j]
        np.testing.assert_array_equal(counter.cpu().numpy(), want)
    assert status.cpu().tolist() == [0, 1, 0] and want.max() == 2


@pytest.fixture(scope="module")
def fold_case(dev):
    """17 payloads at n = 2 * 65536 + 37 (their masks from one batch), three packed local rows."""
    from decentralizepy_amd import codec
    n = 2 * S + 37
    rng = np.random.default_rng(21)
    alphas = [[0.1, 0.5, 1e-8, 1.0][p % 4] for p in range(17)]
    mask, rank, count = codec.mt_mask_batch(list(range(500, 517)), alphas, n, dev)
    pays = []
    for p, k in enumerate(count.cpu().tolist()):
        v = rng.standard_normal(k).astype(np.float32)
        v[::5] = -0.0
        pays.append((mask[p], rank[p], torch.from_numpy(v).to(dev)))
    local = torch.from_numpy(rng.standard_normal((3, n)).astype(np.float32)).to(dev)
    w = [float(v) for v in rng.uniform(0.01, 0.06, 17)]
    return n, pays, local, w


def _dests(fold_case, out, self_term):
    n, pays, local, w = fold_case
    picks = [[4], [0, 1, 2], list(range(16))]  # 1, 3 and 16 payloads in one call
    return [(local[d], out[d], 1 - sum(w[p] for p in pk) if self_term else None,
             [pays[p] + (w[p],) for p in pk]) for d, pk in enumerate(picks)]


@pytest.mark.parametrize("self_term", [True, False])
def test_decode_average_nodes_equals_single_folds(dev, fold_case, self_term):
    from decentralizepy_amd import codec
    n, pays, local, w = fold_case
    out = torch.full((3, n), 7.0, dtype=torch.float32, device=dev)
    dests = _dests(fold_case, out, self_term)
    tab, counts = codec.fold_node_table(dests, dev)
    assert list(counts) == [1, 3, 16]
    guard = torch.zeros(5, dtype=torch.int32, device=dev)
    guard[3] = 2
    assert codec.mask_decode_average_nodes(tab, counts, n, self_term, guard=guard)
    assert (out == 7.0).all()  # a nonzero guard word: nothing written
    guard.zero_()
    assert codec.mask_decode_average_nodes(tab, counts, n, self_term, guard=guard)
    for d, (loc, _, w_self, ps) in enumerate(dests):
        ref = codec.mask_decode_average(loc, [p[:3] for p in ps], [p[3] for p in ps], w_self)
        np.testing.assert_array_equal(_u32(out[d]), _u32(ref), err_msg=str(d))
    out2 = torch.empty_like(out)  # and without a guard
    tab2, _ = codec.fold_node_table(_dests(fold_case, out2, self_term), dev)
    assert codec.mask_decode_average_nodes(tab2, counts, n, self_term)
    np.testing.assert_array_equal(_u32(out2), _u32(out))


def test_decode_average_nodes_refuses_17_payloads(dev, fold_case):
    from decentralizepy_amd import _lib, codec
    n, pays, local, w = fold_case
    out = torch.full((2, n), 7.0, dtype=torch.float32, device=dev)
    dests = [(local[0], out[0], 0.5, [pays[0] + (w[0],)]),
             (local[1], out[1], 0.2, [pays[p] + (w[p],) for p in range(17)])]
    tab, counts = codec.fold_node_table(dests, dev)
    assert list(counts) == [1, 17]
    rc = _lib.lib().dpz_mask_decode_average_nodes(2, tab.data_ptr(), counts, n, 1, None, 0, None)
    assert rc == _lib.DPZ_ERR_UNSUPPORTED
    assert codec.mask_decode_average_nodes(tab, counts, n) is False
    torch.cuda.synchronize()
    assert (out == 7.0).all()  # nothing was enqueued


# ---- the engine -------------------------------------------------------------------------------
N6, ALPHA = 131_109, 0.1


@pytest.fixture(scope="module")
def six_nodes():
    adj = adjacency(6, EDGES6)
    x = models(6, N6)
    return adj, x, list(oracle_rounds(adj, x.numpy(), ALPHA, SEEDS[:6], 3))


def test_engine_matches_oracle_nodes(dev, six_nodes):
    from decentralizepy_amd.gossip_subsampling import SubSamplingRound
    adj, x, want = six_nodes
    eng = SubSamplingRound(adj, x.to(dev), ALPHA, SEEDS[:6])
    assert eng.x.data_ptr() % 16 == 0 and eng.x[1].data_ptr() % 16  # packed rows, N % 4 == 1
    for r, ref in enumerate(want):
        eng.step()
        assert eng.round == r + 1
        check_round(eng, ref)


def test_engine_star_takes_the_chained_fold(dev):
    from decentralizepy_amd.gossip_subsampling import SubSamplingRound
    adj = star(18)
    n = 65_541
    x = models(18, n, seed=4)
    seeds = [1000 + 3 * i for i in range(18)]
    eng = SubSamplingRound(adj, x.to(dev), ALPHA, seeds)
    for ref in oracle_rounds(adj, x.numpy(), ALPHA, seeds, 2):
        eng.step()
        check_round(eng, ref)
    (tab, far, _), = [v for k, v in eng._tabs.items() if k[0] == "fold"][:1]
    assert far == [0] and len(tab[1]) == 17  # the centre's 17 payloads, the leaves batched


def test_engine_layerwise_leaves_the_counters_zero(dev):
    from decentralizepy_amd.gossip_subsampling import SubSamplingRound
    adj = adjacency(6, EDGES6)
    n = S + 5
    x = models(6, n, seed=6)
    eng = SubSamplingRound(adj, x.to(dev), ALPHA, SEEDS[:6], layerwise=True)
    for ref in oracle_rounds(adj, x.numpy(), ALPHA, SEEDS[:6], 2, layerwise=True):
        eng.step()
        check_round(eng, ref)
    assert not eng.counter.any()


def test_engine_small_slot_raises_and_keeps_the_models(dev, six_nodes):
    from decentralizepy_amd.gossip_subsampling import SubSamplingRound
    adj, x, _ = six_nodes
    eng = SubSamplingRound(adj, x.to(dev), ALPHA, SEEDS[:6], slot_cap=1000)
    with pytest.raises(RuntimeError, match="slot"):
        eng.step()
    torch.cuda.synchronize()
    assert eng.round == 0
    np.testing.assert_array_equal(_u32(eng.x), x.numpy().view(np.uint32))


@pytest.fixture
def rccl_group(dev):
    with rccl_loopback(dev) as group:
        yield group


def test_engine_through_rccl_equals_in_place(dev, six_nodes, rccl_group):
    from decentralizepy_amd.gossip_subsampling import SubSamplingRound
    adj, x, want = six_nodes
    eng = SubSamplingRound(adj, x.to(dev), ALPHA, SEEDS[:6], rank=0, world=1, group=rccl_group)
    assert eng.coll and eng.recv is not None
    for ref in want:
        eng.step()
        check_round(eng, ref)
