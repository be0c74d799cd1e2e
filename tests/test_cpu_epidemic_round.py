"""CPU: the whole-topology full-model rounds (decentralizepy_amd/gossip_epidemic.py) — the
EL-Local sampler, the sharding, the exchange and the fold order with the numpy restatement
(tests/epidemic_ops.py) standing in for the HIP kernel, against the runs recorded from the
unmodified reference (tests/golden/epidemic.json, make_golden_epidemic.py); and the argument
checks of ``dpz_dense_average_nodes``, which are all made before a device is touched.  The device
path is covered by tests/test_gpu_epidemic_round.py, which shares the helpers here."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import epidemic_ops as ops
from tests.dist_harness import spawn_gloo

EL_RUNS = ["el_d7", "el_d1", "el_d15"]


def np_fold(local, rows, weights, w_self, out):
    out.copy_(torch.from_numpy(ops.fold(local.numpy(), [r.numpy() for r in rows], weights,
                                        w_self)))


def make_engine(meta, rank=0, world=1, **kw):
    """The engine of a recorded run over this rank's rows of the recipe's models."""
    from decentralizepy_amd.gossip import shard
    from decentralizepy_amd.gossip_epidemic import EpidemicRound, FullShareRound
    adj = ops.graph(meta)
    lo, hi, _ = shard(meta["nodes"], world, rank)
    x = torch.from_numpy(ops.initial_models(meta)[lo:hi])
    if "device" in kw:
        x = x.to(kw["device"])
    if meta["kind"] == "el":
        return EpidemicRound(adj, x, meta["degree"], meta["random_seed"], rank=rank, world=world,
                             **kw)
    return FullShareRound(adj, x, rank=rank, world=world, **kw)


def run_and_check(eng, meta, last):
    for r in range(len(meta["rounds"])):
        eng.step()
        assert eng.round == r + 1
        el = meta["kind"] == "el"
        ops.check_round(meta, last, r, eng.x.cpu().numpy(), lo=eng.lo,
                        received=eng.received_this_round if el else None,
                        send_sets=eng.send_sets if el else None)


def test_fixture_covers_the_empty_the_uneven_and_the_full_list():
    metas = {name: ops.load(name)[0] for name in EL_RUNS}
    adj = ops.graph(metas["el_d7"])
    assert [len(a) for a in adj] == [15] * 16
    first = {n: [set(s) for s in metas[n]["rounds"][0]["send_sets"]] for n in EL_RUNS}
    got = [[len(s) for s in ops.receive_lists(adj, first[n])] for n in EL_RUNS]
    assert (min(got[0]), max(got[0])) == (2, 11)
    assert [i for i, c in enumerate(got[1]) if c == 0] == [1, 8, 10, 12]
    assert got[2] == [15] * 16
    # a node that received nothing later keeps the count of its last averaging
    d1 = metas["el_d1"]["rounds"]
    stale = [(r, i) for r in range(1, len(d1)) for i, c in enumerate(
        len(s) for s in ops.receive_lists(adj, [set(s) for s in d1[r]["send_sets"]]))
        if c == 0 and d1[r]["received_this_round"][i] != 0]
    for r, i in stale:
        assert d1[r]["received_this_round"][i] == d1[r - 1]["received_this_round"][i]


@pytest.mark.parametrize("name", EL_RUNS)
def test_sampler_draws_the_recorded_send_sets(name):
    meta, _ = ops.load(name)
    from decentralizepy_amd.gossip_epidemic import EpidemicRound
    adj = ops.graph(meta)
    eng = EpidemicRound(adj, torch.zeros(16, 8), meta["degree"], meta["random_seed"], fold=np_fold)
    for mr in meta["rounds"]:
        assert [sorted(s) for s in eng.sample(0)] == mr["send_sets"]


@pytest.mark.parametrize("name", EL_RUNS + ["fullshare6"])
def test_single_rank_reproduces_the_reference(name):
    meta, last = ops.load(name)
    eng = make_engine(meta, fold=np_fold)
    assert not eng.coll and eng.stride % 4 == 0 and eng.stride >= meta["n"]
    run_and_check(eng, meta, last)


@pytest.mark.parametrize("name", ["el_d7", "fullshare6"])
def test_numpy_engine_reproduces_the_reference(name):
    """The yardstick of the GPU tests' other shapes is itself held to the fixtures."""
    meta, last = ops.load(name)
    el = meta["kind"] == "el"
    ref = ops.NumpyRound(ops.graph(meta), ops.initial_models(meta),
                         **(dict(degree=meta["degree"], random_seed=meta["random_seed"]) if el
                            else {}))
    for r in range(len(meta["rounds"])):
        ref.step()
        ops.check_round(meta, last, r, ref.x, received=ref.received_this_round if el else None)


def _worker(rank, world, name):
    meta, last = ops.load(name)
    eng = make_engine(meta, rank=rank, world=world, fold=np_fold)
    assert eng.coll and eng.recv.shape == (eng.per * world, eng.stride)
    run_and_check(eng, meta, last)
    return eng.hi - eng.lo, eng.per


def test_two_ranks_reproduce_the_reference():
    """gloo, world 2: the all-gather carries every model; 16 nodes split 8 + 8."""
    assert spawn_gloo(_worker, 2, "el_d7") == [(8, 8), (8, 8)]


def test_three_ranks_with_a_padded_last_rank_reproduce_the_reference():
    """Neither recorded graph pads over 2 ranks (16 and 6 nodes); over 3 ranks the 16 nodes
    split 6 + 6 + 4 and the last block of the all-gather is padded.  The degree-1 run: some
    nodes receive nothing."""
    assert spawn_gloo(_worker, 3, "el_d1") == [(6, 6), (6, 6), (4, 6)]


def test_two_ranks_with_a_padded_last_rank():
    """World 2 with padding needs an odd node count: 5 nodes split 3 + 2, a ``senders`` round,
    against the node-by-node numpy engine."""
    from decentralizepy_amd.gossip import shard
    assert shard(5, 2, 1) == (3, 5, 3)
    got = spawn_gloo(_ring_worker, 2)
    want = _ring_reference()
    for lo, xs in got:
        for a, b in zip(xs, want):
            np.testing.assert_array_equal(a.view(np.uint32), b[lo:lo + len(a)].view(np.uint32))
    assert [len(xs[0]) for _, xs in got] == [3, 2]


RING5 = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (0, 2)]


def _ring_adj():
    adj = [set() for _ in range(5)]
    for a, b in RING5:
        adj[a].add(b)
        adj[b].add(a)
    return adj


def _ring_senders(t):
    """Deterministic send sets: node u sends to its neighbours v with (u + v + t) odd."""
    adj = _ring_adj()
    return [{v for v in adj[u] if (u + v + t) % 2} for u in range(5)]


def _ring_models():
    return np.stack([ops.recipe(300 + u, 203) for u in range(5)])


def _ring_reference(rounds=3):
    ref = ops.NumpyRound(_ring_adj(), _ring_models(), senders=_ring_senders)
    out = []
    for _ in range(rounds):
        ref.step()
        out.append(ref.x.copy())
    return out


def _ring_worker(rank, world):
    from decentralizepy_amd.gossip import shard
    from decentralizepy_amd.gossip_epidemic import EpidemicRound
    lo, hi, _ = shard(5, world, rank)
    eng = EpidemicRound(_ring_adj(), torch.from_numpy(_ring_models()[lo:hi]), 1, 0,
                        senders=_ring_senders, rank=rank, world=world, fold=np_fold)
    xs = []
    for _ in range(3):
        eng.step()
        xs.append(eng.x.numpy().copy())
    return lo, xs


def test_senders_override_is_honoured():
    from decentralizepy_amd.gossip_epidemic import EpidemicRound
    eng = EpidemicRound(_ring_adj(), torch.from_numpy(_ring_models()), 99, 0,
                        senders=_ring_senders, fold=np_fold)  # the degree is the sampler's only
    want = _ring_reference()
    for t in range(3):
        eng.step()
        assert eng.send_sets == _ring_senders(t)
        np.testing.assert_array_equal(eng.x.numpy().view(np.uint32), want[t].view(np.uint32))
    assert ops.receive_lists(_ring_adj(), _ring_senders(0))[3] == [2, 4]  # node 3 heard both
    with pytest.raises(ValueError):
        bad = EpidemicRound(_ring_adj(), torch.from_numpy(_ring_models()), 1, 0,
                            senders=lambda t: [set()] * 4, fold=np_fold)
        bad.step()


def test_engines_reject_what_they_do_not_implement():
    from decentralizepy_amd.gossip_epidemic import EpidemicRound, FullShareRound
    adj = _ring_adj()
    x = torch.from_numpy(_ring_models())
    for bad in (dict(exchange="peer"), dict(exchange="reduce_scatter"), dict(hbm_budget=1),
                dict(compress=True), dict(compression_class="Quantization")):
        with pytest.raises(ValueError, match="not implemented"):
            EpidemicRound(adj, x, 1, 90, fold=np_fold, **bad)
        with pytest.raises(ValueError, match="not implemented"):
            FullShareRound(adj, x, fold=np_fold, **bad)
    with pytest.raises(ValueError, match="degree"):
        EpidemicRound(adj, x, 3, 90, fold=np_fold)  # nodes 1, 3 and 4 have two neighbours


# ---- the C entry point: every check is made on the host copy, before any device call -----------
def _table(srcs, recvs):
    """The fold table's words as codec.DenseTable lays them out, from plain integers."""
    n_src, m = len(srcs), len(recvs)
    n_ent = sum(len(r[3]) for r in recvs)
    words = np.zeros(n_src + 4 * m + n_ent, dtype=np.uint64)
    words[:n_src] = srcs
    halves = words.view(np.uint32)
    pos = 0
    for j, (out, own, w_self, pairs) in enumerate(recvs):
        b = n_src + 4 * j
        words[b] = out
        halves[2 * b + 2] = np.int32(own).view(np.uint32)
        halves[2 * b + 3] = np.float32(w_self).view(np.uint32)
        halves[2 * b + 4], halves[2 * b + 5] = pos, len(pairs)
        for s, w in pairs:
            e = n_src + 4 * m + pos
            halves[2 * e] = np.int32(s).view(np.uint32)
            halves[2 * e + 1] = np.float32(w).view(np.uint32)
            pos += 1
    return words, n_ent


def test_argument_validation_without_gpu():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    ARG, UNSUP = _lib.DPZ_ERR_ARG, _lib.DPZ_ERR_UNSUPPORTED
    n = 100
    row = 1 << 36  # addresses that are never dereferenced (rows of 2^31 floats stay apart)
    srcs = [row * (1 + s) for s in range(3)]
    outs = [row * (10 + j) for j in range(2)]
    good = [(outs[0], 0, 0.5, [(1, 0.25), (2, 0.25)]), (outs[1], 2, 1.0, [])]

    def call(srcs=srcs, recvs=good, m=None, n=n, mode=3, dev=row, host=True, n_src=None,
             n_ent=None):
        words, ne = _table(srcs, recvs)
        return L.dpz_dense_average_nodes(
            len(recvs) if m is None else m, dev,
            ctypes.c_void_p(words.ctypes.data) if host else None,
            ne if n_ent is None else n_ent, len(srcs) if n_src is None else n_src, n, mode, None)

    # every call here must stop at a check: nothing may reach a launch on this machine
    assert call(mode=3) == ARG and call(mode=-1) == ARG
    assert call(mode=0, n=1 << 31) == UNSUP
    assert call(mode=0, m=0) == ARG and call(mode=0, n=0) == ARG and call(mode=0, n_src=0) == ARG
    assert call(mode=0, dev=None) == ARG and call(mode=0, host=False) == ARG
    assert call(mode=0, n_ent=-1) == ARG
    assert call(mode=0, srcs=[srcs[0], 0, srcs[2]]) == ARG  # a null source row
    assert call(mode=0, recvs=[(0, 0, 0.5, [])]) == ARG     # a null out row
    # an index outside [0, n_src): a list entry, a receiver's own row
    assert call(mode=0, recvs=[(outs[0], 0, 0.5, [(3, 0.5)])]) == ARG
    assert call(mode=0, recvs=[(outs[0], 0, 0.5, [(-1, 0.5)])]) == ARG
    assert call(mode=0, recvs=[(outs[0], 3, 0.5, [(1, 0.5)])]) == ARG
    assert call(mode=0, recvs=[(outs[0], -1, 0.5, [(1, 0.5)])]) == ARG
    assert call(mode=0, recvs=good, n_ent=1) == ARG  # a list past the entries
    # an out row that equals a source row, overlaps one from either side, or another out row
    for out in (srcs[1], srcs[1] + 4 * (n - 1), srcs[1] - 4 * (n - 1)):
        assert call(mode=0, recvs=[(out, 0, 0.5, [(1, 0.5)])]) == ARG, out
    assert call(mode=0, recvs=[(outs[0], 0, 0.5, []), (outs[0] + 4, 1, 0.5, [])]) == ARG
    # 65 source rows fit no tile: the staged path is unsupported there, and says so up front
    many = [row * (20 + s) for s in range(65)]
    assert L.dpz_dense_tile_elems(65) == 0
    assert call(mode=1, srcs=many, recvs=[(outs[0], 0, 0.5, [(64, 0.5)])]) == UNSUP
    assert L.dpz_abi_version() == 2  # symbols were added, nothing changed


def test_tile_rule():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    want = {0: 0, -3: 0, 1: 1024, 2: 1024, 16: 1024, 17: 512, 32: 512, 33: 256, 64: 256, 65: 0,
            96: 0}
    for n_src, tile in want.items():
        assert L.dpz_dense_tile_elems(n_src) == tile, n_src
        if tile:  # the largest of 1024 / 512 / 256 whose rows fit 64 KiB
            assert n_src * tile * 4 <= 65536 and (tile == 1024 or n_src * 2 * tile * 4 > 65536)


def test_auto_rule():
    """Staged iff a tile fits, staging at least halves the row reads, and n spans 384 tiles."""
    from decentralizepy_amd import _lib
    L = _lib.lib()
    STAGED, DIRECT = _lib.DPZ_DENSE_STAGED, _lib.DPZ_DENSE_DIRECT
    el = (16, 16 * 8)  # the EL tutorial round: 16 sources, 16 receivers of 7 senders
    assert L.dpz_dense_auto_mode(*el, 89_834) == DIRECT       # 88 tiles: measured slower staged
    assert L.dpz_dense_auto_mode(*el, 200_000) == DIRECT      # 196 tiles: measured slower staged
    assert L.dpz_dense_auto_mode(*el, 400_000) == STAGED      # 391 tiles: measured faster staged
    assert L.dpz_dense_auto_mode(*el, 11_000_000) == STAGED
    assert L.dpz_dense_auto_mode(*el, 383 * 1024) == DIRECT
    assert L.dpz_dense_auto_mode(*el, 383 * 1024 + 1) == STAGED
    assert L.dpz_dense_auto_mode(16, 31, 11_000_000) == DIRECT  # 2 n_src > the row reads
    assert L.dpz_dense_auto_mode(16, 32, 11_000_000) == STAGED
    assert L.dpz_dense_auto_mode(17, 128, 383 * 512 + 1) == STAGED  # tile 512
    assert L.dpz_dense_auto_mode(17, 128, 383 * 512) == DIRECT
    assert L.dpz_dense_auto_mode(96, 476, 11_000_000) == DIRECT  # no tile fits 96 sources
    assert L.dpz_dense_auto_mode(0, 476, 11_000_000) == DIRECT
    assert L.dpz_dense_auto_mode(16, 128, 0) == DIRECT


def test_header_library_and_ctypes_table_agree():
    import re
    from decentralizepy_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "dpz_codec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dpz_[a-z0-9_]+)\s*\(", text))
    assert {"dpz_dense_average_nodes", "dpz_dense_tile_elems"} <= declared
    assert set(_lib.SIGNATURES) == declared
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(handle, s) for s in declared)
    assert len(_lib.SIGNATURES["dpz_dense_average_nodes"][1]) == 8
    for name, value in (("DPZ_DENSE_AUTO", 0), ("DPZ_DENSE_STAGED", 1), ("DPZ_DENSE_DIRECT", 2)):
        assert re.search(rf"#define {name} {value}\b", text) and getattr(_lib, name) == value
    assert handle.dpz_abi_version() == 2
