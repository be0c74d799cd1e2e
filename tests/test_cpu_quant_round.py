"""CPU: the quantised whole-topology full-model rounds (decentralizepy_amd/gossip_quant.py) — the
rows, the sharding, the exchange and the fold order with the numpy restatements
(tests/quantization_ops.py, tests/epidemic_ops.py) standing in for the HIP kernels, against the
runs recorded from the unmodified reference (tests/golden/quant_round.json,
make_golden_quant_round.py); and the argument checks of ``dpz_quant_encode_nodes`` and
``dpz_qdense_average_nodes``, which are all made before a device is touched.  The device path is
covered by tests/test_gpu_quant_round.py, which shares the helpers here."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import quant_round_ops as ops
from tests import quantization_ops as qops
from tests.dist_harness import spawn_gloo


def np_encode(x, k):
    return qops.encode(x.numpy(), k)


def np_fold(local, payloads, weights, w_self, out):
    out.copy_(torch.from_numpy(ops.fold(local.numpy(), payloads, weights, w_self)))


NP = dict(encode=np_encode, fold=np_fold)


def make_engine(meta, rank=0, world=1, **kw):
    """The engine of a recorded run over this rank's rows of the recipe's models."""
    from decentralizepy_amd.gossip import shard
    from decentralizepy_amd.gossip_quant import QuantEpidemicRound, QuantFullShareRound
    adj = ops.graph(meta)
    lo, hi, _ = shard(meta["nodes"], world, rank)
    x = torch.from_numpy(ops.initial_models(meta)[lo:hi])
    if "device" in kw:
        x = x.to(kw["device"])
    k = meta["float_precision"]
    if meta["kind"] == "el":
        return QuantEpidemicRound(adj, x, meta["degree"], meta["random_seed"], k, rank=rank,
                                  world=world, **kw)
    return QuantFullShareRound(adj, x, k, rank=rank, world=world, **kw)


def run_and_check(eng, meta, arrays):
    el = meta["kind"] == "el"
    for r in range(len(meta["rounds"])):
        eng.step()
        assert eng.round == r + 1
        eng.check()
        if r == 0:  # the rows still hold round 0's wire: the owned nodes', every node's gathered
            for q in (range(meta["nodes"]) if eng.coll else range(eng.lo, eng.hi)):
                ops.check_wire(meta, arrays, q, *eng.payload(q))
        ops.check_round(meta, arrays, r, eng.x.cpu().numpy(), lo=eng.lo,
                        received=eng.received_this_round if el else None,
                        send_sets=eng.send_sets if el else None)


def test_fixture_covers_w9_w16_and_the_empty_list():
    metas = {name: ops.load(name)[0] for name in ops.RUNS}
    a, b, c = (metas[n] for n in ops.RUNS)
    assert a["n"] == 2001 and a["n"] % 4 and {w["w"] for w in a["wire"]} == {9}
    assert b["n"] == 1031 and {w["w"] for w in b["wire"] + c["wire"]} == {16}
    adj = ops.graph(c)
    got = [len(s) for s in ops.eops.receive_lists(
        adj, [set(s) for s in c["rounds"][0]["send_sets"]])]
    assert 0 in got
    with open(os.path.join(ops.GOLDEN, "quant_round.json")) as f:
        assert "numpy" in __import__("json").load(f)


@pytest.mark.parametrize("name", ops.RUNS)
def test_numpy_engine_reproduces_the_reference(name):
    """The yardstick of the GPU tests' other shapes is itself held to the fixtures."""
    meta, arrays = ops.load(name)
    el = meta["kind"] == "el"
    ref = ops.NumpyQuantRound(ops.graph(meta), ops.initial_models(meta), meta["float_precision"],
                              **(dict(degree=meta["degree"], random_seed=meta["random_seed"])
                                 if el else {}))
    for r in range(len(meta["rounds"])):
        ref.step()
        if r == 0:
            for q, (scale, to_send) in enumerate(ref.wire):
                ops.check_wire(meta, arrays, q, scale, to_send)
        ops.check_round(meta, arrays, r, ref.x, received=ref.received_this_round if el else None)


def test_an_uncompressed_round_computes_something_else():
    meta, arrays = ops.load("el_d7_q32767")
    ref = ops.eops.NumpyRound(ops.graph(meta), ops.initial_models(meta), degree=meta["degree"],
                              random_seed=meta["random_seed"])
    ref.step()
    assert ops.eops.sha(ref.x[0]) != meta["rounds"][0]["model_sha"][0]


@pytest.mark.parametrize("name", ops.RUNS)
def test_single_rank_reproduces_the_reference(name):
    meta, arrays = ops.load(name)
    eng = make_engine(meta, **NP)
    assert not eng.coll and eng.stride % 4 == 0 and eng.row_words % 4 == 0
    assert eng.slot_bits == meta["wire"][0]["w"]  # the default slot is exactly the width here
    run_and_check(eng, meta, arrays)


def _worker(rank, world, name):
    meta, arrays = ops.load(name)
    eng = make_engine(meta, rank=rank, world=world, **NP)
    assert eng.coll and eng.recv.shape == (eng.per * world, eng.row_words)
    assert eng.recv.dtype == torch.int32  # the packed rows travel, not the fp32 models
    run_and_check(eng, meta, arrays)
    return eng.hi - eng.lo, eng.per


def test_two_ranks_reproduce_the_reference():
    """gloo, world 2: the all-gather carries every packed row; 16 nodes split 8 + 8."""
    assert spawn_gloo(_worker, 2, "el_d7_q32767") == [(8, 8), (8, 8)]
    assert spawn_gloo(_worker, 2, "fullshare6_q255") == [(3, 3), (3, 3)]


def test_three_ranks_with_a_padded_last_block_reproduce_the_reference():
    """16 nodes over 3 ranks split 6 + 6 + 4: the last block of the all-gather is padded.  The
    degree-1 run: some nodes receive nothing."""
    assert spawn_gloo(_worker, 3, "el_d1_q32767") == [(6, 6), (6, 6), (4, 6)]


def test_payload_is_the_recorded_wire():
    meta, arrays = ops.load("fullshare6_q255")
    eng = make_engine(meta, **NP)
    eng.encode()
    for q in range(meta["nodes"]):
        scale, to_send = eng.payload(q)
        ops.check_wire(meta, arrays, q, scale, to_send)
    np.testing.assert_array_equal(eng.payload(5)[1], arrays["to_send_5"])
    assert eng.payload(0)[1][:2].tolist() == [7, 9]  # 2001 * 9 = 18,009 bits: 7 bits of padding


def test_default_slot_holds_the_width():
    from decentralizepy_amd.gossip_quant import default_slot_bits
    for k in (1, 7, 127, 255, 256, 32767, 2 ** 20, 2 ** 24 - 1, 2 ** 30 - 1):
        slot = default_slot_bits(k)
        assert 2 <= slot <= 32
        for seed in range(6):
            for scale in (1.0, 1e-3, 3e7):
                w = qops.params(qops.recipe(seed, 257, scale), k)[3]
                assert w <= slot, (k, seed, scale, w, slot)
        if k <= 2 ** 22:  # exactly the width: nothing is wasted at the default
            assert qops.params(qops.recipe(0, 257), k)[3] == slot
    assert [default_slot_bits(k) for k in (255, 32767)] == [9, 16]


def wide_field_model(n):
    """Multiples of the smallest subnormal with max|x| = 300 ulp: at k = 255 the norm rounds to
    one ulp, so qmax = 300 and the field is 10 bits wide, one more than the default slot."""
    v = np.arange(n, dtype=np.float64) % 299 - 149
    v[0] = 300
    return (v * 2.0 ** -149).astype(np.float32)


def test_a_field_wider_than_the_slot_changes_no_model():
    """A subnormal norm widens the field: status 4 on that node's row, every model stays, and
    check() names the node."""
    from decentralizepy_amd.gossip_quant import QuantFullShareRound
    meta, _ = ops.load("fullshare6_q255")
    x = ops.initial_models(meta)[:, :300].copy()
    x[2] = wide_field_model(300)
    assert qops.params(x[2], 255)[3] == 10
    eng = QuantFullShareRound(ops.graph(meta), torch.from_numpy(x), 255, **NP)
    eng.step()
    np.testing.assert_array_equal(eng.x.numpy().view(np.uint32), x.view(np.uint32))
    with pytest.raises(RuntimeError, match=r"nodes \[2\].*wider than the slot"):
        eng.check()
    wide = QuantFullShareRound(ops.graph(meta), torch.from_numpy(x), 255, slot_bits=32, **NP)
    wide.step()
    wide.check()
    assert (wide.x.numpy() != x).any()


def test_constructor_errors():
    from decentralizepy_amd.gossip_quant import QuantEpidemicRound, QuantFullShareRound
    meta, _ = ops.load("fullshare6_q255")
    adj = ops.graph(meta)
    x = torch.zeros(6, 8)
    for bad in (dict(exchange="peer"), dict(exchange="reduce_scatter"), dict(hbm_budget=1),
                dict(compression_class="EliasQuantization")):
        with pytest.raises(ValueError, match="not implemented"):
            QuantFullShareRound(adj, x, **NP, **bad)
        with pytest.raises(ValueError, match="not implemented"):
            QuantEpidemicRound(adj, x, 1, 90, **NP, **bad)
    for k in (1.5, "255", True, None):
        with pytest.raises(TypeError, match="float_precision"):
            QuantFullShareRound(adj, x, k, **NP)
    for k in (0, -3, 2 ** 30 + 1):
        with pytest.raises(ValueError, match="float_precision"):
            QuantFullShareRound(adj, x, k, **NP)
        with pytest.raises(ValueError, match="float_precision"):
            QuantEpidemicRound(adj, x, 1, 90, k, **NP)
    for bits in (1, 33):
        with pytest.raises(ValueError, match="slot_bits"):
            QuantFullShareRound(adj, x, 255, slot_bits=bits, **NP)
    with pytest.raises(ValueError, match="together"):
        QuantFullShareRound(adj, x, 255, encode=np_encode)
    with pytest.raises(ValueError, match="degree"):
        QuantEpidemicRound(adj, x, 3, 90, **NP)  # the smallest neighbourhood of EDGES6 is 2
    with pytest.raises(ValueError, match="rows"):
        QuantFullShareRound(adj, torch.zeros(5, 8), **NP)
    assert QuantFullShareRound(adj, x, np.int64(255), **NP).k == 255


def test_the_plain_engines_still_reject_compression():
    from decentralizepy_amd.gossip_epidemic import FullShareRound
    meta, _ = ops.load("fullshare6_q255")
    with pytest.raises(ValueError, match="not implemented"):
        FullShareRound(ops.graph(meta), torch.zeros(6, 8), compress=True)


# ---- the C entry points: every check is made on the host, before any device call ---------------
def _table(srcs, recvs):
    """The fold table's words as codec.QDenseTable lays them out, from plain integers."""
    n_src, m = len(srcs), len(recvs)
    n_ent = sum(len(r[3]) for r in recvs)
    words = np.zeros(n_src + 4 * m + n_ent, dtype=np.uint64)
    words[:n_src] = srcs
    halves = words.view(np.uint32)
    pos = 0
    for j, (out, own, w_self, pairs) in enumerate(recvs):
        b = n_src + 4 * j
        words[b], words[b + 1] = out, own
        halves[2 * b + 4] = np.float32(w_self).view(np.uint32)
        halves[2 * b + 6], halves[2 * b + 7] = pos, len(pairs)
        for s, w in pairs:
            e = n_src + 4 * m + pos
            halves[2 * e] = np.int32(s).view(np.uint32)
            halves[2 * e + 1] = np.float32(w).view(np.uint32)
            pos += 1
    return words, n_ent


def test_fold_argument_validation_without_gpu():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    ARG, UNSUP = _lib.DPZ_ERR_ARG, _lib.DPZ_ERR_UNSUPPORTED
    n, cap = 100, 50
    row = 1 << 36  # addresses that are never dereferenced (rows of 2^31 floats stay apart)
    srcs = [row * (1 + s) for s in range(3)]
    outs = [row * (10 + j) for j in range(2)]
    owns = [row * (20 + j) for j in range(2)]
    good = [(outs[0], owns[0], 0.5, [(1, 0.25), (2, 0.25)]), (outs[1], owns[1], 1.0, [])]

    def call(srcs=srcs, recvs=good, m=None, n=n, cap=cap, mode=3, dev=row, host=True,
             n_src=None, n_ent=None, guard=None, guard_n=0):
        words, ne = _table(srcs, recvs)
        return L.dpz_qdense_average_nodes(
            len(recvs) if m is None else m, dev,
            ctypes.c_void_p(words.ctypes.data) if host else None,
            ne if n_ent is None else n_ent, len(srcs) if n_src is None else n_src, n, cap, mode,
            guard, guard_n, None)

    # every call here must stop at a check: nothing may reach a launch on this machine
    assert call(mode=3) == ARG and call(mode=-1) == ARG
    assert call(mode=0, n=1 << 31, cap=1) == UNSUP
    assert call(mode=0, m=0) == ARG and call(mode=0, n=0) == ARG and call(mode=0, n_src=0) == ARG
    assert call(mode=0, dev=None) == ARG and call(mode=0, host=False) == ARG
    assert call(mode=0, n_ent=-1) == ARG
    assert call(mode=0, cap=0) == ARG and call(mode=0, cap=n + 1) == ARG
    assert call(mode=0, guard_n=-1) == ARG and call(mode=0, guard_n=4) == ARG
    assert call(mode=0, guard=row + 2, guard_n=4) == ARG            # a misaligned guard
    assert call(mode=0, srcs=[srcs[0], 0, srcs[2]]) == ARG          # a null packed row
    assert call(mode=0, srcs=[srcs[0], srcs[1] + 2, srcs[2]]) == ARG  # a misaligned one
    assert call(mode=0, recvs=[(0, owns[0], 0.5, [])]) == ARG       # a null out row
    assert call(mode=0, recvs=[(outs[0], 0, 0.5, [])]) == ARG       # a null own row
    assert call(mode=0, recvs=[(outs[0] + 1, owns[0], 0.5, [])]) == ARG
    # an index outside [0, n_src), a list past the entries
    assert call(mode=0, recvs=[(outs[0], owns[0], 0.5, [(3, 0.5)])]) == ARG
    assert call(mode=0, recvs=[(outs[0], owns[0], 0.5, [(-1, 0.5)])]) == ARG
    assert call(mode=0, recvs=good, n_ent=1) == ARG
    # an out row that touches a packed row (header and body included), an own row, an out row
    row_bytes = 4 * (12 + cap)
    for out in (srcs[1], srcs[1] + row_bytes - 4, srcs[1] - 4 * (n - 1)):
        assert call(mode=0, recvs=[(out, owns[0], 0.5, [(1, 0.5)])]) == ARG, out
    assert call(mode=0, recvs=[(owns[0], owns[0], 0.5, [])]) == ARG  # in place
    assert call(mode=0, recvs=[(outs[0], owns[0], 0.5, []),
                               (outs[1], outs[0] + 4 * (n - 1), 0.5, [])]) == ARG
    assert call(mode=0, recvs=[(outs[0], owns[0], 0.5, []),
                               (outs[0] + 4, owns[1], 0.5, [])]) == ARG
    # 65 packed rows fit no tile: the staged path is unsupported there, and says so up front
    many = [row * (30 + s) for s in range(65)]
    assert L.dpz_qdense_tile_elems(65) == 0
    assert call(mode=1, srcs=many, recvs=[(outs[0], owns[0], 0.5, [(64, 0.5)])]) == UNSUP
    for n_src in (1, 16, 17, 33, 64):  # a tile starts on a dword of every body
        assert L.dpz_qdense_tile_elems(n_src) % 32 == 0 and L.dpz_qdense_tile_elems(n_src) > 0
    assert L.dpz_abi_version() == 2  # symbols were added, nothing changed


def test_encode_argument_validation_without_gpu():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    ARG, UNSUP, WS = _lib.DPZ_ERR_ARG, _lib.DPZ_ERR_UNSUPPORTED, _lib.DPZ_ERR_WORKSPACE
    p = 1 << 36
    need = L.dpz_quant_encode_nodes_workspace_bytes(3, 20000)
    assert need == 3 * (1024 + 4 * 3)  # per node: 256 max words and one sum per 8192 elements
    assert L.dpz_quant_encode_nodes_workspace_bytes(1, 20000) == L.dpz_quant_workspace_bytes(20000)
    assert L.dpz_quant_encode_nodes_workspace_bytes(0, 5) == 0
    assert L.dpz_quant_encode_nodes_workspace_bytes(1, 1 << 31) == 0

    def call(m=3, tab=p, n=20000, k=255, bits=9, ws=2 * p, ws_bytes=need):
        return L.dpz_quant_encode_nodes(m, tab, n, k, bits, ws, ws_bytes, None)

    assert call(m=0) == ARG and call(n=0) == ARG
    assert call(k=0) == ARG and call(k=2 ** 30 + 1) == ARG
    assert call(bits=1) == ARG and call(bits=33) == ARG
    assert call(tab=None) == ARG and call(ws=None) == ARG
    assert call(ws=2 * p + 8) == ARG and call(tab=p + 4) == ARG
    assert call(n=1 << 31) == UNSUP and call(m=65536) == UNSUP
    assert call(ws_bytes=need - 1) == WS
    assert L.dpz_quant_row_words(2001, 9) == 12 + (2001 * 9 + 31) // 32
    assert L.dpz_quant_row_words(0, 9) == 0 and L.dpz_quant_row_words(5, 33) == 0
