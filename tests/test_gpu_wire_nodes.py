"""GPU: the batched wire coder ``dpz_wire_encode_nodes`` byte for byte against the oracles and the
single-stream coders at the Elias block edge (1024 codes) and the value block edge (256 values),
its per-node failure handling, and the engines' ``wire_bytes()`` / ``wire_payload()``."""
import numpy as np
import pytest
import torch

from oracle import elias as oelias
from oracle import fpz as ofpz
from tests import jwins_round_ops as ops
from tests.test_cpu_wire_nodes import KS, index_list

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
VAL_KINDS = ["normal", "zeros", "denormal", "special", "oneexp"]


def values(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros(n, dtype=np.float32)
    if kind == "denormal":
        sign = rng.integers(0, 2, n, dtype=np.uint32) << 31
        return (rng.integers(1, 1 << 23, n, dtype=np.uint32) | sign).view(np.float32)
    if kind == "oneexp":
        return rng.uniform(1, 2, n).astype(np.float32)  # exponent 127 throughout
    v = rng.standard_normal(n).astype(np.float32)
    if kind == "special":  # +inf, -inf, a NaN with a low payload bit, -0
        bits = np.array([0x7F800000, 0xFF800000, 0x7FC00001, 0x80000000], dtype=np.uint32)
        v.view(np.uint32)[:min(n, 4)] = bits[:n]
    return v


def catalog():
    """(indices or None, values) per node: every index count x gap pattern, [0, 2^31 - 1], indices
    at the value block edge, and full shares of every value count x content."""
    lists = [index_list(kind, k) for k in KS for kind in ("ones", "pow9", "log")]
    lists += [np.array([0, 2 ** 31 - 1], dtype=np.int32)]
    lists += [index_list("log", k, seed=1) for k in (255, 256, 257)]
    nodes = [(idx, values(VAL_KINDS[j % 5], idx.size, j)) for j, idx in enumerate(lists)]
    nodes += [(None, values(kind, n, n)) for n in (1, 255, 256, 257, 1025) for kind in VAL_KINDS]
    return nodes


CATALOG = catalog()
PICKS = {1: [14], 3: [11, 37, 17], 70: [j % len(CATALOG) for j in range(70)]}


def run_nodes(dev, codec, nodes, precision, size_only=(), idx_cap=None, val_cap=None):
    """One batched call; inputs and slots are 4-byte aligned only relative to each other.
    Returns (sizes, status, [(idx slot, val slot) bytes])."""
    m = len(nodes)
    ni = sum(v.size + 1 for _, v in nodes)
    idx_in = torch.zeros(ni, dtype=torch.int32, device=dev)
    val_in = torch.zeros(ni, dtype=torch.float32, device=dev)
    L = codec._lib.lib()
    tab = codec.WireNodesTable(m, dev)
    off, pos, place = 0, 0, []
    for j, (idx, vals) in enumerate(nodes):
        n = vals.size
        val_in[off:off + n] = torch.from_numpy(vals).to(dev)
        if idx is not None:
            idx_in[off:off + n] = torch.from_numpy(idx).to(dev)
        ci = 0 if idx is None else codec.elias_bound_bytes(n, int(idx[-1]) + 1)
        cv = int(L.dpz_fpz_max_bytes(n))
        ci = idx_cap.get(j, ci) if idx_cap else ci
        cv = val_cap.get(j, cv) if val_cap else cv
        place.append((pos, ci, pos + ci + 4, cv))
        pos += ci + cv + 8
        off += n + 1
    slots = torch.full((pos,), SENTINEL, dtype=torch.uint8, device=dev)
    off = 0
    for j, (idx, vals) in enumerate(nodes):
        oi, ci, ov, cv = place[j]
        out = j not in size_only
        tab.set(j, None if idx is None else idx_in[off:], val_in[off:], vals.size,
                slots[oi:] if out and idx is not None else None, slots[ov:] if out else None,
                ci, cv)
        off += vals.size + 1
    tab.upload()
    sizes = torch.full((m, 2), -1, dtype=torch.int64, device=dev)
    status = torch.full((m,), 77, dtype=torch.int32, device=dev)
    codec.wire_encode_nodes(tab, sizes, status, precision)
    host = slots.cpu().numpy()
    return (sizes.cpu().numpy(), status.cpu().numpy(),
            [(host[oi:oi + ci + 4], host[ov:ov + cv + 4]) for oi, ci, ov, cv in place])


def check_slot(slot, want, what):
    """The slot starts with the stream and keeps the sentinel in every byte past it."""
    n = 0 if want is None else want.size
    assert n == 0 or np.array_equal(slot[:n], want), what
    assert (slot[n:] == SENTINEL).all(), what


@pytest.mark.parametrize("precision", [0, 16])
@pytest.mark.parametrize("m", [1, 3, 70])
def test_streams_equal_the_oracles_and_the_single_coders(dev, m, precision):
    from decentralizepy_amd import codec
    nodes = [CATALOG[j] for j in PICKS[m]]
    size_only = set(range(2, m, 7))
    sizes, status, slots = run_nodes(dev, codec, nodes, precision, size_only)
    assert not status.any()
    for j, (idx, vals) in enumerate(nodes):
        want_i = None if idx is None else oelias.encode(idx)
        want_v = ofpz.encode(vals, precision)
        if idx is not None:
            one = codec.elias_encode(torch.from_numpy(idx).to(dev)).cpu().numpy()
            assert np.array_equal(one, want_i), j
        one = codec.fpz_encode(torch.from_numpy(vals).to(dev), precision).cpu().numpy()
        assert np.array_equal(one, want_v), j
        assert sizes[j].tolist() == [0 if idx is None else want_i.size, want_v.size], j
        written = j not in size_only
        check_slot(slots[j][0], want_i if written else None, (j, "idx"))
        check_slot(slots[j][1], want_v if written else None, (j, "val"))


def test_a_bad_list_and_a_short_slot_stay_with_their_node(dev):
    from decentralizepy_amd import _lib, codec
    good = CATALOG[14]                                  # k = 2049, log-uniform gaps
    bad = (good[0].copy(), good[1])
    bad[0][1500] = bad[0][1499]                         # a repeated index in the second block
    streams = [(oelias.encode(i), ofpz.encode(v)) for i, v in (good, good, CATALOG[4])]
    short_i = (streams[2][0].size + 3) // 4 * 4 - 4     # one word short of the stream
    short_v = streams[2][1].size - 4
    sizes, status, slots = run_nodes(dev, codec, [good, bad, CATALOG[4], good], 0,
                                     idx_cap={2: short_i}, val_cap={2: short_v})
    assert status.tolist() == [0, 1, 2 | 4, 0]
    for j in (0, 3):                                    # the neighbours are exact
        check_slot(slots[j][0], streams[0][0], j)
        check_slot(slots[j][1], streams[0][1], j)
        assert sizes[j].tolist() == [streams[0][0].size, streams[0][1].size]
    check_slot(slots[1][0], None, "bad list: no index stream")
    check_slot(slots[1][1], streams[1][1], "bad list: its values are coded")
    check_slot(slots[2][0], None, "short index slot")
    check_slot(slots[2][1], None, "short value slot")
    assert sizes[2].tolist() == [streams[2][0].size, streams[2][1].size]
    # one index is no Elias stream: refused on the host table, nothing enqueued or written
    tab = codec.WireNodesTable(1, dev)
    one = torch.zeros(4, dtype=torch.int32, device=dev)
    tab.set(0, one, one.view(torch.float32), 1)
    tab.upload()
    sizes = torch.full((1, 2), -1, dtype=torch.int64, device=dev)
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    assert codec.wire_encode_nodes(tab, sizes, status, check_rc=False) == _lib.DPZ_ERR_ARG
    assert sizes.tolist() == [[-1, -1]] and status.tolist() == [77]


def _engine(which, dev):
    from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound, JwinsWaveletBatchRound
    from decentralizepy_amd.gossip_topkacc import TopKAccRound
    adj = ops.run_adjacency(next(m for m, _ in ops.load_runs() if m["name"] == "irr6"))
    n = 2051 if which == "topkacc" else 1030
    x = torch.randn(len(adj), n, generator=torch.Generator().manual_seed(11)).to(dev)
    if which == "jwins":
        return JwinsBatchRound(adj, x, ops.TUTORIAL_ALPHAS, device=dev)
    if which == "wavelet":
        return JwinsWaveletBatchRound(adj, x, ops.TUTORIAL_ALPHAS, wavelet="db4", level=2,
                                      device=dev)
    return TopKAccRound(adj, x, 0.1, device=dev)


@pytest.mark.parametrize("which", ["jwins", "wavelet", "topkacc"])
def test_engine_wire_layer_equals_the_plugin_streams_and_leaves_the_round_alone(dev, which):
    from decentralizepy_amd.compression.EliasFpzip import EliasFpzip
    eng, plain = _engine(which, dev), _engine(which, dev)
    comp = EliasFpzip()
    partial = full = 0
    for r in range(2):
        for e in (eng, plain):
            e.x.add_(torch.roll(e.x, r + 1, 1), alpha=0.01)  # a round of "training"
            e.step()
        got = eng.wire_bytes()
        assert got.is_cuda and got.dtype == torch.int64 and eng.wire_bytes() is got
        for q in range(eng.n_nodes):
            idx, vals = (t if t is None else t.cpu().numpy() for t in eng.payload(q))
            msg = eng.wire_payload(q)
            want = [0 if idx is None else oelias.encode(idx).size, ofpz.encode(vals).size]
            assert got[q].tolist() == want == [
                msg["indices"].size if idx is not None else 0, msg["params"].size]
            back = np.atleast_1d(comp.decompress_float(msg["params"]))
            assert np.array_equal(back.view(np.uint32), vals.view(np.uint32))
            if idx is None:
                full += 1
                assert set(msg) == {"params"}
            else:
                partial += 1
                assert np.array_equal(comp.decompress(msg["indices"]), idx)
                alpha = eng.alpha if which == "topkacc" else eng.alphas[q]
                assert msg["alpha"] == alpha and msg["send_partial"] is True
    assert partial and (full or which == "topkacc")
    for name in ("x", "x0", "acc", "counter"):
        assert torch.equal(getattr(eng, name), getattr(plain, name)), name
