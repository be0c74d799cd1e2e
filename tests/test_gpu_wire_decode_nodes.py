"""GPU: the batched wire decoder ``dpz_wire_decode_nodes`` against the oracles at the chunk, super
map and value block edges, its per-node rejection of malformed streams, and ``TopKAccRound``'s
coded exchange against the uncoded round."""
import functools

import numpy as np
import pytest
import torch

from oracle import elias as oelias
from oracle import fpz as ofpz
from tests.dist_harness import rccl_loopback
from tests.test_cpu_topkacc_round import run_named
from tests.test_cpu_wire_nodes import KS, index_list
from tests.test_gpu_wire_nodes import values

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
FULL = 18  # a full share's place in the catalog


@functools.lru_cache(maxsize=None)
def catalog(precision):
    """(indices or None, index stream or None, value stream, decoded values) per node."""
    lists = [index_list(kind, k) for k in KS for kind in ("ones", "pow16", "log")]
    lists += [None]                                           # FULL: 257 values, no indices
    lists += [index_list("ones", k) for k in (65537, 65538)]  # one super map, and one bit over
    lists += [np.array([0, 2 ** 31 - 1], dtype=np.int32)]     # one 61-bit code
    lists += [index_list("log", k, seed=1) for k in (256, 257)]
    nodes = []
    for j, idx in enumerate(lists):
        vs = ofpz.encode(values(["normal", "special", "oneexp"][j % 3],
                                257 if idx is None else idx.size, j), precision)
        nodes.append((idx, None if idx is None else oelias.encode(idx), vs, ofpz.decode(vs)))
    return nodes


# m = 3: the three-super stream (33-bit codes straddling chunks), a full share, one chunk + 1 bit
PICKS = {1: [16], 3: [16, FULL, 9], 70: [j % 24 for j in range(70)]}


def decode_nodes(dev, codec, nodes, precision, sizes=None, counts=None):
    """One batched call over (idx, index stream, value stream, values) nodes.  Returns (status,
    [(indices, values, guards intact)])."""
    m = len(nodes)
    up4 = lambda v: -(-v // 4) * 4
    counts = counts or [n[3].size for n in nodes]
    caps = [(0 if n[1] is None else up4(n[1].size), n[2].size) for n in nodes]
    slots = torch.zeros(sum(a + b for a, b in caps) + 4, dtype=torch.uint8, device=dev)
    out_i = torch.full((sum(counts) + 4 * m,), GUARD, dtype=torch.int32, device=dev)
    out_v = torch.full((sum(counts) + 4 * m,), GUARD, dtype=torch.int32, device=dev)
    real = [[0 if n[1] is None else n[1].size, n[2].size] for n in nodes]
    dsizes = torch.tensor(sizes or real, dtype=torch.int64, device=dev)
    tab = codec.WireDecodeTable(m, dev)
    pos = off = 0
    place = []
    for j, (idx, si, sv, _) in enumerate(nodes):
        ci, cv = caps[j]
        if si is not None:
            slots[pos:pos + si.size] = torch.from_numpy(si).to(dev)
        slots[pos + ci:pos + ci + cv] = torch.from_numpy(sv).to(dev)
        tab.set(j, slots[pos:] if ci else None, slots[pos + ci:], counts[j],
                out_i[off:] if ci else None, out_v[off:].view(torch.float32), dsizes[j], ci, cv)
        place.append(off)
        pos, off = pos + ci + cv, off + up4(counts[j]) + 1  # odd offsets: 4-byte aligned only
    tab.upload()
    status = torch.full((m,), 77, dtype=torch.int32, device=dev)
    codec.wire_decode_nodes(tab, status, precision)
    hi, hv = out_i.cpu().numpy(), out_v.cpu().numpy()
    ends = place[1:] + [hi.size]
    res = []
    for j, (o, e) in enumerate(zip(place, ends)):
        c = counts[j]
        intact = (hv[o + c:e] == GUARD).all() and (hi[o + (c if caps[j][0] else 0):e] == GUARD).all()
        res.append((hi[o:o + c], hv[o:o + c].view(np.float32), bool(intact)))
    return status.cpu().numpy(), res


@pytest.mark.parametrize("precision", [0, 9, 16])
@pytest.mark.parametrize("m", [1, 3, 70])
def test_decode_equals_the_oracles(dev, m, precision):
    from decentralizepy_amd import codec
    nodes = [catalog(precision)[j] for j in PICKS[m]]
    chunks = [-(-(n[1].size - 16) * 8 // 1024) for n in nodes if n[1] is not None]
    assert m < 70 or max(chunks) >= 10 * min(chunks)  # idle workgroups run
    status, res = decode_nodes(dev, codec, nodes, precision)
    assert not status.any(), status
    for j, ((idx, _, _, vals), (gi, gv, intact)) in enumerate(zip(nodes, res)):
        assert intact, j
        assert np.array_equal(gv.view(np.uint32), vals.view(np.uint32)), j
        assert idx is None or np.array_equal(gi, idx), j


def test_faults_stay_with_their_node(dev):
    """Rejection of malformed input whose outcome is fixed on the CPU: nothing here reads or
    writes outside a slot."""
    from decentralizepy_amd import codec
    idx, si, sv, vals = catalog(0)[14]                       # k = 2049, log-uniform gaps
    k = idx.size
    long_bits = si.copy()
    long_bits[-8:] = np.frombuffer(np.int64(8 * (si.size - 16) + 128 + 8).tobytes(), np.uint8)
    magic = sv.copy()
    magic[0] ^= 1
    short = oelias.encode(idx[:-1])                          # a valid stream of k - 1 indices
    nodes = [(idx, si, sv, vals), (idx, long_bits, sv, vals), (idx, si, magic, vals),
             (idx, short, sv, vals), (idx, si, sv, vals)]
    cap = -(-si.size // 4) * 4
    sizes = [[cap + 4, sv.size]] + [[n[1].size, n[2].size] for n in nodes[1:]]
    status, res = decode_nodes(dev, codec, nodes, 0, sizes=sizes, counts=[k] * 5)
    assert status.tolist() == [1, 1, 4, 2, 0]
    assert all(r[2] for r in res)
    assert np.array_equal(res[4][0], idx)
    assert np.array_equal(res[4][1].view(np.uint32), vals.view(np.uint32))
    for j in (0, 1, 3):  # a refused index stream writes no index; its values are independent
        assert (res[j][0] == GUARD).all(), j
        assert np.array_equal(res[j][1].view(np.uint32), vals.view(np.uint32)), j
    assert np.array_equal(res[2][0], idx)


@pytest.fixture(params=["in_place", "rccl"])
def group(request, dev):
    if request.param == "in_place":
        yield None
    else:
        with rccl_loopback(dev) as g:
            yield g


@pytest.mark.parametrize("precision", [0, 16])
@pytest.mark.parametrize("mode", ["acc", "avg"])
def test_coded_exchange_equals_the_round_on_truncated_values(dev, group, mode, precision):
    from decentralizepy_amd.compression.EliasFpzipLossy import EliasFpzipLossy
    from decentralizepy_amd.gossip_topkacc import TopKAccRound
    from tests import topkacc_round_ops as ops
    meta, arr = run_named(f"{mode}_irr6")
    assert meta["n"] == 4100

    def engine(**kw):
        return TopKAccRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]).to(dev),
                            meta["alpha"], accumulate_averaging_changes=meta["avg"], group=group,
                            **kw)

    coded, plain = engine(coded_exchange=True, float_precision=precision), engine()
    lo = plain.cap + 4  # the rows' value words

    def truncate(leg):  # finite models: the top 16 bits are a plain bit mask
        if leg == "exchange" and precision:
            plain.rows[:, lo:] &= -(1 << (32 - precision))

    comp = EliasFpzipLossy()
    gen = torch.Generator().manual_seed(5)
    for r in range(3):
        noise = (0.01 * torch.randn(6, meta["n"], generator=gen)).to(dev)
        for e in (coded, plain):
            e.x.add_(noise)
        coded.step()
        plain.step(mark=truncate)
        for name in ("x", "acc", "counter"):
            assert torch.equal(getattr(coded, name), getattr(plain, name)), (r, name)
        sizes = coded.wire_bytes().cpu().numpy()
        for q in range(6):
            msg = coded.wire_payload(q)
            assert sizes[q].tolist() == [msg["indices"].size, msg["params"].size]
            idx, vals = (t.cpu().numpy() for t in coded.payload(q))
            assert np.array_equal(comp.decompress(msg["indices"]), idx)
            assert np.array_equal(np.atleast_1d(comp.decompress_float(msg["params"])).view(
                np.uint32), vals.view(np.uint32))
            assert np.array_equal(coded.send[q, 4:4 + coded.k].cpu().numpy(), idx)
        assert not coded.guard.any()
