"""GPU: the batched quantiser (``dpz_quant_encode_nodes``, csrc/dpz_quant_nodes.hip) against the
single call, the fused unpack-and-fold (``dpz_qdense_average_nodes``, csrc/dpz_qdense.hip) against
``quant_decode`` + ``dense_average_nodes`` and the numpy restatements, and the engines of
decentralizepy_amd/gossip_quant.py against the runs recorded from the unmodified reference
(tests/golden/quant_round.json) — everything bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import quant_round_ops as ops
from tests import quantization_ops as qops
from tests.dist_harness import rccl_loopback
from tests.test_cpu_quant_round import make_engine, run_and_check, wide_field_model
from tests.test_gpu_epidemic_round import receivers, sources

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
INFO, BODY = 4, 12
ULP = 2.0 ** -149


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


# ---- the batched encode -----------------------------------------------------------------------
ENC_NS = [1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 3 * 8192 + 4099]


def encode_inputs(m, n, k, slot):
    """m rows of n values: mixed scales and, from five rows on, one row per status: all zero
    (1), a NaN (2), max|x| / k underflowing (3, for k > 1) and multiples of the smallest
    subnormal whose field is one bit wider than k's (for k <= 2^22: 4 at the default slot
    wherever the wider body needs another dword)."""
    x = np.stack([qops.recipe(100 * n + j + k % 97, n, 10.0 ** (j % 5 - 3)) for j in range(m)])
    want = [0] * m
    if m >= 5:
        x[1] = 0
        x[2, n // 2] = np.nan
        x[3] = np.float32(ULP)
        x[3, ::2] *= -1
        want[1:4] = [1, 2, 3 if k > 1 else 0]
        if 1 < k <= 2 ** 22:
            v = np.arange(n, dtype=np.float64) % 7 - 3
            v[n - 1] = int(1.4 * k)
            x[4] = (v * ULP).astype(np.float32)
            w = int(1.4 * k).bit_length() + 1
            assert w == slot + 1
            want[4] = 4 if (n * w + 31) // 32 > (n * slot + 31) // 32 else 0
    return x, want


@pytest.mark.parametrize("m", [1, 3, 13])
@pytest.mark.parametrize("k", [1, 255, 32767, 2 ** 30 - 1])
def test_batched_encode_equals_the_single_call(dev, k, m):
    from decentralizepy_amd import _lib, codec
    from decentralizepy_amd.gossip_quant import default_slot_bits
    L = _lib.lib()
    assert codec.quant_block_elems() == 8192  # ENC_NS are its edges and the chunk's
    ws = None
    for n in ENC_NS:
        x, want = encode_inputs(m, n, k, default_slot_bits(k))
        for aligned in (True, False):
            for slot in sorted({default_slot_bits(k), max(2, default_slot_bits(k) - 3)}):
                cap = (n * slot + 31) // 32
                words = codec.quant_row_words(n, slot)
                assert words == BODY + cap
                # rows 16-byte aligned, or x and the packed rows at a 4-byte-only alignment
                xs, rs = (-(-n // 4) * 4, -(-(words + 3) // 4) * 4) if aligned else \
                    (n + 1 + (n + 1) % 2, words + 3 + (words + 3) % 2 + 1)
                xbuf = torch.zeros(m * xs + 1, dtype=torch.float32, device=dev)
                off = 0 if aligned else 1
                xt = xbuf[off:off + m * xs].view(m, xs)[:, :n]
                xt.copy_(torch.from_numpy(x))
                rbuf = torch.full((m * rs + 1,), FILL, dtype=torch.int32, device=dev)
                rows = rbuf[off:off + m * rs].view(m, rs)
                if aligned:
                    assert xt[m - 1].data_ptr() % 16 == 0 and rows[m - 1].data_ptr() % 16 == 0
                else:
                    assert xt[0].data_ptr() % 16 == 4 and rows[0].data_ptr() % 16 == 4
                    assert all(xt[j].data_ptr() % 8 == 4 for j in range(m))
                tab = codec.quant_node_table(xt, rows)
                ws = codec.quant_encode_nodes(tab, n, k, slot, ws)
                # the single call per row, same capacity, into prefilled buffers
                one_ws = torch.empty(max(256, int(L.dpz_quant_workspace_bytes(n))),
                                     dtype=torch.uint8, device=dev)
                body = torch.full((m, cap), FILL, dtype=torch.int32, device=dev)
                info = torch.full((m, 8), FILL, dtype=torch.int32, device=dev)
                for j in range(m):
                    rc = L.dpz_quant_encode(_ptr(xt[j]), n, k, _ptr(body[j]), 4 * cap,
                                            _ptr(info[j]), _ptr(one_ws), one_ws.numel(), None)
                    assert rc == 0
                got, inf, bod = _u32(rows), _u32(info), _u32(body)
                err = str((k, m, n, aligned, slot))
                np.testing.assert_array_equal(got[:, INFO:BODY], inf, err_msg=err)
                np.testing.assert_array_equal(got[:, BODY:BODY + cap], bod, err_msg=err)
                assert (got[:, BODY + cap:] == FILL).all(), err  # nothing past the slot
                assert (got[:, 0] == n).all() and (got[:, 1] == 0).all(), err
                np.testing.assert_array_equal(got[:, 2], inf[:, 0], err_msg=err)
                assert (got[:, 3] == 0).all(), err
                status = inf[:, 0].astype(np.int64)
                for j in np.flatnonzero(status):  # a row that was not quantised: body untouched
                    assert (got[j, BODY:] == FILL).all(), (err, j)
                ndw = (n * inf[:, 1].astype(np.int64) + 31) // 32
                for j in np.flatnonzero(status == 0):  # and nothing past a row's own body
                    assert (got[j, BODY + ndw[j]:] == FILL).all(), (err, j)
                if slot == default_slot_bits(k):
                    assert status.tolist() == want, (err, status)
                    j = m - 1  # against the restatement: the body and the scale
                    scale, to_send = qops.encode(x[j], k)
                    assert inf[j, 3] == qops.bits_of(scale) and inf[j, 1] == to_send[1], err
                    nb = to_send.size - 2
                    np.testing.assert_array_equal(got[j, BODY:].view(np.uint8)[:nb], to_send[2:])
                elif n * (default_slot_bits(k) - slot) >= 32 and m < 5:
                    assert (status == 4).all(), (err, status)  # the narrow slot holds no row


# ---- the fused fold -----------------------------------------------------------------------------
KS = [255, 1, 7, 32767, 2 ** 20, 2 ** 23, 2 ** 24, 2 ** 30]
WIDTHS = {2, 4, 9, 16, 22, 25, 26, 32}


def packed_sources(n_src, n, seed):
    """Per source (scale, to_send, decoded values) from the numpy quantiser: source s encoded
    with KS[s % 8] (widths 9, 2, 4, 16, 22, 25, 26 and 32: the fp32 / fp64 border from both
    sides; k = 2^24 gives 26), the first and the last from the "tiny" recipe (max|x| ~ 1e-38:
    subnormal scales and products) with k = 255 and 7."""
    out = []
    for s in range(n_src):
        if s in (0, n_src - 1):
            k = 255 if s == 0 else 7
            x = qops.case_input(dict(kind="tiny", seed=seed + s, n=n))
            x[0] = np.float32(1e-38)  # never all zero
        else:
            k = KS[s % 8]
            x = qops.recipe(seed + s, n, 0.3)
            x[0] = 2.0  # max|x| a power of two: norm = 2 / k and qmax = k exactly for k = 2^j
        scale, to_send = qops.encode(x, k)
        out.append((scale, to_send, qops.decode(scale, to_send)))
    return out


def pack_rows(dev, pays, n, aligned):
    """The packed rows of wire values on the device: (rows, cap); 16-byte aligned, or at a
    4-byte-only alignment."""
    cap = max((n * int(t[1]) + 31) // 32 for _, t, _ in pays)
    stride = -(-(BODY + cap) // 4) * 4 + (0 if aligned else 1)
    host = np.full((len(pays), stride), FILL, dtype=np.uint32)
    for s, (scale, to_send, _) in enumerate(pays):
        host[s, :BODY] = 0
        host[s, 0] = n
        host[s, INFO + 1], host[s, INFO + 2] = int(to_send[1]), int(to_send[0])
        host[s, INFO + 3] = qops.bits_of(scale)
        nb = to_send.size - 2
        ndw = (nb + 3) // 4
        host[s, BODY:BODY + ndw] = 0
        host[s, BODY:].view(np.uint8)[:nb] = to_send[2:]
    buf = torch.zeros(host.size + 1, dtype=torch.int32, device=dev)
    off = 0 if aligned else 1
    rows = buf[off:off + host.size].view(len(pays), stride)
    rows.copy_(torch.from_numpy(host.view(np.int32)))
    assert (rows[len(pays) - 1] if aligned else rows[0]).data_ptr() % 16 == 4 * off
    return rows, cap


def fp32_rows(dev, x, aligned, fill=None):
    """Device rows of x wider than n: 16-byte aligned, or never aligned."""
    m, n = x.shape
    stride = -(-n // 4) * 4 + 4 if aligned else n + 5 + ((n + 5) % 4 == 0)
    t = torch.full((m, stride), FILL, dtype=torch.int32, device=dev).view(torch.float32)
    if fill is None:
        t[:, :n] = torch.from_numpy(x).to(dev)
    return t


def device_reference(dev, pays, own, recvs, n):
    """quant_decode of every source + dense_average_nodes: the composed sequence."""
    from decentralizepy_amd import _lib, codec
    dec = []
    for scale, to_send, want in pays:
        body = np.zeros((to_send.size - 2 + 3) // 4 * 4, np.uint8)
        body[:to_send.size - 2] = to_send[2:]
        d = codec.quant_decode(torch.from_numpy(body).to(dev), n, int(to_send[1]), scale)
        np.testing.assert_array_equal(_u32(d), want.view(np.uint32))
        dec.append(d)
    n_src = len(pays)
    srcs = dec + [own[j, :n] for j in range(len(recvs))]
    out = torch.zeros(len(recvs), -(-n // 4) * 4, dtype=torch.float32, device=dev)
    tab = codec.DenseTable(srcs, [(out[j], n_src + j, w_self, pairs)
                                  for j, (_, w_self, pairs) in enumerate(recvs)], dev)
    codec.dense_average_nodes(tab, n, _lib.DPZ_DENSE_DIRECT)
    return out[:, :n].cpu().numpy()


def run_fold(dev, n_src, n, aligned, modes, seed=0):
    from decentralizepy_amd import codec
    pays = packed_sources(n_src, n, seed + 1000 * n_src + n)
    recvs = receivers(n_src)
    own_np = sources(len(recvs), n, seed=seed + n_src + n)
    rows, cap = pack_rows(dev, pays, n, aligned)
    own = fp32_rows(dev, own_np, aligned)
    out = fp32_rows(dev, own_np, aligned, fill=True)
    want = np.stack([ops.eops.fold(own_np[j], [pays[s][2] for s, _ in pairs],
                                   [w for _, w in pairs], w_self)
                     for j, (_, w_self, pairs) in enumerate(recvs)])
    np.testing.assert_array_equal(device_reference(dev, pays, own, recvs, n).view(np.uint32),
                                  want.view(np.uint32))
    tab = codec.QDenseTable([rows[s] for s in range(n_src)],
                            [(out[j], own[j], w_self, pairs)
                             for j, (_, w_self, pairs) in enumerate(recvs)], dev)
    guard = torch.zeros(n_src, dtype=torch.int32, device=dev)
    tripped = guard.clone()
    tripped[n_src - 1] = 3
    rows_before = _u32(rows).copy()
    for mode in modes:
        err = str((n_src, n, aligned, mode))
        for g in (None, guard):
            out.view(torch.int32).fill_(FILL)
            codec.qdense_average_nodes(tab, n, cap, mode, guard=g)
            np.testing.assert_array_equal(_u32(out[:, :n]), want.view(np.uint32), err_msg=err)
            assert (_u32(out[:, n:]) == FILL).all(), err  # the padding came back untouched
        out.view(torch.int32).fill_(FILL)
        codec.qdense_average_nodes(tab, n, cap, mode, guard=tripped)
        np.testing.assert_array_equal(_u32(out[:, :n]), own_np.view(np.uint32), err_msg=err)
        assert (_u32(out[:, n:]) == FILL).all(), err
    assert np.array_equal(_u32(rows), rows_before) and np.array_equal(
        _u32(own[:, :n]), own_np.view(np.uint32))
    return pays, want, own_np


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "packed"])
@pytest.mark.parametrize("n_src", [2, 16, 17])
def test_fused_fold_equals_decode_then_dense_fold(dev, n_src, aligned):
    from decentralizepy_amd import _lib, codec
    T = codec.qdense_tile_elems(n_src)
    assert T == (1024 if n_src <= 16 else 512) and T % 32 == 0
    sub, widths = 0, set()
    for n in (1, 3, 4, 31, 32, 33, T - 1, T, T + 1, 3 * T + 37):
        pays, want, own_np = run_fold(
            dev, n_src, n, aligned,
            (_lib.DPZ_DENSE_STAGED, _lib.DPZ_DENSE_DIRECT, _lib.DPZ_DENSE_AUTO))
        widths |= {int(t[1]) for _, t, _ in pays}
        tiny = np.finfo(np.float32).tiny
        sub += int(((np.abs(want) < tiny) & (want != 0)).sum())
        # receiver 0 has an empty list: its -0.0 values are copied as they are
        assert n < 8 or np.signbit(want[0][want[0] == 0]).any()
        assert any(np.abs(d).max() < tiny for _, _, d in pays)  # whole sources are subnormal
    assert sub  # subnormal results occurred: nothing flushed them on either side
    assert widths >= (WIDTHS if n_src >= 16 else {9, 4})


def test_more_sources_than_the_staged_path_fits(dev):
    from decentralizepy_amd import _lib, codec
    n_src, n = 65, 1029
    assert codec.qdense_tile_elems(n_src) == 0
    pays = packed_sources(n_src, n, 5)
    recvs = receivers(n_src)
    own_np = sources(len(recvs), n)
    rows, cap = pack_rows(dev, pays, n, True)
    own, out = fp32_rows(dev, own_np, True), fp32_rows(dev, own_np, True, fill=True)
    tab = codec.QDenseTable(rows, [(out[j], own[j], w_self, pairs)
                                   for j, (_, w_self, pairs) in enumerate(recvs)], dev)
    rc = codec.qdense_average_nodes(tab, n, cap, _lib.DPZ_DENSE_STAGED, check_rc=False)
    assert rc == _lib.DPZ_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (_u32(out) == FILL).all()  # nothing was launched
    # auto has only the direct path left, and it matches decode + dense fold and numpy
    run_fold(dev, n_src, n, True, (_lib.DPZ_DENSE_AUTO, _lib.DPZ_DENSE_DIRECT))
    run_fold(dev, n_src, n, False, (_lib.DPZ_DENSE_AUTO,))


def test_auto_at_a_size_where_it_stages(dev):
    """16 sources of 7 senders per receiver over 384 tiles and a ragged tail: auto takes the
    staged path there, and every mode gives the numpy result."""
    from decentralizepy_amd import _lib, codec
    n_src, n = 16, 383 * 1024 + 5
    lists = [[(i + d) % n_src for d in range(1, 8)] for i in range(n_src)]
    reads = sum(len(got) + 1 for got in lists)
    assert codec.qdense_auto_mode(n_src, reads, n) == _lib.DPZ_DENSE_STAGED
    assert codec.qdense_auto_mode(n_src, reads, n - 5) == _lib.DPZ_DENSE_DIRECT
    x = np.stack([qops.recipe(40 + s, n, 0.1) for s in range(n_src)])
    base = []
    for s in range(4):  # four distinct streams (w = 16 and 8) shared by the 16 rows
        scale, to_send = qops.encode(x[s], (32767, 127)[s % 2])
        base.append((scale, to_send, qops.decode(scale, to_send)))
    pays = [base[s % 4] for s in range(n_src)]
    rows, cap = pack_rows(dev, pays, n, True)
    own, out = fp32_rows(dev, x, True), fp32_rows(dev, x, True, fill=True)
    want = np.stack([ops.eops.fold(x[i], [pays[j][2] for j in got], [0.125] * 7, 0.125)
                     for i, got in enumerate(lists)])
    tab = codec.QDenseTable(rows, [(out[i], own[i], 0.125, [(j, 0.125) for j in got])
                                   for i, got in enumerate(lists)], dev)
    for mode in (_lib.DPZ_DENSE_AUTO, _lib.DPZ_DENSE_STAGED, _lib.DPZ_DENSE_DIRECT):
        out.view(torch.int32).fill_(FILL)
        codec.qdense_average_nodes(tab, n, cap, mode)
        np.testing.assert_array_equal(_u32(out[:, :n]), want.view(np.uint32), err_msg=str(mode))
        assert (_u32(out[:, n:]) == FILL).all()


@pytest.mark.parametrize("name", ["sharing_quant_small", "sharing_quant", "plain_quant"])
def test_fold_of_the_recorded_plugin_wire(dev, name):
    """The neighbours' recorded wire of the per-node plugin fixtures as sources, the recorded
    weights: out is the reference node's model after round 0."""
    from decentralizepy_amd import _lib, codec
    sc, arrays = qops.load_plugin(name)
    n, nb = sc["n"], len(sc["neighbours"])
    pays = [(arrays[f"r0_nbr{j}_scale"][0], arrays[f"r0_nbr{j}_to_send"], None)
            for j in range(nb)]
    if sc["degree"]:  # Sharing._averaging: Metro-Hastings from the neighbours' degrees
        w = [1 / (max(nb, v["degree"]) + 1) for v in sc["neighbours"]]
        total = 0
        for v in w:
            total += v
        w_self = 1 - total
    else:  # PlainAverageSharing._averaging
        w = [1 / (nb + 1)] * nb
        w_self = w[0]
    rows, cap = pack_rows(dev, pays, n, True)
    x = arrays["r0_x"][None, :]
    own, out = fp32_rows(dev, x, True), fp32_rows(dev, x, True, fill=True)
    tab = codec.QDenseTable(rows, [(out[0], own[0], w_self, list(zip(range(nb), w)))], dev)
    for mode in (_lib.DPZ_DENSE_STAGED, _lib.DPZ_DENSE_DIRECT, _lib.DPZ_DENSE_AUTO):
        out.view(torch.int32).fill_(FILL)
        codec.qdense_average_nodes(tab, n, cap, mode)
        np.testing.assert_array_equal(_u32(out[0, :n]),
                                      arrays["r0_model_after"].view(np.uint32))


def test_fold_argument_errors_launch_nothing(dev):
    from decentralizepy_amd import _lib, codec
    n_src, n = 4, 1000
    pays = packed_sources(n_src, n, 9)
    rows, cap = pack_rows(dev, pays, n, True)
    x = sources(2, n)
    own, out = fp32_rows(dev, x, True), fp32_rows(dev, x, True, fill=True)
    ok = [(1, 0.5), (2, 0.25)]
    cases = {
        "out is another's own row": [(own[1], own[0], 0.5, ok), (out[1], own[1], 0.5, ok)],
        "out is its own row": [(own[0], own[0], 0.5, ok)],
        "out lies in a packed row": [(rows[2, 4:].view(torch.float32), own[0], 0.5, ok)],
        "a list index past the sources": [(out[0], own[0], 0.5, [(1, 0.5), (n_src, 0.25)])],
        "a negative list index": [(out[0], own[0], 0.5, [(-1, 0.5)])],
        "two receivers share an out row": [(out[0], own[0], 0.5, ok), (out[0], own[1], 0.5, ok)],
    }
    before = _u32(rows).copy()
    for what, recvs in cases.items():
        tab = codec.QDenseTable(rows, recvs, dev)
        for mode in (0, 1, 2):
            rc = codec.qdense_average_nodes(tab, n, cap, mode, check_rc=False)
            assert rc == _lib.DPZ_ERR_ARG, what
    with pytest.raises(_lib.CodecError):
        codec.qdense_average_nodes(codec.QDenseTable(rows, cases["a negative list index"], dev),
                                   n, cap)
    torch.cuda.synchronize()
    assert (_u32(out) == FILL).all() and np.array_equal(_u32(rows), before)
    np.testing.assert_array_equal(_u32(own[:, :n]), x.view(np.uint32))


# ---- the engines ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", ops.RUNS)
def test_engine_reproduces_the_reference(dev, name, mode):
    meta, arrays = ops.load(name)
    eng = make_engine(meta, device=dev, mode=mode)
    assert eng.x.is_cuda and eng.x[1].data_ptr() % 16 == 0 and eng.send[1].data_ptr() % 16 == 0
    run_and_check(eng, meta, arrays)
    assert len(eng._enc_tabs) == 2  # one node table per buffer order, built once


@pytest.fixture
def rccl_group(dev):
    with rccl_loopback(dev) as group:
        yield group


def test_engines_through_rccl_equal_in_place(dev, rccl_group):
    for name in ops.RUNS:
        meta, arrays = ops.load(name)
        eng = make_engine(meta, device=dev, group=rccl_group)
        assert eng.coll and eng.recv.shape == (meta["nodes"], eng.row_words)
        run_and_check(eng, meta, arrays)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("what", ["zero", "nan", "wide"])
def test_a_round_that_cannot_be_quantised_changes_no_model(dev, what, mode):
    from decentralizepy_amd.gossip_quant import QuantFullShareRound
    meta, _ = ops.load("fullshare6_q255")
    x = ops.initial_models(meta)
    bad = {"zero": [2], "nan": [4], "wide": [0, 5]}[what]
    for q in bad:
        if what == "zero":
            x[q] = 0
        elif what == "nan":
            x[q, 1000] = np.nan
        else:
            x[q] = wide_field_model(meta["n"])
    eng = QuantFullShareRound(ops.graph(meta), torch.from_numpy(x).to(dev), 255, mode=mode)
    before = eng.x.data_ptr()
    eng.step()
    assert eng.x.data_ptr() != before  # the buffers swapped all the same
    np.testing.assert_array_equal(_u32(eng.x), x.view(np.uint32))
    reason = {"zero": "all-zero", "nan": "non-finite", "wide": "wider than the slot"}[what]
    with pytest.raises(RuntimeError, match=rf"nodes \[{', '.join(map(str, bad))}\].*{reason}"):
        eng.check()
    np.testing.assert_array_equal(_u32(eng.x), x.view(np.uint32))
    for q in bad:  # repaired between rounds through the writable view: the next round runs
        eng.x[q] = torch.from_numpy(ops.eops.recipe(77 + q, meta["n"])).to(dev)
    eng.step()
    eng.check()
    assert (_u32(eng.x) != x.view(np.uint32)).any()


@pytest.fixture(scope="module")
def regular96():
    from decentralizepy_amd.gossip import read_edges
    adj = read_edges(os.path.join(ops.GOLDEN, "96_regular.edges"))
    n = 4001
    x = np.stack([ops.eops.recipe(500 + u, n) for u in range(96)])
    ref = ops.NumpyQuantRound(adj, x, 32767)
    want, wire = [], None
    for _ in range(2):
        ref.step()
        wire = wire or ref.wire
        want.append(ref.x.copy())
    return adj, x, want, wire


def test_full_share_over_96_nodes(dev, regular96):
    from decentralizepy_amd import codec
    from decentralizepy_amd.gossip_quant import QuantFullShareRound
    adj, x, want, wire = regular96
    assert len(adj) == 96 and codec.qdense_tile_elems(96) == 0  # auto: only the direct path
    eng = QuantFullShareRound(adj, torch.from_numpy(x).to(dev))
    for r, ref in enumerate(want):
        eng.step()
        if r == 0:
            for q in (0, 50, 95):
                scale, to_send = eng.payload(q)
                assert qops.bits_of(scale) == qops.bits_of(wire[q][0])
                np.testing.assert_array_equal(to_send, wire[q][1])
        np.testing.assert_array_equal(_u32(eng.x), ref.view(np.uint32))
    eng.check()
    assert len(eng._tabs) == 2  # a static topology: one table per buffer order, built once
