"""GPU: the dense multi-node fold (``dpz_dense_average_nodes``, csrc/dpz_dense.hip) against the
single-node dense ``codec.decode_average`` and the numpy restatement (tests/epidemic_ops.py), bit
for bit on the staged and the direct path, and the engines of decentralizepy_amd/gossip_epidemic.py
against the runs recorded from the unmodified reference (tests/golden/epidemic.json).  Sizes: one
element, less than and exactly one 16-byte column, the tile's edges, several tiles with a ragged
tail; 2, 16 and 17 source rows (one tile width each side of the 1024 / 512 step)."""
import numpy as np
import pytest
import torch

from tests import epidemic_ops as ops
from tests.dist_harness import rccl_loopback
from tests.test_cpu_epidemic_round import EL_RUNS, make_engine, run_and_check

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
TINY_W = 2.5e-9  # times a 1e-30 element: a subnormal product


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def sources(n_src, n, seed=11):
    """Rows with -0.0, mixed magnitudes, and columns where every row is around 1e-37: each
    weighted product there is subnormal (or underflows under TINY_W), and so is the sum."""
    x = np.random.default_rng(seed).standard_normal((n_src, n)).astype(np.float32)
    flat = x.reshape(-1)
    flat[3::11] *= np.float32(1e-30)
    x[:, 2::17] *= np.float32(1e-37)
    flat[::7] = -0.0
    return x


def receivers(n_src):
    """(own row, w_self, [(source, weight)]) with list lengths 0, 1, n_src - 1 and one list that
    repeats a source; every weight differs."""
    def weights(k, off):
        return [TINY_W if p == 1 else 1.0 / (p + 3 + off) for p in range(k)]

    others = [s for s in range(n_src) if s != 1][::-1]  # n_src - 1 rows, not ascending
    rep = [0, n_src - 1, 0, 0]
    lists = [[], [n_src - 1], others, rep]
    return [(j % n_src, 0.5 / (j + 1), list(zip(lst, weights(len(lst), j))))
            for j, lst in enumerate(lists)]


def layout(dev, x, n_recv, aligned):
    """Device rows of the sources and prefilled output rows wider than n: 16-byte aligned rows,
    or packed rows (unaligned whenever n % 4 != 0)."""
    n_src, n = x.shape
    if aligned:
        s_stride = o_stride = -(-n // 4) * 4 + 4
    else:
        s_stride, o_stride = n, n + 5 + ((n + 5) % 4 == 0)  # the out rows never aligned
    src = torch.zeros(n_src, s_stride, dtype=torch.float32, device=dev)
    src[:, :n] = torch.from_numpy(x).to(dev)
    out = torch.full((n_recv, o_stride), FILL, dtype=torch.int32, device=dev).view(torch.float32)
    return src, out


def expected(dev, x, src, recvs):
    """Per receiver: the numpy restatement, checked against the single-node dense fold."""
    from decentralizepy_amd import codec
    n = x.shape[1]
    want = []
    ws = codec.Workspace(dev)
    for own, w_self, pairs in recvs:
        ref = ops.fold(x[own], [x[s] for s, _ in pairs], [w for _, w in pairs], w_self)
        if pairs:
            one = codec.decode_average(src[own, :n], [(None, src[s, :n]) for s, _ in pairs],
                                       [w for _, w in pairs], w_self, workspace=ws)
            np.testing.assert_array_equal(_u32(one), ref.view(np.uint32))
        else:
            np.testing.assert_array_equal(ref.view(np.uint32), x[own].view(np.uint32))
        want.append(ref)
    return np.stack(want)


def run_modes(dev, x, recvs, aligned, modes):
    from decentralizepy_amd import codec
    n = x.shape[1]
    src, out = layout(dev, x, len(recvs), aligned)
    if aligned:
        assert all(src[s].data_ptr() % 16 == 0 for s in range(len(x)))
    else:
        assert out[1].data_ptr() % 16 and (n % 4 == 0 or src[1].data_ptr() % 16)
    want = expected(dev, x, src, recvs)
    for mode in modes:
        out.view(torch.int32).fill_(FILL)
        tab = codec.DenseTable([src[s, :n] for s in range(len(x))],
                               [(out[j], own, w_self, pairs)
                                for j, (own, w_self, pairs) in enumerate(recvs)], dev)
        codec.dense_average_nodes(tab, n, mode)
        err = str((len(x), n, aligned, mode))
        np.testing.assert_array_equal(_u32(out[:, :n]), want.view(np.uint32), err_msg=err)
        assert (_u32(out[:, n:]) == FILL).all(), err  # the padding came back untouched
    return want


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "packed"])
@pytest.mark.parametrize("n_src", [2, 16, 17])
def test_kernel_equals_the_single_node_dense_fold(dev, n_src, aligned):
    from decentralizepy_amd import _lib, codec
    T = codec.dense_tile_elems(n_src)
    assert T == (1024 if n_src <= 16 else 512)
    recvs = receivers(n_src)
    assert [len(r[2]) for r in recvs] == [0, 1, n_src - 1, 4]
    sub = 0
    for n in (1, 3, 4, T - 1, T, T + 1, 3 * T + 37):
        x = sources(n_src, n, seed=n_src + n)
        want = run_modes(dev, x, recvs, aligned,
                         (_lib.DPZ_DENSE_STAGED, _lib.DPZ_DENSE_DIRECT, _lib.DPZ_DENSE_AUTO))
        tiny = np.finfo(np.float32).tiny
        sub += int(((np.abs(want) < tiny) & (want != 0)).sum())
        assert n < 8 or np.signbit(want[0][want[0] == 0]).any()  # a -0.0 copied as it is
    assert sub  # subnormal results occurred: nothing flushed them on either side


def test_more_sources_than_the_staged_path_fits(dev):
    from decentralizepy_amd import _lib, codec
    n_src, n = 65, 1029
    assert codec.dense_tile_elems(n_src) == 0
    x = sources(n_src, n)
    recvs = receivers(n_src)
    src, out = layout(dev, x, len(recvs), True)
    tab = codec.DenseTable(src[:, :n].unbind(0), [(out[j], own, w_self, pairs)
                                                   for j, (own, w_self, pairs) in enumerate(recvs)],
                           dev)
    rc = codec.dense_average_nodes(tab, n, _lib.DPZ_DENSE_STAGED, check_rc=False)
    assert rc == _lib.DPZ_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (_u32(out) == FILL).all()  # nothing was launched
    # auto has only the direct path left, and it matches the single-node fold and numpy
    run_modes(dev, x, recvs, True, (_lib.DPZ_DENSE_AUTO, _lib.DPZ_DENSE_DIRECT))
    run_modes(dev, x, recvs, False, (_lib.DPZ_DENSE_AUTO,))


def test_auto_at_a_size_where_it_stages(dev):
    """The EL round's lists (16 receivers, round 0 of the degree-7 run) over 384 tiles and a
    ragged tail: auto takes the staged path there, and every mode gives the numpy result."""
    from decentralizepy_amd import _lib, codec
    meta, _ = ops.load("el_d7")
    adj = ops.graph(meta)
    lists = ops.receive_lists(adj, [set(s) for s in meta["rounds"][0]["send_sets"]])
    n_src, n = 16, 383 * 1024 + 5
    reads = sum(len(got) + 1 for got in lists)
    assert codec.dense_auto_mode(n_src, reads, n) == _lib.DPZ_DENSE_STAGED
    assert codec.dense_auto_mode(n_src, reads, n - 5) == _lib.DPZ_DENSE_DIRECT
    x = sources(n_src, n)
    src, out = layout(dev, x, n_src, True)
    recvs = [(i, 1 / (len(got) + 1), [(j, 1 / (len(got) + 1)) for j in got])
             for i, got in enumerate(lists)]
    want = np.stack([ops.fold(x[i], [x[j] for j, _ in pairs], [w for _, w in pairs], ws)
                     for i, ws, pairs in recvs])
    tab = codec.DenseTable(src[:, :n].unbind(0),
                           [(out[j], own, ws, pairs) for j, (own, ws, pairs) in enumerate(recvs)],
                           dev)
    for mode in (_lib.DPZ_DENSE_AUTO, _lib.DPZ_DENSE_STAGED, _lib.DPZ_DENSE_DIRECT):
        out.view(torch.int32).fill_(FILL)
        codec.dense_average_nodes(tab, n, mode)
        np.testing.assert_array_equal(_u32(out[:, :n]), want.view(np.uint32), err_msg=str(mode))
        assert (_u32(out[:, n:]) == FILL).all()


def test_argument_errors_launch_nothing(dev):
    from decentralizepy_amd import _lib, codec
    n_src, n = 4, 1000
    x = sources(n_src, n)
    src, out = layout(dev, x, 2, True)
    before = _u32(src).copy()
    rows = [src[s, :n] for s in range(n_src)]
    ok = [(1, 0.5), (2, 0.25)]
    cases = {
        "out is a source row": [(src[3], 0, 0.5, ok), (out[1], 1, 0.5, ok)],
        "out overlaps a source row": [(out[0], 0, 0.5, ok), (src[2, 8:], 1, 0.5, ok)],
        "a list index past the sources": [(out[0], 0, 0.5, [(1, 0.5), (n_src, 0.25)])],
        "a negative list index": [(out[0], 0, 0.5, [(-1, 0.5)])],
        "an own row past the sources": [(out[0], n_src, 0.5, ok)],
    }
    for what, recvs in cases.items():
        tab = codec.DenseTable(rows, recvs, dev)
        for mode in (0, 1, 2):
            assert codec.dense_average_nodes(tab, n, mode, check_rc=False) == _lib.DPZ_ERR_ARG, what
    with pytest.raises(_lib.CodecError):
        codec.dense_average_nodes(codec.DenseTable(rows, cases["a negative list index"], dev), n)
    torch.cuda.synchronize()
    assert (_u32(out) == FILL).all() and np.array_equal(_u32(src), before)


# ---- the engines ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EL_RUNS + ["fullshare6"])
def test_engine_reproduces_the_reference(dev, name):
    meta, last = ops.load(name)
    eng = make_engine(meta, device=dev)
    assert eng.x.is_cuda and eng.x[1].data_ptr() % 16 == 0 and meta["n"] % 4  # padded stride
    run_and_check(eng, meta, last)


@pytest.mark.parametrize("mode", [1, 2])
def test_engine_on_a_forced_path(dev, mode):
    meta, last = ops.load("el_d7")
    run_and_check(make_engine(meta, device=dev, mode=mode), meta, last)


@pytest.fixture(scope="module")
def regular96():
    import os
    from decentralizepy_amd.gossip import read_edges
    adj = read_edges(os.path.join(ops.GOLDEN, "96_regular.edges"))
    n = 4001
    x = np.stack([ops.recipe(500 + u, n) for u in range(96)])
    ref = ops.NumpyRound(adj, x)
    want = []
    for _ in range(2):
        ref.step()
        want.append(ref.x.copy())
    return adj, x, want


def test_full_share_over_96_nodes_takes_the_direct_path(dev, regular96):
    from decentralizepy_amd import codec
    from decentralizepy_amd.gossip_epidemic import FullShareRound
    adj, x, want = regular96
    assert len(adj) == 96 and codec.dense_tile_elems(96) == 0  # auto: only the direct path
    eng = FullShareRound(adj, torch.from_numpy(x).to(dev))
    for ref in want:
        eng.step()
        np.testing.assert_array_equal(_u32(eng.x), ref.view(np.uint32))
    assert len(eng._tabs) == 2  # a static topology: one table per buffer order, built once


def test_senders_override_on_the_device(dev):
    from decentralizepy_amd.gossip_epidemic import EpidemicRound
    from tests.test_cpu_epidemic_round import (_ring_adj, _ring_models, _ring_reference,
                                               _ring_senders)
    eng = EpidemicRound(_ring_adj(), torch.from_numpy(_ring_models()).to(dev), 1, 0,
                        senders=_ring_senders)
    for ref in _ring_reference():
        eng.step()
        np.testing.assert_array_equal(_u32(eng.x), ref.view(np.uint32))


@pytest.fixture
def rccl_group(dev):
    with rccl_loopback(dev) as group:
        yield group


def test_engines_through_rccl_equal_in_place(dev, rccl_group):
    for name in ("el_d7", "fullshare6"):
        meta, last = ops.load(name)
        eng = make_engine(meta, device=dev, group=rccl_group)
        assert eng.coll and eng.recv is not None and eng.recv.shape[0] == meta["nodes"]
        run_and_check(eng, meta, last)
