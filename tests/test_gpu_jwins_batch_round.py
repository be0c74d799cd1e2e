"""GPU: the batched JWINS round.  ``dpz_dwt_sym2_nodes`` / ``dpz_idwt_sym2_nodes`` bit for bit
against the single-node calls at the tile edges of both transforms, ``dpz_jwins_encode_nodes``
against the numpy restatement (tests/jwins_round_ops.py) and the single-node
``codec.topk_encode`` on its exact path, and the engine
(decentralizepy_amd/gossip_jwins_batch.py) against the runs recorded from the unmodified
reference, against ``JwinsRound`` on the HIP ops and, on a star, against the oracle written out
node by node."""
import numpy as np
import pytest
import torch

from decentralizepy_amd.gossip_round import up4
from oracle import topk as otopk
from tests import jwins_round_ops as ops
from tests.dist_harness import rccl_loopback
from tests.jwins_ops import direct_round_nodes

RUNS = ops.load_runs()
RUN_IDS = [m["name"] for m, _ in RUNS]

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
PAD = 7.0
QUANT_P = np.array([0.07] + [0.86 / 9] * 9 + [0.07])


def _rows(dev, data, off, dtype=torch.float32, pad=PAD):
    """Device rows of the matrix ``data``, the words around them prefilled; every row ``off``
    words past a 16-byte boundary.  Returns (view, backing)."""
    m, n = data.shape
    back = torch.full((m, up4(n) + 8), pad, dtype=dtype, device=dev)
    view = back[:, off:off + n]
    view.copy_(torch.from_numpy(data).to(dev))
    assert all(view[j].data_ptr() % 16 == 4 * (off % 4) for j in range(m))
    return view, back


def _padding_intact(back, n, off, pad=PAD):
    return bool((back[:, :off] == pad).all() and (back[:, off + n:] == pad).all())


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


# ---- the transforms -------------------------------------------------------------------------------
def _min_n(codec, level):
    return next(n for n in range(1, 64) if codec._lib.lib().dpz_wavedec_len(n, level) > 0)


def _sizes(codec, level):
    T = int(codec._lib.lib().dpz_dwt_tile_width()) << level
    V = int(codec._lib.lib().dpz_idwt_tile_width())
    return [_min_n(codec, level), 100, 101, T - 1, T, T + 1, 3 * T + 37, V - 1, V + 1,
            2 * V + T + 5]


@pytest.mark.parametrize("level", [1, 2, 3, 4])
def test_transforms_of_nodes_equal_the_single_calls(dev, level):
    from decentralizepy_amd import codec
    assert _min_n(codec, 4) == 11
    sizes = _sizes(codec, level)
    assert sizes[6] % 2 == 1  # 3T + 37: the last output of an odd-length level
    for n in sizes:
        M = codec.wavedec_len(n, level)
        rng = np.random.default_rng([n, level])
        x = rng.standard_normal((3, n)).astype(np.float32)
        x0 = (x + 0.1 * rng.standard_normal((3, n))).astype(np.float32)
        acc = rng.standard_normal((3, M)).astype(np.float32)
        tx, bx = _rows(dev, x, 4)
        t0, b0 = _rows(dev, x0, 4)
        for m in (3, 1):
            err = str((n, level, m))
            # pair mode
            wx, bwx = _rows(dev, np.full((m, M), PAD, np.float32), 4)
            wc, bwc = _rows(dev, np.full((m, M), PAD, np.float32), 4)
            codec.dwt_sym2_nodes(codec.DwtNodesTable(tx[:m], t0[:m], wx, wc, dev), n, level)
            for j in range(m):
                sx, sc = codec.wavedec(tx[j].contiguous(), level, x0=t0[j].contiguous())
                assert np.array_equal(_bits(wx[j]), _bits(sx)), err
                assert np.array_equal(_bits(wc[j]), _bits(sc)), err
            # W(x) alone and W(x - x0) alone
            ox, box = _rows(dev, np.full((m, M), PAD, np.float32), 4)
            od, bod = _rows(dev, np.full((m, M), PAD, np.float32), 4)
            codec.dwt_sym2_nodes(codec.DwtNodesTable(tx[:m], None, ox, None, dev), n, level)
            codec.dwt_sym2_nodes(codec.DwtNodesTable(tx[:m], t0[:m], None, od, dev), n, level)
            assert np.array_equal(_bits(ox), _bits(wx)) and np.array_equal(_bits(od), _bits(wc))
            # accumulate mode
            ta, ba = _rows(dev, acc[:m], 4)
            codec.dwt_sym2_nodes(codec.DwtNodesTable(tx[:m], t0[:m], None, ta, dev), n, level,
                                 accumulate=True)
            for j in range(m):
                sa = torch.from_numpy(acc[j].copy()).to(dev)
                codec.wavedec(tx[j].contiguous(), level, x0=t0[j].contiguous(), want_x=False,
                              coeffs_diff=sa, accumulate=True)
                assert np.array_equal(_bits(ta[j]), _bits(sa)), err
            # the inverse, of the accumulators (arbitrary coefficients)
            out, bout = _rows(dev, np.full((m, n), PAD, np.float32), 4)
            codec.idwt_sym2_nodes(codec.IdwtNodesTable(ta, out, dev), n, level)
            for j in range(m):
                so = codec.waverec(ta[j].contiguous(), n, level)
                assert np.array_equal(_bits(out[j]), _bits(so)), err
            for back, ln in ((bx, n), (b0, n), (bwx, M), (bwc, M), (box, M), (bod, M), (ba, M),
                             (bout, n)):
                assert _padding_intact(back, ln, 4), err
            assert np.array_equal(_bits(tx), x.view(np.uint32))
            assert np.array_equal(_bits(t0), x0.view(np.uint32))


def test_transforms_of_nodes_refuse_bad_tables_before_writing(dev):
    from decentralizepy_amd import _lib, codec
    n, level = 101, 4
    M = codec.wavedec_len(n, level)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, n)).astype(np.float32)
    for col in range(4):  # a row 4 bytes off in x, x0, coeffs_x, coeffs_diff
        cols = [_rows(dev, x, 4)[0], _rows(dev, x, 4)[0],
                _rows(dev, np.full((3, M), PAD, np.float32), 4)[0],
                _rows(dev, np.full((3, M), PAD, np.float32), 4)[0]]
        backs = [torch.full((3, up4(M) + 8), PAD, device=dev) for _ in range(2)]
        if col >= 2:
            cols[col] = backs[col - 2][:, 5:5 + M]
        else:
            cols[col] = _rows(dev, x, 5)[0]
        tab = codec.DwtNodesTable(*cols, dev)
        assert codec.dwt_sym2_nodes(tab, n, level, check_rc=False) == _lib.DPZ_ERR_ARG
        torch.cuda.synchronize(dev)
        assert all((c == PAD).all() for c in cols[2:])  # nothing written
    # mixed output sets: node 2 without coeffs_x, then without coeffs_diff
    for word in (2, 3):
        wx = torch.full((3, up4(M)), PAD, device=dev)[:, :M]
        wc = torch.full((3, up4(M)), PAD, device=dev)[:, :M]
        tx, t0 = _rows(dev, x, 4)[0], _rows(dev, x, 4)[0]
        tab = codec.DwtNodesTable(tx, t0, wx, wc, dev)
        tab.host[4 * 2 + word] = 0
        tab._upload(dev)
        assert codec.dwt_sym2_nodes(tab, n, level, check_rc=False) == _lib.DPZ_ERR_ARG
        torch.cuda.synchronize(dev)
        assert (wx == PAD).all() and (wc == PAD).all()
    # the inverse: a misaligned coefficient row, a misaligned output row
    co = _rows(dev, rng.standard_normal((3, M)).astype(np.float32), 4)[0]
    for bad_out in (False, True):
        out, bout = _rows(dev, np.full((3, n), PAD, np.float32), 5 if bad_out else 4)
        src = co if bad_out else _rows(dev, rng.standard_normal((3, M)).astype(np.float32), 5)[0]
        tab = codec.IdwtNodesTable(src, out, dev)
        assert codec.idwt_sym2_nodes(tab, n, level, check_rc=False) == _lib.DPZ_ERR_ARG
        torch.cuda.synchronize(dev)
        assert (bout == PAD).all()
    with pytest.raises(_lib.CodecError):
        codec.idwt_sym2_nodes(codec.IdwtNodesTable(co, _rows(dev, x, 4)[0], dev), n, 5)


# ---- the selection --------------------------------------------------------------------------------
SIZES = ["1", "3", "4", "5", "1025", "C-1", "C", "C+1", "3*C+37"]


def _quant(rng, shape):
    return (rng.choice(np.arange(-5, 6), size=shape, p=QUANT_P) * np.float32(0.25)).astype(
        np.float32)


def _ks(n):
    """Five nodes: k = 1, round(0.1 n), n // 2 + 1, n and 0, as far as n allows."""
    return [1, max(1, round(0.1 * n)), min(n, n // 2 + 1), n, 0]


def _select_data(n, C, kind, seed):
    """5 nodes (c, acc, vals_src, counter).  kind "mixed": random rows, node 1 with 11 levels in c
    alone (acc = 0) and +-1.25 on the two sides of the first chunk edge, node 2 with 11 levels in
    both c and acc; kind "ties": every key equal and nonzero on the even nodes, every key zero on
    the odd ones."""
    rng = np.random.default_rng([seed, n])
    c = rng.standard_normal((5, n)).astype(np.float32)
    acc = (0.05 * rng.standard_normal((5, n))).astype(np.float32)
    if kind == "mixed":
        c[1], acc[1] = _quant(rng, n), 0.0
        if n > C:
            c[1, C - 1], c[1, C] = 1.25, -1.25
        c[2], acc[2] = _quant(rng, n), _quant(rng, n)
    else:
        c[0::2] = np.float32(0.5) * rng.choice([-1, 1], size=c[0::2].shape).astype(np.float32)
        acc[0::2] = np.where(c[0::2] > 0, np.float32(0.25), np.float32(-0.25))  # |c + acc| = 0.75
        c[1::2] = acc[1::2]
        acc[1::2] = -acc[1::2]  # c + acc = +0
    vals = rng.standard_normal((5, n)).astype(np.float32)
    counter = rng.integers(0, 5, size=(5, n)).astype(np.int32)
    return c, acc, vals, counter


def _run_select(dev, codec, c, acc, vals, counter, ks, aligned, with_counter, full_copy):
    """The kernel on device copies; returns the rows it left and the slot buffer's words, and
    checks vals_src and every word around the rows."""
    m, n = c.shape
    off = 4 if aligned else 5
    tc, bc = _rows(dev, c, off)
    ta, ba = _rows(dev, acc, off)
    tv, bv = _rows(dev, vals, off)
    tn, bn = _rows(dev, counter, off, torch.int32, 77)
    # slots: [5 words | idx slot | 5 words | val slot] per node, 4-byte aligned at odd words
    lens = [(up4(k), up4(k) if k else (up4(n) if full_copy else 0)) for k in ks]
    starts, pos = [], 0 if aligned else 1
    for li, lv in lens:
        starts.append((pos + 5, pos + 5 + li + 5))
        pos += 5 + li + 5 + lv
    slots = torch.from_numpy(np.full(pos + 5, FILL, dtype=np.uint32).view(np.int32)).to(dev)
    tab = codec.JwinsEncodeTable(tc, ta, tv, tn if with_counter else None, dev)
    base = slots.data_ptr()
    for j, k in enumerate(ks):
        si, sv = starts[j]
        if k:
            tab.set(j, k, base + 4 * si, base + 4 * sv)
        else:
            tab.set(j, 0, 0, base + 4 * sv if full_copy else None)
    codec.jwins_encode_nodes(tab.upload(), n)
    assert np.array_equal(_bits(tv), vals.view(np.uint32))
    for back, pad in ((bc, PAD), (ba, PAD), (bv, PAD), (bn, 77)):
        assert _padding_intact(back, n, off, pad)
    return (tc.cpu().numpy(), ta.cpu().numpy(), tn.cpu().numpy(), slots.cpu().numpy(), starts)


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset4"])
@pytest.mark.parametrize("which", SIZES)
def test_encode_nodes_equals_restatement_and_topk_encode(dev, which, aligned):
    from decentralizepy_amd import codec
    C = codec.jwins_chunk_elems()
    n = eval(which, {"C": C})
    ws = codec.Workspace(dev)
    ks = _ks(n)
    assert all(0 <= k <= n for k in ks) and ks[-1] == 0
    for kind in ("mixed", "ties"):
        c, acc, vals, counter = _select_data(n, C, kind, seed=11)
        if kind == "mixed" and n > C:
            # the quantised node's input is what the tie allotment needs: the k-th key ties, the
            # run lies in at least two chunks, some of it is taken and some left
            k1 = ks[1]
            keys = otopk.keys_u32(ops.key(c[1], acc[1]))
            T = np.sort(keys)[n - k1]
            run, taken = np.flatnonzero(keys == T), k1 - int((keys > T).sum())
            assert len(run) > 1 and len(np.unique(run // C)) >= 2, which
            assert 0 < taken < len(run), which
            if which == "3*C+37":  # the taken ties themselves span a chunk edge
                assert run[taken - 1] >= C and run[0] < C
        if kind == "ties":
            keys = otopk.keys_u32(ops.key(c, acc))
            assert (keys[0::2] == keys[0, 0]).all() and keys[0, 0] != 0 and not keys[1::2].any()
        want_acc, want_cnt = acc.copy(), counter.copy()
        pays = [ops.encode_node(c[j], want_acc[j], vals[j], want_cnt[j], k)
                for j, k in enumerate(ks)]
        if kind == "ties":
            assert all((p[0] == np.arange(k)).all() for p, k in zip(pays[:4], ks))
        for with_counter in (True, False):
            err = str((n, kind, aligned, with_counter))
            full_copy = with_counter  # the k = 0 node without a val_out: no copy
            gc, ga, gn, slots, starts = _run_select(dev, codec, c, acc, vals, counter, ks,
                                                    aligned, with_counter, full_copy)
            covered = np.zeros(slots.size, bool)
            for j, k in enumerate(ks):
                si, sv = starts[j]
                if k:
                    assert np.array_equal(slots[si:si + k], pays[j][0]), err
                    assert np.array_equal(slots[sv:sv + k], pays[j][1].view(np.int32)), err
                    covered[si:si + k] = covered[sv:sv + k] = True
                    # the key vector, stored in place into the c row
                    assert np.array_equal(gc[j].view(np.uint32),
                                          ops.key(c[j], acc[j]).view(np.uint32)), err
                else:  # a full share: acc all +0, c and the counter untouched, val_out = vals_src
                    assert not ga[j].view(np.uint32).any(), err
                    assert np.array_equal(gc[j].view(np.uint32), c[j].view(np.uint32)), err
                    assert np.array_equal(gn[j], counter[j]), err
                    if full_copy:
                        assert np.array_equal(slots[sv:sv + n], vals[j].view(np.int32)), err
                        covered[sv:sv + n] = True
            # the slots' tails and every word between and around them: untouched
            assert (slots.view(np.uint32)[~covered] == FILL).all(), err
            assert np.array_equal(ga.view(np.uint32), want_acc.view(np.uint32)), err
            assert np.array_equal(gn, want_cnt if with_counter else counter), err
        # the single-node encode on its exact path with the accumulator, the value source and
        # the counter
        for j, k in enumerate(ks[:4]):
            sc, sa, sv = (torch.from_numpy(a[j].copy()).to(dev) for a in (c, acc, vals))
            sn = torch.from_numpy(counter[j].copy()).to(dev)
            si, so = codec.topk_encode(sc, k, acc=sa, acc_mode=codec.DPZ_ACC_ADD, vals_src=sv,
                                       counter=sn, workspace=ws, exact=True)
            err = f"{(n, kind, aligned)} topk_encode node {j}"
            assert np.array_equal(si.cpu().numpy(), pays[j][0]), err
            assert np.array_equal(_bits(so), pays[j][1].view(np.uint32)), err
            assert np.array_equal(_bits(sa), want_acc[j].view(np.uint32)), err
            assert np.array_equal(sn.cpu().numpy(), want_cnt[j]), err


def test_encode_nodes_wrapper_refuses_a_bad_table(dev):
    from decentralizepy_amd import codec
    z = torch.zeros(2, 8, device=dev)
    out = torch.zeros(16, dtype=torch.int32, device=dev)
    tab = codec.JwinsEncodeTable(z, z.clone(), z.clone(), None, dev)
    tab.set(0, 9, out[:8], out[8:])
    tab.set(1, 0, None, None)
    with pytest.raises(ValueError, match="exceeds"):
        codec.jwins_encode_nodes(tab.upload(), 8)
    tab.set(0, 3, None, out[8:])
    with pytest.raises(ValueError, match="null row"):
        codec.jwins_encode_nodes(tab.upload(), 8)


# ---- the engine -----------------------------------------------------------------------------------
def run_named(name):
    return RUNS[RUN_IDS.index(name)]


def _engine(meta, arr, dev, **kw):
    from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound
    return JwinsBatchRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]).to(dev),
                           meta["alpha_list"], wavelet=meta["wavelet"], level=meta["level"],
                           metadata_cap=meta["metadata_cap"], device=dev, **kw)


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_engine_reproduces_the_reference(dev, meta, arr):
    eng = _engine(meta, arr, dev)
    assert eng.x.is_cuda and eng.M == meta["m_len"]
    for rows in (eng.x, eng.x0, eng.acc, eng.wx, eng.wc, eng.counter):
        assert rows[1].data_ptr() % 256 == 0
    ops.drive(eng, meta, arr)


@pytest.fixture
def rccl_group(dev):
    with rccl_loopback(dev) as group:
        yield group


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_engine_through_rccl_equals_the_reference(dev, rccl_group, meta, arr):
    eng = _engine(meta, arr, dev, rank=0, world=1, group=rccl_group)
    assert eng.coll and eng.recv is not None
    ops.drive(eng, meta, arr, every_payload=True)


@pytest.mark.parametrize("alpha_list", [ops.TUTORIAL_ALPHAS, [0.1, 0.25, 0.4]],
                         ids=["tutorial", "partial_only"])
def test_engine_equals_jwins_round_on_the_hip_ops(dev, alpha_list):
    """regular_16 at N = 4,100 over 3 rounds against JwinsRound (sampled selections on three
    streams, sliced counters): models, accumulators, counters and payloads, bit for bit, on
    inputs whose selections do not tie at the k-th key.  With the tutorial's list every round
    holds a full share and the fold runs node after node; with partial shares only, every round
    takes the guarded one-launch fold."""
    from decentralizepy_amd import codec
    from decentralizepy_amd.gossip_jwins import JwinsRound
    from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound
    meta = run_named("reg16")[0]
    adj = ops.run_adjacency(meta)
    n, nn = 4100, 16
    x = torch.from_numpy(np.random.default_rng(81).standard_normal((nn, n)).astype(np.float32))
    new = JwinsBatchRound(adj, x.to(dev), alpha_list, device=dev)
    old = JwinsRound(adj, x.to(dev), str(alpha_list), metadata_cap=0.5, device=dev)
    assert new.M == old.M == codec.wavedec_len(n, 4)
    for r in range(3):
        for u in range(nn):
            step = torch.from_numpy(ops.perturbation(82, r, u, n)).to(dev)
            new.x[u] += step
            old.x[u] += step
        keys = [(codec.wavedec(new.x[u].contiguous(), 4, x0=new.x0[u].contiguous())[1]
                 + new.acc[u]).cpu().numpy() for u in range(nn)]
        new.step()
        old.step()
        assert new.alphas == old.alphas
        assert any(a >= 0.5 for a in new.alphas) == (len(alpha_list) == 7)
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


def test_engine_with_more_than_four_neighbours_equals_the_restatement(dev):
    """A 7-node star: the hub's six payloads take the fold's node-after-node path."""
    from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound
    adj = [set(range(1, 7))] + [{0} for _ in range(6)]
    n, rounds = 2051, 3
    x = np.random.default_rng(70).standard_normal((7, n)).astype(np.float32)
    eng = JwinsBatchRound(adj, torch.from_numpy(x).to(dev), ops.TUTORIAL_ALPHAS, device=dev)
    drawn = []
    for r in range(rounds):
        for u in range(7):
            eng.x[u] += torch.from_numpy(ops.perturbation(71, r, u, n)).to(dev)
        eng.step()
        drawn += eng.alphas
    assert any(a >= 0.5 for a in drawn) and any(a < 0.5 for a in drawn)
    nodes = direct_round_nodes(adj, x, ops.TUTORIAL_ALPHAS, rounds,
                               lambda r, u: ops.perturbation(71, r, u, n))
    for u, nd in enumerate(nodes):
        assert np.array_equal(_bits(eng.x[u]), nd.model.view(np.uint32)), u
        assert np.array_equal(_bits(eng.x0[u]), nd.init.view(np.uint32)), u
        assert np.array_equal(_bits(eng.acc[u]), nd.acc.view(np.uint32)), u
        assert np.array_equal(eng.counter[u].cpu().numpy(), nd.counter), u


NEW_KERNELS = {"dwt": 2, "idwt": 1, "topk_exact_hist": 3, "topk_exact_resolve": 3,
               "topk_exact_count": 1, "topk_exact_scan": 1, "topk_exact_write": 1}


def test_step_launch_count_is_independent_of_the_node_count(dev):
    """The transforms' and the selection's launches of a step, 6 and 16 nodes.  (The fold's
    count is the library's: a round with a dense payload folds node after node.)"""
    from decentralizepy_amd import codec
    seen = []
    for name in ("irr6", "reg16"):
        meta, arr = run_named(name)
        eng = _engine(meta, arr, dev)
        eng.step()
        with codec.KernelTimer() as t:
            eng.step()
        seen.append({name: cnt for name, (_, cnt) in t.result.items()})
    for counts in seen:
        assert {k: counts.get(k) for k in NEW_KERNELS} == NEW_KERNELS
        assert counts.get("topk_accumulate", 0) == 0 and set(counts) - set(NEW_KERNELS)


def test_step_never_waits_for_the_device(dev, monkeypatch):
    meta, arr = run_named("irr6")
    eng = _engine(meta, arr, dev)
    eng.step()

    def no_wait(*a, **kw):
        raise AssertionError("the step waited for the device")

    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "synchronize", no_wait)
        mp.setattr(torch.cuda.Stream, "synchronize", no_wait)
        mp.setattr(torch.cuda.Event, "synchronize", no_wait)
        legs = []
        eng.step(mark=legs.append)
    assert legs == ["encode", "exchange", "fold", "post"]
    torch.cuda.synchronize(dev)
    assert eng.round == 2 and torch.equal(eng.x, eng.x0)


def test_steps_enqueued_back_to_back_equal_steps_waited_for(dev):
    """Six rounds enqueued without a wait in between (the host runs rounds ahead of the device,
    so a round's encode table is rebuilt on the host while earlier uploads are still queued)
    against the same rounds with a wait after each: equal in every bit."""
    from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound
    adj = ops.run_adjacency(run_named("reg16")[0])
    n, nn, rounds = 1_000_003, 16, 6
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(nn, n, device=dev, generator=gen)
    noise = torch.randn(n, device=dev, generator=gen)
    engines = [JwinsBatchRound(adj, x, ops.TUTORIAL_ALPHAS, device=dev) for _ in range(2)]
    for waited, eng in enumerate(engines):
        torch.cuda.synchronize(dev)
        for r in range(rounds):
            for u in range(nn):
                eng.x[u].add_(torch.roll(noise, 7919 * (u + 1) + r), alpha=0.01)
            eng.step()
            if waited:
                torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)
    a, b = engines
    assert a.alphas == b.alphas and a.round == b.round == rounds
    for ta, tb in ((a.x, b.x), (a.x0, b.x0), (a.acc, b.acc), (a.counter, b.counter)):
        assert torch.equal(ta.view(torch.int32), tb.view(torch.int32))
    for u in range(nn):
        (ai, av), (bi, bv) = a.payload(u), b.payload(u)
        assert (ai is None) == (bi is None) and (ai is None or torch.equal(ai, bi))
        assert torch.equal(av.view(torch.int32), bv.view(torch.int32))
