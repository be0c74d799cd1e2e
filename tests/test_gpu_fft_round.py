"""GPU: the batched FFT round.  ``dpz_rfft_nodes`` / ``dpz_irfft_nodes`` bit for bit against the
single calls (plus ``dpz_elementwise`` SUB / ADD for the two fusions), ``dpz_cplx_encode_nodes``
against the numpy restatement (tests/fft_round_ops.py) and the single-node sequence ``cplx_key`` ->
exact ``topk_encode`` -> ``cplx_gather`` -> ``cplx_pair_indices``, and the engine
(decentralizepy_amd/gossip_fft.py) against the runs recorded from the unmodified reference, against
the per-node ``sharing.JWINS.FFT`` plugin, through the RCCL loopback and on two ranks.

Measured on an MI355X against the recorded runs, as fractions of ``fft_round_ops.tol`` (printed by
test_engine_reproduces_the_reference): models at most 0.072, payload values 0.036, accumulators
0.038; the keys within 1.4e-6 of the float64 oracle's, relative to a row's largest key, where the
recorded selections keep the k-th key 1.0e-4 or more from the next."""
import numpy as np
import pytest
import torch

from oracle import topk as otopk
from tests import fft_round_ops as ops
from tests import scenario
from tests.dist_harness import rccl_loopback

RUNS = ops.load_runs()
RUN_IDS = [m["name"] for m, _ in RUNS]

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
PAD = 7.0
c64 = np.complex64


def _rows(dev, data, off, pad=PAD):
    """Device rows of the matrix ``data`` (fp32, complex64 or int32), the elements around them
    prefilled; every row ``off`` elements past the start of its backing row, whose length is a
    multiple of 32 elements.  Returns (view, backing)."""
    m, n = data.shape
    back = torch.full((m, -(-(n + 8) // 32) * 32), pad, dtype=torch.from_numpy(data).dtype,
                      device=dev)
    view = back[:, off:off + n]
    view.copy_(torch.from_numpy(data).to(dev))
    return view, back


def _padding_intact(back, n, off, pad=PAD):
    return bool((back[:, :off] == pad).all() and (back[:, off + n:] == pad).all())


def _bits(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint32)


# ---- the transforms -------------------------------------------------------------------------------
# the smallest plan, a radix-17 sub-pass, the primes 257 and 2053 as passes of their own, block
# column tails, one-, two- and three-pass plans (262,144: 256 * 256 * 2)
FFT_SIZES = [4, 6, 60, 272, 514, 1024, 1030, 4100, 4106, 65_536, 131_584, 262_144]


def _single_forward(codec, x, x0, acc):
    """The single-call sequence of one job: rfft(x) or rfft(SUB(x, x0)), ADDed to acc."""
    src = x.contiguous()
    if x0 is not None:
        src = codec.elementwise(codec.DPZ_EW_SUB, src, x0.contiguous())
    f = codec.rfft(src)
    if acc is None:
        return f
    a = torch.view_as_real(acc.contiguous()).reshape(-1).clone()
    codec.elementwise(codec.DPZ_EW_ADD, a, torch.view_as_real(f).reshape(-1), out=a)
    return torch.view_as_complex(a.view(-1, 2))


@pytest.mark.parametrize("n", FFT_SIZES)
def test_transforms_of_jobs_equal_the_single_calls(dev, n):
    from decentralizepy_amd import codec
    assert codec.fft_native(n)
    M = n // 2 + 1
    rng = np.random.default_rng(n)
    x = rng.standard_normal((3, n)).astype(np.float32)
    x0 = (x + 0.1 * rng.standard_normal((3, n))).astype(np.float32)
    acc = (rng.standard_normal((3, M)) + 1j * rng.standard_normal((3, M))).astype(c64)
    tx, bx = _rows(dev, x, 2)   # 8 bytes past a 16-byte boundary
    t0, b0 = _rows(dev, x0, 2)
    zeros = np.full((3, M), PAD, c64)
    for jobs in (1, 3):
        err = str((n, jobs))
        ws = codec.fft_nodes_workspace(jobs, n, dev)
        # plain, with x0, accumulating (x0 and the sum), and per-job flags in one call
        modes = [([False] * 3, [False] * 3), ([True] * 3, [False] * 3), ([True] * 3, [True] * 3),
                 ([False, True, True], [False, False, True])]
        for with_x0, accum in modes:
            init = np.where(np.array(accum)[:, None], acc, zeros)[:jobs]
            out, bout = _rows(dev, init, 1)  # complex rows 8 bytes past a 16-byte boundary
            tab = codec.FftNodesTable(list(tx[:jobs]),
                                      [t0[j] if with_x0[j] else None for j in range(jobs)],
                                      list(out), accum[:jobs], dev)
            codec.rfft_nodes(tab, n, ws)
            for j in range(jobs):
                want = _single_forward(codec, tx[j], t0[j] if with_x0[j] else None,
                                       torch.from_numpy(acc[j]).to(dev) if accum[j] else None)
                assert np.array_equal(_bits(out[j]), _bits(want)), (err, with_x0, accum, j)
            assert _padding_intact(bout, M, 1), err
        # the inverse, of arbitrary coefficients; they are only read
        co, bco = _rows(dev, acc[:jobs], 1)
        back, bback = _rows(dev, np.full((jobs, n), PAD, np.float32), 2)
        codec.irfft_nodes(codec.IfftNodesTable(list(co), list(back), dev), n, ws)
        for j in range(jobs):
            want = codec.irfft(torch.from_numpy(acc[j].copy()).to(dev), n)
            assert np.array_equal(_bits(back[j]), _bits(want)), (err, j)
        assert np.array_equal(_bits(co), acc[:jobs].view(np.uint32)), err
        assert _padding_intact(bco, M, 1) and _padding_intact(bback, n, 2), err
    assert _padding_intact(bx, n, 2) and _padding_intact(b0, n, 2)
    assert np.array_equal(_bits(tx), x.view(np.uint32))
    assert np.array_equal(_bits(t0), x0.view(np.uint32))
    if n <= 4106:  # accuracy, once: the batch against the float64 transform
        fx, _ = _rows(dev, zeros, 1)
        codec.rfft_nodes(codec.FftNodesTable(list(tx), None, list(fx), False, dev), n)
        ref = np.fft.rfft(x.astype(np.float64), axis=1)
        assert np.abs(fx.cpu().numpy() - ref).max() <= scenario.fft_tol(
            "params", n, float(np.abs(x).max()))


def test_transforms_of_jobs_refuse_before_writing(dev):
    """Odd n, n = 2, a hipFFT size and a row 4 bytes off: refused with the documented code, the
    outputs (accumulating ones too) untouched."""
    from decentralizepy_amd import _lib, codec
    rng = np.random.default_rng(9)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    U, A = _lib.DPZ_ERR_UNSUPPORTED, _lib.DPZ_ERR_ARG

    def attempt(n, forward, word=None, accumulate=False):
        """One call on 3 jobs whose rows hold at least n values; ``word``: that word of job 1's
        entry moved 4 bytes."""
        ln = max(n, 8)
        M = ln // 2 + 1
        x = rng.standard_normal((3, ln)).astype(np.float32)
        co = (rng.standard_normal((3, M)) + 1j * rng.standard_normal((3, M))).astype(c64)
        if forward:
            tx, t0 = _rows(dev, x, 2)[0], _rows(dev, x, 2)[0]
            out, bout = _rows(dev, np.full((3, M), PAD, c64), 1)
            tab = codec.FftNodesTable(list(tx), list(t0), list(out), accumulate, dev)
        else:
            tc, _ = _rows(dev, co, 1)
            out, bout = _rows(dev, np.full((3, ln), PAD, np.float32), 2)
            tab = codec.IfftNodesTable(list(tc), list(out), dev)
        if word is not None:
            tab.host[(4 if forward else 2) * 1 + word] += 4
            tab._upload(dev)
        rc = (codec.rfft_nodes if forward else codec.irfft_nodes)(tab, n, ws, check_rc=False)
        torch.cuda.synchronize(dev)
        assert (bout == PAD).all(), (n, forward, word)  # nothing written
        return rc

    assert not codec.fft_native(8198) and codec.fft_native(1030)
    for forward in (True, False):
        for n in (1031, 2, 3, 8198):  # odd, below the smallest plan, 2 * 4099: a hipFFT size
            assert attempt(n, forward) == U, (n, forward)
        for word in range(3 if forward else 2):  # x, x0, out / coeffs, out: 4 bytes off
            assert attempt(1030, forward, word) == A, (forward, word)
    assert attempt(1030, True, 2, accumulate=True) == A
    assert attempt(8198, True, accumulate=True) == U
    with pytest.raises(ValueError, match="native plan"):
        codec.fft_nodes_workspace(3, 8198, dev)
    x = torch.zeros(3, 1030, device=dev)
    out = torch.full((3, 516), PAD, dtype=torch.complex64, device=dev)
    with pytest.raises(_lib.CodecError):  # a short workspace
        codec.rfft_nodes(codec.FftNodesTable(x, None, out, False, dev), 1030,
                         torch.empty(256, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize(dev)
    assert (out == PAD).all()


# ---- the selection --------------------------------------------------------------------------------
SIZES = ["3", "257", "C-1", "C", "C+1", "3*C+37"]
MODES = [otopk.ACC_NONE, otopk.ACC_ACCUMULATE, otopk.ACC_ADD]


def _quant(rng, shape):
    """Complex values on a grid of 0.25 in [-1, 1]^2: few distinct magnitudes, so the k-th key
    ties with many."""
    q = np.float32(0.25)
    return (rng.integers(-4, 5, size=shape) * q + 1j * (rng.integers(-4, 5, size=shape) * q)
            ).astype(c64)


def _select_data(M, seed):
    """3 nodes (change, acc, vals_src, counter): node 0 quantised in change and acc, node 1
    gaussian, node 2 with every key equal under every mode (change = 3 + 4i, acc = 0)."""
    rng = np.random.default_rng([seed, M])
    ch = (rng.standard_normal((3, M)) + 1j * rng.standard_normal((3, M))).astype(c64)
    acc = (0.05 * (rng.standard_normal((3, M)) + 1j * rng.standard_normal((3, M)))).astype(c64)
    ch[0], acc[0] = _quant(rng, M), _quant(rng, M)
    ch[2], acc[2] = c64(3 + 4j), 0
    vals = (rng.standard_normal((3, M)) + 1j * rng.standard_normal((3, M))).astype(c64)
    counter = rng.integers(0, 5, size=(3, M)).astype(np.int32)
    return ch, acc, vals, counter


def _ks(M):
    return sorted({1, max(1, M // 2), max(1, M - 1), M})


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset"])
@pytest.mark.parametrize("which", SIZES)
def test_encode_nodes_equals_restatement_and_the_single_sequence(dev, which, aligned):
    from decentralizepy_amd import codec
    C = codec.cplx_chunk_elems()
    M = eval(which, {"C": C})
    ch, acc, vals, counter = _select_data(M, seed=13)
    wsp = codec.Workspace(dev)
    oc, ok_ = (0, 0) if aligned else (1, 1)  # complex rows 8, the key row 4 bytes past 16
    for k in _ks(M):
        for mode in MODES:
            want_acc, want_cnt = acc.copy(), counter.copy()
            want = [ops.encode_node(ch[j], None if mode == otopk.ACC_NONE else want_acc[j], mode,
                                    vals[j], want_cnt[j], k) for j in range(3)]
            # the quantised node ties at its k-th key; the constant node selects 0 .. k - 1
            keys0 = otopk.keys_u32(want[0][0])
            if 1 < k < M and M > 3:
                assert otopk.kth_has_tie(keys0, k), (M, k, mode)
            assert np.array_equal(want[2][1][0::2], 2 * np.arange(k)), (M, k, mode)
            for m, with_counter in ((3, True), (3, False), (1, True), (1, False)):
                err = str((M, k, mode, m, with_counter, aligned))
                tch, bch = _rows(dev, ch[:m], oc)
                tacc, bacc = _rows(dev, acc[:m], oc)
                tv, bv = _rows(dev, vals[:m], oc)
                tkey, bkey = _rows(dev, np.full((m, M), PAD, np.float32), ok_)
                tn, bn = _rows(dev, counter[:m], ok_, 77)
                # slots: [6 words | 2 k pair words | 6 words | 2 k value words] per node
                span = 6 + 2 * k + 6 + 2 * k
                slots = torch.from_numpy(np.full(m * span + 6, FILL, np.uint32).view(np.int32)
                                         ).to(dev)
                pair = [slots[j * span + 6:j * span + 6 + 2 * k] for j in range(m)]
                val = [slots[j * span + 12 + 2 * k:j * span + 12 + 4 * k] for j in range(m)]
                tab = codec.CplxEncodeTable(tch, None if mode == otopk.ACC_NONE else tacc, tv,
                                            tkey, tn if with_counter else None, pair, val, dev)
                codec.cplx_encode_nodes(tab, M, k, mode)
                got = slots.cpu().numpy()
                covered = np.zeros(got.size, bool)
                for j in range(m):
                    key, pairs, v = want[j]
                    p0, v0 = j * span + 6, j * span + 12 + 2 * k
                    assert np.array_equal(got[p0:p0 + 2 * k], pairs), err
                    assert np.array_equal(got[v0:v0 + 2 * k], v.view(np.int32)), err
                    covered[p0:p0 + 2 * k] = covered[v0:v0 + 2 * k] = True
                    assert np.array_equal(_bits(tkey[j]), key.view(np.uint32)), err
                assert (got.view(np.uint32)[~covered] == FILL).all(), err
                assert np.array_equal(_bits(tacc), (acc if mode == otopk.ACC_NONE
                                                    else want_acc)[:m].view(np.uint32)), err
                assert np.array_equal(tn.cpu().numpy(),
                                      (want_cnt if with_counter else counter)[:m]), err
                assert np.array_equal(_bits(tch), ch[:m].view(np.uint32)), err
                assert np.array_equal(_bits(tv), vals[:m].view(np.uint32)), err
                for back, ln, off, pad in ((bch, M, oc, PAD), (bacc, M, oc, PAD),
                                           (bv, M, oc, PAD), (bkey, M, ok_, PAD),
                                           (bn, M, ok_, 77)):
                    assert _padding_intact(back, ln, off, pad), err
            # the single-node sequence of the plugin, on its exact path
            for j in range(3):
                sc, sa, sv = (torch.from_numpy(a[j].copy()).to(dev) for a in (ch, acc, vals))
                sn = torch.from_numpy(counter[j].copy()).to(dev)
                use = None if mode == otopk.ACC_NONE else sa
                key = codec.cplx_key(sc, use, mode)
                idx, _ = codec.topk_encode(key, k, counter=sn, workspace=wsp, exact=True)
                v = codec.cplx_gather(sv, idx, acc=use)
                pairs = codec.cplx_pair_indices(idx)
                err = f"{(M, k, mode)} the single sequence, node {j}"
                assert np.array_equal(_bits(key), want[j][0].view(np.uint32)), err
                assert np.array_equal(pairs.cpu().numpy(), want[j][1]), err
                assert np.array_equal(_bits(v), want[j][2].view(np.uint32)), err
                assert np.array_equal(_bits(sa), (acc if mode == otopk.ACC_NONE
                                                  else want_acc)[j].view(np.uint32)), err
                assert np.array_equal(sn.cpu().numpy(), want_cnt[j]), err


# ---- the engine -----------------------------------------------------------------------------------
def run_named(name):
    return RUNS[RUN_IDS.index(name)]


def _engine(meta, arr, dev, lo=0, hi=None, **kw):
    from decentralizepy_amd.gossip_fft import FftRound
    return FftRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"][lo:hi]).to(dev),
                    device=dev, **ops.engine_kwargs(meta), **kw)


def _key_error(meta, arr, dev):
    """The device keys' worst relative error against the float64 oracle's keys over the run."""
    from decentralizepy_amd import codec
    eng = _engine(meta, arr, dev)
    ref = _engine_cpu(meta, arr)
    worst = 0.0
    for r in range(meta["rounds"]):
        for e in (eng, ref):
            x = e.x.cpu().numpy()
            for j in range(meta["nodes"]):
                x[j] = ops.train(x[j], meta, r, j)
            e.x.copy_(torch.from_numpy(x).to(e.x.device))
            e.step()
        a, b = eng.key.cpu().numpy().astype(np.float64), ref.key.numpy().astype(np.float64)
        worst = max(worst, float((np.abs(a - b) / np.abs(b).max(axis=1, keepdims=True)).max()))
    assert codec.fft_native(meta["n"])
    return worst


def _engine_cpu(meta, arr):
    from decentralizepy_amd.gossip_fft import FftRound
    return FftRound(ops.run_adjacency(meta), torch.from_numpy(arr["x0"]),
                    device=torch.device("cpu"), ops=ops.OracleFftOps(), **ops.engine_kwargs(meta))


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_engine_reproduces_the_reference(dev, meta, arr):
    eng = _engine(meta, arr, dev)
    assert eng.x.is_cuda and eng.M == meta["m_len"] and eng.native
    rows = [eng.x, eng.x0, eng.fx, eng.ch, eng.key, eng.counter]
    for t in rows + ([eng.acc] if eng.acc is not None else []):
        assert t[0].data_ptr() % 256 == 0 and t[1].data_ptr() % 256 == 0
    errs = {}
    ops.drive(eng, meta, arr, errs=errs)
    # the keys against the oracle's, relative to the row's largest key: far inside the gap that
    # separates the k-th key from the next in every recorded selection
    kerr = _key_error(meta, arr, dev)
    print(meta["name"], {w: round(max(v), 4) for w, v in errs.items()}, "key error", kerr,
          "gap", meta["min_gap"])
    assert kerr < 1e-5 < ops.MIN_GAP <= meta["min_gap"]


@pytest.fixture
def rccl_group(dev):
    with rccl_loopback(dev) as group:
        yield group


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_engine_through_rccl_equals_one_rank_without_a_group(dev, rccl_group, meta, arr):
    eng = _engine(meta, arr, dev, rank=0, world=1, group=rccl_group)
    assert eng.coll and eng.recv is not None
    got = ops.drive(eng, meta, arr, every_payload=True)
    ops.same_bits(got, ops.drive(_engine(meta, arr, dev), meta, arr, every_payload=True))


@pytest.mark.parametrize("meta,arr", RUNS, ids=RUN_IDS)
def test_two_ranks_equal_one_rank(dev, meta, arr):
    """Two ranks' engines in this process (RCCL refuses two ranks on one device, so their
    all-gather is done here with device copies; the collective itself is covered by the loopback
    above and by gloo on the CPU): every array equals the one-rank run's, bit for bit."""
    from decentralizepy_amd.gossip_round import shard
    nn = meta["nodes"]
    engines = []
    for rank in range(2):
        lo, hi, _ = shard(nn, 2, rank)
        engines.append(_engine(meta, arr, dev, lo, hi, rank=rank, world=2))
    one = _engine(meta, arr, dev)
    for r in range(meta["rounds"]):
        for e in engines + [one]:
            x = e.x.cpu().numpy()
            for j in range(e.m):
                x[j] = ops.train(x[j], meta, r, e.lo + j)
            e.x.copy_(torch.from_numpy(x).to(dev))
        one.step()
        for e in engines:
            e.encode()
        for e in engines:
            e.recv.copy_(torch.cat([s.send for s in engines]))
        for e in engines:
            e.fold()
            e.post()
        for e in engines:
            rows = slice(e.lo, e.hi)
            pairs = [(e.x, one.x[rows]), (e.x0, one.x0[rows]), (e.key, one.key[rows]),
                     (e.counter, one.counter[rows]), (e.fx, one.fx[rows])]
            pairs += [(e.acc, one.acc[rows])] if e.acc is not None else []
            for a, b in pairs:
                assert np.array_equal(_bits(a), _bits(b)), (r, e.rank)
            for u in range(nn):
                (ai, av), (bi, bv) = e.payload(u), one.payload(u)
                assert torch.equal(ai, bi) and np.array_equal(_bits(av), _bits(bv)), (r, u)


class _TopoGraph:
    def __init__(self, adj):
        self.adj = adj

    def neighbors(self, uid):
        return self.adj[uid]


def _plugin_rounds(adj, x0, shape, rounds, seed, kwargs, tmpdir):
    """The per-node plugin driven node by node over ``adj``: per round the payloads, and after
    it the models, accumulators and counters."""
    from collections import deque

    from decentralizepy_amd.sharing.JWINS.FFT import FFT
    nn = len(adj)
    plugins = []
    for u in range(nn):
        model = scenario.make_model(shape)
        scenario.set_flat(model, x0[u])
        plugins.append(FFT(u, 0, None, scenario._Mapping(nn), _TopoGraph(adj), model, None,
                           str(tmpdir), dict_ordered=True, **kwargs))
    out = []
    meta = {"seed": seed}
    for r in range(rounds):
        msgs = []
        for u, p in enumerate(plugins):
            scenario.set_flat(p.model, ops.train(scenario.get_flat(p.model), meta, r, u))
            m = p.get_data_to_send(degree=len(adj[u]))
            m["CHANNEL"] = "DPSGD"
            msgs.append(m)
        got = {}
        for u, m in enumerate(msgs):
            got[f"idx{u}"] = np.asarray(m["indices"], dtype=np.int32)
            got[f"vals{u}"] = np.asarray(m["params"], dtype=c64)
        if kwargs.get("accumulation"):
            got["acc_enc"] = np.stack([p.model.accumulated_changes.cpu().numpy()
                                       for p in plugins])
        for u, p in enumerate(plugins):
            p._averaging({v: deque([dict(msgs[v])]) for v in adj[u]})
        got["x"] = np.stack([scenario.get_flat(p.model) for p in plugins])
        got["counter"] = np.stack([np.asarray(p.model.shared_parameters_counter.cpu().numpy(),
                                              dtype=np.int32) for p in plugins])
        if kwargs.get("accumulation"):
            got["acc"] = np.stack([p.model.accumulated_changes.cpu().numpy() for p in plugins])
        out.append(got)
    return out


def _engine_rounds(eng, rounds, seed):
    out, meta = [], {"seed": seed}
    for r in range(rounds):
        x = eng.x.cpu().numpy()
        for j in range(eng.m):
            x[j] = ops.train(x[j], meta, r, j)
        eng.x.copy_(torch.from_numpy(x).to(eng.x.device))
        snap = {}

        def mark(leg):
            if leg == "encode" and eng.acc is not None:
                snap["acc_enc"] = eng.acc.clone()
        eng.step(mark=mark)
        got = {"x": eng.x.cpu().numpy(), "counter": eng.counter.cpu().numpy()}
        for u in range(eng.n_nodes):
            idx, vals = eng.payload(u)
            got[f"idx{u}"], got[f"vals{u}"] = idx.cpu().numpy(), vals.cpu().numpy()
        if eng.acc is not None:
            got["acc_enc"], got["acc"] = snap["acc_enc"].cpu().numpy(), eng.acc.cpu().numpy()
        out.append(got)
    return out


PLUGIN_CASES = [("plain", (30, 33, 34), dict()),
                ("acc", (30, 33, 40), dict(accumulation=True)),
                ("accavg", (50, 81, 50), dict(accumulation=True,
                                              accumulate_averaging_changes=True)),
                # N = 8,198 = 2 * 4099: no native plan, the transforms run node after node
                ("accavg_hipfft", (90, 90, 98), dict(accumulation=True,
                                                     accumulate_averaging_changes=True))]


@pytest.mark.parametrize("name,shape,kwargs", PLUGIN_CASES, ids=[c[0] for c in PLUGIN_CASES])
def test_engine_equals_the_per_node_plugin(dev, tmp_path, name, shape, kwargs):
    """3 rounds over the 6-node graph against ``sharing.JWINS.FFT`` plugin objects driven node by
    node: payloads, models, accumulators (after the encode and after the round) and counters, bit
    for bit."""
    from decentralizepy_amd import codec
    from decentralizepy_amd.gossip_fft import FftRound
    adj = ops.adjacency(6, ops.EDGES_IRR6)
    n = shape[0] * shape[1] + shape[2]
    assert codec.fft_native(n) == (name != "accavg_hipfft") and (n == 8198) == (not
                                                                               codec.fft_native(n))
    x0 = np.random.default_rng(n).standard_normal((6, n)).astype(np.float32)
    eng = FftRound(adj, torch.from_numpy(x0).to(dev), 0.1, device=dev, **kwargs)
    assert eng.native == codec.fft_native(n)
    got = _engine_rounds(eng, 3, seed=91)
    want = _plugin_rounds(adj, x0, shape, 3, 91, dict(alpha=0.1, **kwargs), tmp_path)
    ops.same_bits(got, want)
    assert set(got[0]) == set(want[0])


def test_engine_with_more_than_four_neighbours_equals_the_plugin(dev, tmp_path):
    """A 7-node star: the hub's six payloads take the fold's node-after-node path."""
    from decentralizepy_amd.gossip_fft import FftRound
    adj = [set(range(1, 7))] + [{0} for _ in range(6)]
    shape, kwargs = (30, 33, 40), dict(accumulation=True, accumulate_averaging_changes=True)
    x0 = np.random.default_rng(70).standard_normal((7, 1030)).astype(np.float32)
    eng = FftRound(adj, torch.from_numpy(x0).to(dev), 0.1, device=dev, **kwargs)
    ops.same_bits(_engine_rounds(eng, 2, seed=92),
                  _plugin_rounds(adj, x0, shape, 2, 92, dict(alpha=0.1, **kwargs), tmp_path))


def test_step_launch_count_is_independent_of_the_node_count(dev):
    """The kernel launches of a step at m = 1 and m = 3, on a native size, from the library's
    own timing counters: equal, kernel by kernel."""
    from decentralizepy_amd import codec
    from decentralizepy_amd.gossip_fft import FftRound
    n = 4100
    seen = []
    for adj in ([set()], [{1, 2}, {0}, {0}]):
        x = torch.from_numpy(np.random.default_rng(3).standard_normal((len(adj), n))
                             .astype(np.float32)).to(dev)
        eng = FftRound(adj, x, 0.1, accumulation=True, accumulate_averaging_changes=True,
                       device=dev)
        eng.x += 0.01
        eng.step()
        eng.x += 0.01
        with codec.KernelTimer() as t:
            eng.step()
        seen.append({name: cnt for name, (_, cnt) in t.result.items()})
    one, three = seen
    fold = {k: v for k, v in three.items() if not k.startswith(("fft", "topk_exact"))}
    assert fold  # the fold's kernels: the library's own count
    for counts in seen:
        # 2050 = 205 * 10: two passes and the pairing per forward set, two passes per inverse
        assert counts["fft"] == 3 + 2 + 3
        assert (counts["topk_exact_hist"], counts["topk_exact_resolve"]) == (3, 3)
        assert (counts["topk_exact_count"], counts["topk_exact_scan"],
                counts["topk_exact_write"]) == (1, 1, 1)
        assert "cplx" not in counts and "ew" not in counts and "topk_accumulate" not in counts
    assert {k: v for k, v in one.items() if k.startswith(("fft", "topk_exact"))} == \
        {k: v for k, v in three.items() if k.startswith(("fft", "topk_exact"))}


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
        mp.setattr(torch.Tensor, "item", no_wait)
        mp.setattr(torch.Tensor, "cpu", no_wait)
        legs = []
        eng.step(mark=legs.append)
    assert legs == ["encode", "exchange", "fold", "post"]
    torch.cuda.synchronize(dev)
    assert eng.round == 2 and torch.equal(eng.x, eng.x0)
