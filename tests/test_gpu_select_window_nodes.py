"""The windowed one-read selection of the batched round encodes (csrc/dpz_select_window_nodes.h)
against the selection restated plainly (tests/topkacc_round_ops.py: the fp32 key as the engine
forms it, the k largest by a stable sort on (-key, index)) and against the same engine or entry
point with the exact selection, bit for bit."""
import numpy as np
import pytest
import torch

from tests import topkacc_round_ops as ops
from tests.choco_round_ops import EDGES_IRR6, adjacency

pytestmark = pytest.mark.gpu

C = 8192  # EX_CHUNK: a filter block's elements; a list's segment is a quarter of it
SIZES = [C - 1, C + 1, 3 * C + 5, 2 * C + 2]  # the last: rows that are not 16-byte aligned
GRAPHS = {"path3": adjacency(3, [(0, 1), (1, 2)]), "irr6": adjacency(6, EDGES_IRR6)}
ROUNDS = 4
f32 = np.float32


def window(T):
    """[lo, hi] around a prior threshold key: dpz_topk.h HINT_LO / HINT_HI, the +-1/16 rule of
    dpz_topk_sampled.hip's hint_window, both ends inside."""
    t = np.array([T], np.uint32).view(f32)
    return int((t * f32(1 - 0.0625)).view(np.uint32)[0]), int((t * f32(1 + 0.0625)).view(np.uint32)[0])


def kth_key(c, k):
    return int(np.sort(ops.keys(c))[c.size - k])


def steps(seed, nn, n, k, r):
    """A round's training steps: k + k/4 fresh elements per node and round, spread over the row;
    k of them get magnitudes spread over [1.5, 2.5), the others lie in [1, 1.3), everything else
    is noise of 1e-3.  Every round's k-th key is then near 1.5, inside the window of the last
    one, and what stays in the accumulator lies below every window."""
    out = np.empty((nn, n), f32)
    f = k + k // 4
    for u in range(nn):
        rng = np.random.default_rng([seed, r, u])
        s = (1e-3 * rng.standard_normal(n)).astype(f32)
        where = np.random.default_rng([seed, u]).permutation(n)[f * r:f * (r + 1)]
        mag = np.concatenate([1.5 + np.arange(k) / f32(k), 1 + 0.3 * rng.random(f - k)])
        s[where] = mag * rng.choice([-1, 1], f)
        out[u] = s
    return out


def same(a, b, names):
    for name in names:
        p, q = getattr(a, name), getattr(b, name)
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), name


@pytest.mark.parametrize("alpha", [0.01, 0.1])
@pytest.mark.parametrize("graph", list(GRAPHS))
@pytest.mark.parametrize("n", SIZES)
def test_smooth_run_hits_every_round_and_equals_the_restatement(dev, n, graph, alpha):
    """Round 0 runs exact (status 0); every later round is a window hit for every node, which the
    restatement's own thresholds guarantee before the device is looked at."""
    adj = GRAPHS[graph]
    nn, k = len(adj), round(alpha * n)
    x = np.random.default_rng(5).standard_normal((nn, n)).astype(f32)
    from decentralizepy_amd.gossip_topkacc import TopKAccRound
    win, exact = (TopKAccRound(adj, torch.from_numpy(x).to(dev), alpha, device=dev, selection=s)
                  for s in ("window", "exact"))
    rx, rx0 = x.copy(), x.copy()
    racc, rcnt = np.zeros_like(x), np.zeros((nn, n), np.int32)
    prior = None
    for r in range(ROUNDS):
        st = steps(9, nn, n, k, r)
        rx = (rx + st).astype(f32)
        T = [kth_key((racc[u] + (rx[u] - rx0[u]).astype(f32)).astype(f32), k) for u in range(nn)]
        if prior is not None:  # the condition of a hit, on the CPU
            for u in range(nn):
                lo, hi = window(prior[u])
                assert lo <= T[u] <= hi, (r, u)
        prior = T
        pays = ops.round_all(adj, rx, rx0, racc, rcnt, k, False)
        for e in (win, exact):
            e.x += torch.from_numpy(st).to(dev)
            e.step()
        status = win.selection_status().cpu().numpy()
        assert np.array_equal(status, np.full(nn, 0 if r == 0 else 1)), (r, status)
        assert not exact.selection_status().any()
        same(win, exact, ("x", "x0", "acc", "counter", "send"))
        for u in range(nn):
            idx, vals = win.payload(u)
            assert np.array_equal(idx.cpu().numpy(), pays[u][0]), (r, u)
            assert np.array_equal(ops.u32(vals.cpu().numpy()), ops.u32(pays[u][1])), (r, u)
        assert np.array_equal(ops.u32(win.x.cpu().numpy()), ops.u32(rx)), r
        assert np.array_equal(ops.u32(win.acc.cpu().numpy()), ops.u32(racc)), r
        assert np.array_equal(win.counter.cpu().numpy(), rcnt), r


def table(dev, x, x0, acc, k, aligned):
    """Device rows (every row 16-byte aligned, or 4 bytes past) and the node table over them."""
    from decentralizepy_amd import codec
    m, n = x.shape
    off, stride = (0 if aligned else 1), (n + 3) // 4 * 4 + 8

    def rows(data, dtype=torch.float32):
        back = torch.zeros(m, stride, dtype=dtype, device=dev)
        back[:, off:off + n] = torch.from_numpy(data).to(dev)
        return back[:, off:off + n]

    t = dict(x=rows(x), x0=rows(x0), acc=rows(acc), key=rows(np.zeros_like(x)),
             counter=rows(np.zeros(x.shape, np.int32), torch.int32),
             row=torch.zeros(m, codec.topkacc_row_words(k), dtype=torch.int32, device=dev))
    t["tab"] = codec.topkacc_node_table(t["x"], t["x0"], t["acc"], t["row"], key=t["key"],
                                        counter=t["counter"])
    return t


def run_pair(dev, cs, k, avg, aligned):
    """``cs``: per round the key rows wanted (m, n), or a function of the last round's thresholds
    that gives them; x is set so that the key comes out as wanted whatever acc holds.  The
    windowed entry point, its workspace kept, beside the exact one and the restatement; returns
    every round's status and thresholds."""
    from decentralizepy_amd import codec
    mode = codec.DPZ_ACC_ADD if avg else codec.DPZ_ACC_ACCUMULATE
    racc = rcnt = tw = te = ws = None
    status, Ts = [], []
    for c in cs:
        c = c(Ts[-1]) if callable(c) else c
        if tw is None:
            m, n = c.shape
            racc, rcnt = np.zeros((m, n), f32), np.zeros((m, n), np.int32)
            tw, te = (table(dev, racc, racc, racc, k, aligned) for _ in range(2))
        x, x0 = (c - racc).astype(f32), np.zeros((m, n), f32)
        Ts.append([kth_key((racc[u] + x[u]).astype(f32), k) for u in range(m)])
        for t in (tw, te):
            t["x"].copy_(torch.from_numpy(x).to(dev))
        ws = codec.topkacc_encode_nodes_window(tw["tab"], n, k, mode, ws)
        codec.topkacc_encode_nodes(te["tab"], n, k, mode)
        status.append(codec.window_status(ws, m).cpu().numpy().copy())
        cap = (k + 3) // 4 * 4
        for u in range(m):
            idx, vals = ops.encode(x[u], x0[u], racc[u], rcnt[u], k, avg)
            row = tw["row"][u].cpu().numpy()
            assert np.array_equal(row[4:4 + k], idx), u
            assert np.array_equal(row[4 + cap:4 + cap + k], ops.u32(vals).view(np.int32)), u
        for name in ("acc", "counter", "row"):
            assert torch.equal(tw[name].view(torch.int32), te[name].view(torch.int32)), name
        assert np.array_equal(ops.u32(tw["acc"].cpu().numpy()), ops.u32(racc))
        assert np.array_equal(tw["counter"].cpu().numpy(), rcnt)
    return status, Ts


def inside(T, prior):
    lo, hi = window(prior)
    return lo <= T <= hi


@pytest.mark.parametrize("avg", [False, True], ids=["accumulate", "add"])
@pytest.mark.parametrize("n", SIZES)
def test_a_scaled_node_misses_and_a_constant_node_overflows(dev, n, avg):
    """Three nodes, the same key rows every round, so the thresholds stay put.  In round 1 node
    1's row is multiplied by 8: its k-th key leaves the window (status 2, the others 1), and it
    misses again on the way back.  In round 2 node 2's row is wanted constant at its last
    threshold (equal where acc is +0, within an ulp elsewhere): all of n lies in the window, the
    lists overflow (status 2) and the choice is the restatement's."""
    k, m = round(0.1 * n), 3
    base = np.random.default_rng(n).standard_normal((m, n)).astype(f32)
    scaled = base.copy()
    scaled[1] *= f32(8)

    def constant(T):
        c = base.copy()
        c[2] = np.array([T[2]], np.uint32).view(f32)[0]
        return c

    status, T = run_pair(dev, [base, scaled, constant], k, avg, aligned=n % 4 != 2)
    assert inside(T[1][0], T[0][0]) and inside(T[1][2], T[0][2]) and inside(T[2][0], T[1][0])
    assert not inside(T[1][1], T[0][1]) and not inside(T[2][1], T[1][1])
    assert inside(T[2][2], T[1][2])  # a hit by its threshold: what misses is the capacity
    assert np.array_equal(status[0], [0, 0, 0])
    assert np.array_equal(status[1], [1, 2, 1]), status[1]
    assert np.array_equal(status[2], [1, 2, 2]), status[2]


@pytest.mark.parametrize("avg", [False, True], ids=["accumulate", "add"])
def test_ties_across_the_threshold_go_to_the_lowest_indices(dev, avg):
    """12 % of the keys quantised to 1/64 in [1, 2), the others below 1/4 (the lists hold 17.5 % of
    a segment at alpha = 0.1): the k-th key has more equals than are taken, and those taken lie in
    more than one list segment; the same row again is a hit (status 1) with the exact path's
    choice."""
    n, m = 3 * C + 5, 2
    k = round(0.1 * n)
    rng = np.random.default_rng(3)
    c = np.where(rng.random((m, n)) < 0.12, (64 + rng.integers(0, 64, (m, n))) / f32(64),
                 0.25 * rng.random((m, n)))
    c = (c * rng.choice([-1, 1], (m, n))).astype(f32)
    for u in range(m):
        key = ops.keys(c[u])
        eq = np.flatnonzero(key == kth_key(c[u], k))
        ties = k - int((key > kth_key(c[u], k)).sum())
        assert 1 <= ties < eq.size and eq[0] // (C // 4) != eq[ties - 1] // (C // 4)
    status, _ = run_pair(dev, [c, c], k, avg, aligned=True)
    assert np.array_equal(status[0], [0, 0]) and np.array_equal(status[1], [1, 1]), status


@pytest.mark.parametrize("n", SIZES)
def test_jwins_nodes_use_the_prior_of_their_k_slot(dev, n):
    """``jwins_encode_nodes_window`` on 3 nodes whose k changes from round to round: a node hits
    only where its slot has a prior, runs exact (status 0) where it has none, a full share is 0
    and leaves the priors alone; outputs, acc and counter equal the exact entry point's, the
    indices the restatement's."""
    from decentralizepy_amd import codec
    m, ks = 3, [round(0.05 * n), round(0.1 * n)]
    draws = [(0, 1, None), (0, 1, 0), (1, 0, 0), (0, None, 0)]  # the slot per node, None: full
    want = [(0, 0, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1)]
    c = np.random.default_rng(4).standard_normal((m, n)).astype(f32)
    sides = []
    for _ in range(2):  # rows 4 n + 12 bytes apart: 16-byte aligned or not, as n falls
        t = {name: torch.zeros(m, n + 3, dtype=dt, device=dev)[:, :n]
             for name, dt in (("c", torch.float32), ("acc", torch.float32), ("vals", torch.float32),
                              ("counter", torch.int32), ("idx", torch.int32),
                              ("val", torch.float32))}
        t["vals"].copy_(torch.from_numpy(c[::-1].copy()).to(dev))
        t["tab"] = codec.JwinsEncodeTable(t["c"], t["acc"], t["vals"], t["counter"], dev)
        sides.append(t)
    ws = None
    for draw, st in zip(draws, want):
        for t in sides:  # the key comes out as c whatever acc holds
            t["c"].copy_(torch.from_numpy(c).to(dev) - t["acc"])
            for u, slot in enumerate(draw):
                t["tab"].set(u, 0 if slot is None else ks[slot], t["idx"][u], t["val"][u],
                             0 if slot is None else slot)
            t["tab"].upload()
        ws = codec.jwins_encode_nodes_window(sides[0]["tab"], n, max(ks), ws)
        codec.jwins_encode_nodes(sides[1]["tab"], n)
        assert np.array_equal(codec.window_status(ws, m).cpu().numpy(), st), (draw, st)
        for name in ("c", "acc", "counter", "idx", "val"):
            assert torch.equal(sides[0][name].view(torch.int32),
                               sides[1][name].view(torch.int32)), (draw, name)
        for u, slot in enumerate(draw):
            if slot is not None:
                idx = sides[0]["idx"][u, :ks[slot]].cpu().numpy()
                assert np.array_equal(idx, ops.select(c[u], ks[slot])), (draw, u)


# (M, wavelet, level, N): the issue's sizes as coefficient counts; sym2 at levels 1-4 is
# JwinsBatchRound on the path, the others JwinsWaveletBatchRound on the 6-node graph
JW_CASES = [(C - 1, "sym2", 4, 8179), (C + 1, "sym2", 2, 8187), (3 * C + 5, "sym2", 3, 24573),
            (2 * C + 2, "sym2", 4, 16375), (C - 1, "db3", 2, 8181), (C + 1, "db4", 2, 8179),
            (3 * C + 5, "db3", 3, 24567), (2 * C + 2, "db4", 2, 16373)]
JW_ALPHAS = [0.02, 0.05, 1.0]


def jwins_models(M, wavelet, level, n, rounds):
    """Models G_r = waverec(F_r), F_r sparse: the same 1.25 k_max magnitudes from 2.5 down to 1
    at fresh interior places of the finest detail band, the places of even and odd rounds
    disjoint.  With the step G_r - G_{r-1} the accumulator holds F_{r-1} and the key is F_r, so a
    slot's k-th key is the same magnitude every round."""
    from oracle import wavelet as owav
    fine, f = owav.level_lengths(n, level, wavelet)[1], round(0.05 * M) * 5 // 4
    rng = np.random.default_rng(M)
    places = M - fine + 8 + rng.permutation(fine - 16)[:2 * f].reshape(2, f)
    out = []
    for r in range(rounds):
        F = np.zeros(M, f32)
        F[places[r % 2]] = rng.permutation(2.5 - 1.5 * np.arange(f) / f) * rng.choice([-1, 1], f)
        out.append(owav.waverec_array(F, n, level, wavelet))
    return out


@pytest.mark.parametrize("M,wavelet,level,n", JW_CASES)
def test_jwins_engines_hit_wherever_the_slot_has_a_prior(dev, M, wavelet, level, n):
    """Two partial alphas and 1.0.  The status is foretold on the CPU from the oracle engine's own
    k-th keys: 0 for a full share or a slot without a prior, 1 where the key lies inside the
    window of the slot's last one, which it does unless a full share of the node came between
    (its accumulator then holds F_r - F_{r-1}), else 2.  The device reports exactly that, with
    at least a hit per node, and ends bit for bit where direct_round_nodes and the exact engine
    end."""
    from decentralizepy_amd import gossip_jwins_batch as jb
    from tests.jwins_ops import OracleJwinsOps, direct_round_nodes

    class Noting(OracleJwinsOps):
        def encode(self, wc, k, acc, *rest):
            self.T.append(kth_key(wc.numpy() + acc.numpy(), k))
            super().encode(wc, k, acc, *rest)

    cls, adj = ((jb.JwinsBatchRound, GRAPHS["path3"]) if wavelet == "sym2"
                else (jb.JwinsWaveletBatchRound, GRAPHS["irr6"]))
    nn, kw = len(adj), dict(wavelet=wavelet, level=level)
    x = (1e-4 * np.random.default_rng(7).standard_normal((nn, n))).astype(f32)
    G = [np.zeros(n, f32)] + jwins_models(M, wavelet, level, n, ROUNDS + 2)
    step = [(b - a).astype(f32) for a, b in zip(G, G[1:])]
    cpu = cls(adj, torch.from_numpy(x), JW_ALPHAS, ops=Noting(wavelet, level), **kw)
    win, exact = (cls(adj, torch.from_numpy(x).to(dev), JW_ALPHAS, device=dev, selection=s, **kw)
                  for s in ("window", "exact"))
    assert cpu.M == win.M == M
    prior, hits = [{} for _ in adj], 0
    for r, st in enumerate(step):
        cpu.ops.T = []
        cpu.x += torch.from_numpy(st)
        cpu.step()
        want, T = [], iter(cpu.ops.T)
        for u, a in enumerate(cpu.alphas):
            t = next(T) if a < 0.5 else None
            want.append(0 if t is None or a not in prior[u] else 1 if inside(t, prior[u][a]) else 2)
            if t is not None:
                prior[u][a] = t
        for e in (win, exact):
            e.x += torch.from_numpy(st).to(dev)
            e.step()
        assert win.alphas == cpu.alphas
        assert win.selection_status().tolist() == want, r
        hits += want.count(1)
    assert hits >= nn
    nodes = direct_round_nodes(adj, x, JW_ALPHAS, len(step), lambda r, u: step[r], level=level,
                               wavelet=wavelet)
    for u, nd in enumerate(nodes):
        for got, ref in ((win.x, nd.model), (win.x0, nd.init), (win.acc, nd.acc)):
            assert np.array_equal(ops.u32(got[u].cpu().numpy()), ops.u32(ref)), u
        assert np.array_equal(win.counter[u].cpu().numpy(), nd.counter), u
    same(win, exact, ("x", "acc", "counter", "send"))
