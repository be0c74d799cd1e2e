"""GPU: the fused sym2 / haar wavelet kernels at the lengths their tiling makes special
(tests/wavelet_edges.py: every length around 1, 2, (3,) 4 forward tiles and around 1, 2, 3
inverse tiles, from the built kernels' own widths), bit for bit against the oracle
(oracle/wavelet.py, pinned to PyWavelets by fixtures and independent of the device code).

Per length: the W(x), W(x - x0) pair, each output alone, the accumulating pass with and without
the rewind mask, the inverse of the oracle's coefficients; x and x0 from 16-byte aligned storage
and as views one float into a buffer (the scalar-load path of the span loader); every output
followed by guard words that must come back untouched.  At level 4 also the sharded tile entry
(last tile alone, then the rest), and at the lengths of the one-output odd tail (below) the
generic-filter kernels with the sym2 bank as a second device implementation.

Before the one-output tail tile was widened (dwt_tile_first, csrc/dpz_dwt.hip) the sym2 sweep
failed on an MI355X at exactly the lengths tests/wavelet_edges.py::predicted_unstaged names —
n mod 128 * 2^L in {255} (L = 1), {507, 508} (L = 2), {1011..1014} (L = 3), {2019..2026}
(L = 4), for every k: 53 lengths in the 13 sym2 cases — and nowhere else.  Two words differed
each time, the last cA_L and the last cD_L (all that a one-output tail tile owns), in the forward
forms, aligned and not, sharded and not (which forms failed at a length varied: the unwritten
LDS slots hold what the previous launch left there, at times the right values).  The generic
kernels, the guards and every haar and inverse case agreed with the oracle throughout
(DESIGN.md §3.4).
"""
import numpy as np
import pytest
import torch

from oracle import wavelet as owav
from tests import wavelet_edges as we

pytestmark = pytest.mark.gpu

GUARD = 8                    # words after every output
PATTERN = 0x7FC5A5A5         # a NaN no kernel produces
CHUNK = 220                  # lengths per parametrised case (haar level 8: 1281 per window)
HAAR_LEVELS = (1, 4, 8)
INVERSE_LEVELS = (1, 4, 8)


def _widths():
    from decentralizepy_amd import shard
    return shard.tile_widths()


def _forward_cases():
    out = []
    for wavelet, levels in (("sym2", we.FORWARD_LEVELS), ("haar", HAAR_LEVELS)):
        for level, k in we.forward_cases(levels):
            count = 5 * (1 << level) + 1
            parts = -(-count // CHUNK)
            for part in range(parts):
                out.append(pytest.param(wavelet, level, k, part, parts,
                                        id=f"{wavelet}-L{level}-k{k}" +
                                        (f"-part{part}" if parts > 1 else "")))
    return out


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).view(np.int32))


class _Out:
    """an m-word output followed by GUARD pattern words, at an odd or even word offset"""

    def __init__(self, m, dev, prefill=None):
        self.m = m
        self.buf = torch.full((m + GUARD,), PATTERN, dtype=torch.int32, device=dev)
        self.view = self.buf[:m].view(torch.float32)
        if prefill is not None:
            self.view.copy_(prefill)

    def diff(self, want_i32):
        """None, or what differs from `want` (device int32) / from the guard pattern"""
        got = self.buf[:self.m]
        msg = []
        if not torch.equal(got, want_i32):
            ne = (got != want_i32).nonzero().flatten()
            msg.append(f"{ne.numel()} of {self.m} words differ, first {int(ne[0])}, "
                       f"last {int(ne[-1])}")
        if not bool((self.buf[self.m:] == PATTERN).all()):
            msg.append("guard words overwritten")
        return "; ".join(msg) or None


def _inputs(base_x, base_noise, n):
    """standard normals with a few +-0.0 and a subnormal near each end; x0 = x - 0.01 noise"""
    x = base_x[:n].copy()
    x[1], x[4], x[2] = 0.0, -0.0, 1e-40
    x[n - 2], x[n - 5], x[n - 3] = -0.0, 0.0, -3e-41
    x0 = (x - np.float32(0.01) * base_noise[:n]).astype(np.float32)
    return x, x0


def _on_device(a, dev, offset):
    """`a` on the device: from 16-byte aligned storage (offset 0) or as a view one float into a
    larger buffer (offset 1)"""
    t = torch.from_numpy(a).to(dev)
    if offset:
        big = torch.empty(a.shape[0] + 4, dtype=torch.float32, device=dev)
        big[offset:offset + a.shape[0]].copy_(t)
        t = big[offset:offset + a.shape[0]]
    assert t.data_ptr() % 16 == 4 * offset and t.is_contiguous()
    return t


def _selection(rng, lens, level, m):
    """m // 10 selected positions: the last cA_L, the last of every cD_l, positions = 31 (mod 32)
    and random ones"""
    ends = {lens[level] - 1}
    off = lens[level]
    for lv in range(level, 0, -1):
        off += lens[lv]
        ends.add(off - 1)
    assert max(ends) == m - 1
    want = max(m // 10, len(ends))
    at31 = [p for p in range(31, m, 32) if p not in ends]  # m / 32 of them: all fit
    forced = np.array(sorted(ends) + at31[:want - len(ends)], dtype=np.int64)
    need, extra = want - forced.shape[0], np.empty(0, dtype=np.int64)
    while extra.shape[0] < need:  # distinct random positions outside the forced ones
        cand = np.unique(np.concatenate([extra, rng.integers(0, m, size=2 * need + 8)]))
        extra = cand[~np.isin(cand, forced)]
    return np.sort(np.concatenate([forced, rng.permutation(extra)[:need]]))


def _mask_of(idx, m):
    words = np.zeros((m + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return words


def _generic_sym2(tx, tx0, level, cx, cd):
    """the generic-filter kernels driven with the sym2 bank (what codec.wavedec does past level
    4): a second device implementation of the same transform"""
    from decentralizepy_amd import _lib, codec
    n = tx.numel()
    ws, nb = codec._generic_ws(n, level, "sym2", tx.device)
    rc = _lib.lib().dpz_dwt_generic(codec._ptr(tx), codec._ptr(tx0), n, level,
                                    codec._ptr(codec._bank("sym2", tx.device)), 4,
                                    codec._ptr(cx), codec._ptr(cd), 0, None, codec._ptr(ws), nb,
                                    codec._stream(tx.device))
    _lib.check(rc, "dpz_dwt_generic(sym2)")


def _report(failures, what):
    if failures:
        ns = sorted({n for n, _ in failures})
        lines = [f"n={n}: {msg}" for n, msg in failures]
        more = f"\n... {len(lines) - 60} more" if len(lines) > 60 else ""
        pytest.fail(f"{what}: {len(ns)} failing lengths {ns}\n" + "\n".join(lines[:60]) + more,
                    pytrace=False)


@pytest.mark.parametrize("wavelet,level,k,part,parts", _forward_cases())
def test_forward_sweep_bit_exact(dev, wavelet, level, k, part, parts):
    from decentralizepy_amd import codec
    from decentralizepy_amd.shard import dwt_rank_part
    dwt_tile, _ = _widths()
    lengths = we.forward_lengths(level, k, dwt_tile)[part * CHUNK:(part + 1) * CHUNK]
    assert lengths
    rng = np.random.default_rng(1000 * level + 10 * k + part + (7 if wavelet == "haar" else 0))
    nmax = max(lengths)
    base_x = rng.standard_normal(nmax).astype(np.float32)
    base_noise = rng.standard_normal(nmax).astype(np.float32)
    base_acc = (0.01 * rng.standard_normal(owav.coeff_len(nmax, level, wavelet) + 64)
                ).astype(np.float32)
    t_span = dwt_tile << level
    predicted = set(we.predicted_unstaged(level, dwt_tile)) if wavelet == "sym2" else set()
    failures = []
    for n in lengths:
        x, x0 = _inputs(base_x, base_noise, n)
        lens = we.level_lengths(n, level, wavelet)
        want_x = owav.wavedec_array(x, level, wavelet)
        want_d = owav.wavedec_array((x - x0).astype(np.float32), level, wavelet)
        m = want_x.shape[0]
        assert m == codec.wavedec_len(n, level, wavelet) == lens[level] + sum(lens[1:])
        sel = _selection(rng, lens, level, m)
        acc0 = base_acc[:m].copy()
        acc0[sel[::3]] = -0.0
        acc0[rng.integers(0, m, size=4)] = -0.0
        rewound = acc0.copy()
        rewound[sel] = 0.0
        w_x, w_d = _i32(want_x).to(dev), _i32(want_d).to(dev)
        w_acc = _i32((acc0 + want_d).astype(np.float32)).to(dev)
        w_rw = _i32((rewound + want_d).astype(np.float32)).to(dev)
        t_acc0 = torch.from_numpy(acc0).to(dev)
        mask = torch.from_numpy(_mask_of(sel, m).view(np.int32)).to(dev)
        assert mask.numel() >= codec.mask_words(m)

        def note(name, out, want, n=n):
            d = out.diff(want)
            if d:
                failures.append((n, f"{name}: {d}"))

        for off in (0, 1):
            tx, tx0 = _on_device(x, dev, off), _on_device(x0, dev, off)
            tag = "aligned" if off == 0 else "view+1"
            cx, cd = _Out(m, dev), _Out(m, dev)
            codec.wavedec(tx, level, x0=tx0, coeffs_x=cx.view, coeffs_diff=cd.view,
                          wavelet=wavelet)
            note(f"pair W(x) {tag}", cx, w_x)
            note(f"pair W(x-x0) {tag}", cd, w_d)
            ox = _Out(m, dev)
            codec.wavedec(tx, level, coeffs_x=ox.view, wavelet=wavelet)
            note(f"W(x) only {tag}", ox, w_x)
            od = _Out(m, dev)
            codec.wavedec(tx, level, x0=tx0, want_x=False, coeffs_diff=od.view, wavelet=wavelet)
            note(f"W(x-x0) only {tag}", od, w_d)
            oa = _Out(m, dev, t_acc0)
            codec.wavedec(tx, level, x0=tx0, want_x=False, coeffs_diff=oa.view, accumulate=True,
                          wavelet=wavelet)
            note(f"accumulate {tag}", oa, w_acc)
            orw = _Out(m, dev, t_acc0)
            codec.wavedec(tx, level, x0=tx0, want_x=False, coeffs_diff=orw.view, accumulate=True,
                          wavelet=wavelet, rewind_mask=mask)
            note(f"accumulate + rewind {tag}", orw, w_rw)
            if off == 0 and wavelet == "sym2" and level == 4:
                # the sharded entry: the last tile alone, then the rest, into one output; equal
                # to the unsharded result above
                nt = we.forward_tiles(n, level, dwt_tile)
                sx, sd, sa = _Out(m, dev), _Out(m, dev), _Out(m, dev, t_acc0)
                for lo, hi in ((nt - 1, nt), (0, nt - 1)):
                    dwt_rank_part(tx, tx0, 0, n, level, lo, hi, sx.view, sd.view)
                    dwt_rank_part(tx, tx0, 0, n, level, lo, hi, None, sa.view, accumulate=True)
                note("sharded W(x) vs unsharded", sx, cx.buf[:m])
                note("sharded W(x-x0) vs unsharded", sd, cd.buf[:m])
                note("sharded accumulate vs unsharded", sa, oa.buf[:m])
            if off == 0 and n % t_span in predicted:
                gx, gd = _Out(m, dev), _Out(m, dev)
                _generic_sym2(tx, tx0, level, gx.view, gd.view)
                note("generic kernels, sym2 bank, W(x)", gx, w_x)
                note("generic kernels, sym2 bank, W(x-x0)", gd, w_d)
        rec = _Out(n, dev)
        codec.waverec(w_x.view(torch.float32), n, level, out=rec.view, wavelet=wavelet)
        note("waverec", rec, _i32(owav.waverec_array(want_x, n, level, wavelet)).to(dev))
    torch.cuda.synchronize()
    _report(failures, f"{wavelet} level {level}, k = {k}")


@pytest.mark.parametrize("level", INVERSE_LEVELS)
@pytest.mark.parametrize("wavelet", ["sym2", "haar"])
def test_inverse_sweep_bit_exact(dev, wavelet, level):
    """waverec of the oracle's coefficients around 1, 2, 3 inverse tiles (sym2 at level 8:
    codec.waverec takes the generic kernels, so the fused entry is also called directly)"""
    from decentralizepy_amd import _lib, codec
    _, idwt_tile = _widths()
    rng = np.random.default_rng(50 + level)
    nmax = 3 * idwt_tile + 4
    base_x = rng.standard_normal(nmax).astype(np.float32)
    failures = []
    for k in we.INVERSE_K:
        for n in we.inverse_lengths(k, idwt_tile):
            x, _ = _inputs(base_x, base_x, n)
            c = owav.wavedec_array(x, level, wavelet)
            want = _i32(owav.waverec_array(c, n, level, wavelet)).to(dev)
            tc = torch.from_numpy(c).to(dev)
            outs = [("waverec", _Out(n, dev))]
            codec.waverec(tc, n, level, out=outs[0][1].view, wavelet=wavelet)
            if wavelet == "sym2" and not codec._fused(wavelet, level):
                outs.append(("dpz_idwt_sym2", _Out(n, dev)))
                rc = _lib.lib().dpz_idwt_sym2(codec._ptr(tc), n, level,
                                              codec._ptr(outs[1][1].view), codec._stream(dev))
                _lib.check(rc, "dpz_idwt_sym2")
            for name, out in outs:
                d = out.diff(want)
                if d:
                    failures.append((n, f"{name}: {d}"))
    torch.cuda.synchronize()
    _report(failures, f"{wavelet} inverse, level {level}")
