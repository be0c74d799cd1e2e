"""The fp16 packing kernels (csrc/dpz_misc.hip: f2h / h2f) on bits: every half pattern, the
midpoint of every pair of adjacent finite halves with its two fp32 neighbours (round to nearest,
ties to even; 2^-25 and 65520 included), subnormal halves, the overflow threshold, Inf, NaN
payloads, +-FLT_MAX and fp32 denormals.  Expected: numpy's software conversion, the same on
every machine (tests/codec_edges.py); NaN lanes of the narrowing compare by NaN-ness only."""
import numpy as np
import pytest
import torch

from tests import codec_edges as ce

pytestmark = pytest.mark.gpu


def _check_pack(got_u16, x, what):
    want = ce.fp16_expected(x)
    nan = np.isnan(x)
    got_nan = (got_u16 & 0x7C00 == 0x7C00) & (got_u16 & 0x03FF != 0)
    np.testing.assert_array_equal(got_nan, nan, err_msg=f"{what}: NaN lanes")
    bad = np.flatnonzero((got_u16 != want) & ~nan)
    assert bad.size == 0, (what, bad[:8], x[bad[:8]], got_u16[bad[:8]], want[bad[:8]])


def _wide_bits():
    with np.errstate(invalid="ignore"):
        return ce.fp16_all_patterns().view(np.float16).astype(np.float32).view(np.uint32)


def test_pack_rounds_to_nearest_even(dev):
    from decentralizepy_amd import codec
    x = ce.fp16_vector()
    h = codec.pack_fp16(torch.from_numpy(x).to(dev))
    assert h.dtype == torch.float16 and h.numel() == x.size
    _check_pack(h.cpu().numpy().view(np.uint16), x, "pack_fp16")


def test_unpack_widens_every_pattern(dev):
    """All 65 536 patterns against numpy's widening, bit for bit: subnormal halves are exact in
    fp32, and a NaN keeps its sign and payload (mantissa shifted left by 13)."""
    from decentralizepy_amd import codec
    pat = ce.fp16_all_patterns()
    h = torch.from_numpy(pat.view(np.float16)).to(dev)
    got = codec.unpack_fp16(h).cpu().numpy().view(np.uint32)
    want = _wide_bits()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, [hex(v) for v in pat[bad[:8]]],
                           [hex(v) for v in got[bad[:8]]], [hex(v) for v in want[bad[:8]]])


@pytest.mark.parametrize("n", (1, 7, 8, 9, 15, 16, 17, 2055))
def test_sizes_around_the_vector_body(dev, n):
    """The first n values of the tie vector: the 8-per-thread body against the scalar tail, one
    block (2048 values) + 7."""
    from decentralizepy_amd import codec
    x = ce.fp16_tie_vector()[:n].copy()
    out = torch.from_numpy(np.full(n + 24, 0x5A5A, dtype=np.uint16).view(np.float16)).to(dev)
    h = codec.pack_fp16(torch.from_numpy(x).to(dev), out=out)
    got = h.cpu().numpy().view(np.uint16)
    _check_pack(got[:n], x, f"pack n={n}")
    assert np.all(got[n:] == 0x5A5A)
    wide = torch.from_numpy(np.full(n + 24, 0xDEADBEEF, dtype=np.uint32).view(np.float32)).to(dev)
    pat = ce.fp16_all_patterns()[0x03F0:0x03F0 + n]  # across the subnormal / normal border
    back = codec.unpack_fp16(torch.from_numpy(pat.view(np.float16).copy()).to(dev), out=wide)
    got = back.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got[:n], _wide_bits()[0x03F0:0x03F0 + n])
    assert np.all(got[n:] == 0xDEADBEEF)


def test_through_the_compressor(dev):
    from decentralizepy_amd.compression.EliasFp16 import EliasFp16
    c = EliasFp16()
    x = ce.fp16_vector()
    enc = c.compress_float(x)
    assert enc.dtype == np.uint8 and enc.size == 2 * x.size
    _check_pack(enc.view(np.uint16), x, "compress_float")
    pat = ce.fp16_all_patterns()
    back = c.decompress_float(pat.view(np.uint8))
    assert back.dtype == np.float32
    np.testing.assert_array_equal(back.view(np.uint32), _wide_bits())
