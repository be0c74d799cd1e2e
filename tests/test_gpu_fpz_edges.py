"""The block-floating float kernels (csrc/dpz_fpz.hip) at their structural edges, every comparison
on bits: blocks built to get each exponent width 0..8 (both sides of every bit_length step) at
counts around a float4, a plane word and a full block, through precisions on both sides of
every mantissa-width step; multi-block streams around one grid block (4 waves) and one scan
pass (1024 blocks); decode into unaligned and guarded outputs; encode from unaligned inputs.
Expected bytes: oracle/fpz.py; expected values: the top-p truncation stated in
tests/codec_edges.py without the format (tests/test_cpu_codec_edges.py pins both)."""
import numpy as np
import pytest
import torch

from oracle import fpz as ofpz
from tests import codec_edges as ce
from tests.test_oracle_fpz import SPECIALS

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF


def _dev_f32(u, dev):
    return torch.from_numpy(np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)).to(dev)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _header(ref):
    w = ref[:16].view("<u4")
    return int(w[1]), int(w[2])


@pytest.mark.parametrize("p", ce.FPZ_PRECISIONS)
def test_every_width_and_count(dev, p):
    """Each block case alone (a short block can only be a stream's last): bytes equal the
    oracle's, the decode equals the top-p truncation, and nothing past the block's count is
    written.  All cases share one input, one stream and one output table on the device."""
    from decentralizepy_amd import _lib, codec
    cases = ce.fpz_block_cases()
    nc = len(cases)
    x_host = np.zeros((nc, 256), dtype=np.uint32)
    for i, (_, cnt, _, _, u) in enumerate(cases):
        x_host[i, :cnt] = u
    x = _dev_f32(x_host, dev)                       # rows are 1 KiB apart: 16-byte aligned
    row = int(_lib.lib().dpz_fpz_max_bytes(256))
    streams = torch.zeros((nc, row), dtype=torch.uint8, device=dev)
    outs = _dev_f32(np.full((nc, 256), SENTINEL, dtype=np.uint32), dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = codec.Workspace(dev)
    scratch = torch.empty(row, dtype=torch.uint8, device=dev)
    refs, sizes = [], []
    for i, (name, cnt, _, _, u) in enumerate(cases):
        ref = ofpz.encode(u.view(np.float32), p)
        n, prec = _header(ref)
        assert n == cnt
        enc = codec.fpz_encode(x[i, :cnt], p, out=scratch, workspace=ws)
        sizes.append(enc.numel())
        streams[i, :min(enc.numel(), row)] = enc[:row]
        back = codec.fpz_decode(enc, n, prec, out=outs[i, :cnt], status=status)
        assert back.data_ptr() == outs[i].data_ptr()
        refs.append(ref)
    assert int(status.item()) == 0
    got, vals = streams.cpu().numpy(), _bits(outs)
    bad = []
    for i, (name, cnt, _, _, u) in enumerate(cases):
        if sizes[i] != refs[i].size or not np.array_equal(got[i, :sizes[i]], refs[i]):
            bad.append(f"{name}:bytes")
        if not np.array_equal(vals[i, :cnt], ce.fpz_expected_bits(u, p)):
            bad.append(f"{name}:values")
        if not np.all(vals[i, cnt:] == SENTINEL):
            bad.append(f"{name}:overrun")
    assert not bad, bad


@pytest.mark.parametrize("p", (0, 16, 9))
def test_multi_block_streams(dev, p):
    """1, 3, 4, 5 and 1025 blocks of mixed widths, full and short last blocks: the offset table
    and the block bytes equal the oracle's."""
    from decentralizepy_amd import codec
    ws = codec.Workspace(dev)
    for name, u in ce.fpz_stream_cases():
        ref = ofpz.encode(u.view(np.float32), p)
        n, prec = _header(ref)
        nblk = (n + 255) // 256
        enc = codec.fpz_encode(_dev_f32(u, dev), p, workspace=ws)
        got = enc.cpu().numpy()
        assert got.size == ref.size, name
        t0, t1 = 16, 16 + 4 * (nblk + 1)
        np.testing.assert_array_equal(got[:t0].view("<u4"), ref[:t0].view("<u4"), err_msg=name)
        np.testing.assert_array_equal(got[t0:t1].view("<u4"), ref[t0:t1].view("<u4"),
                                      err_msg=f"{name} table")
        np.testing.assert_array_equal(got[t1:], ref[t1:], err_msg=f"{name} blocks")
        back = codec.fpz_decode(enc, n, prec)
        np.testing.assert_array_equal(_bits(back), ce.fpz_expected_bits(u, p), err_msg=name)


@pytest.mark.parametrize("n", (1, 5, 255, 256, 257, 259))
@pytest.mark.parametrize("lead", (1, 0))
def test_guarded_decode(dev, n, lead):
    """Decode into a view ``lead`` words into a sentinel-filled buffer (lead 1: 4-byte aligned
    only, the scalar store path; lead 0: the float4 path with a guard after n): the values are
    right and every word outside the view keeps the sentinel."""
    from decentralizepy_amd import codec
    u = ce.mixed_stream(2, 256, 11 + n)[:n]
    for p in (0, 16):
        enc = torch.from_numpy(ofpz.encode(u.view(np.float32), p)).to(dev)
        base = _dev_f32(np.full(n + 64, SENTINEL, dtype=np.uint32), dev)
        out = base[lead:lead + n]
        assert out.data_ptr() % 16 == (4 if lead else 0)
        back = codec.fpz_decode(enc, n, 32 if p == 0 else p, out=out)
        assert back.data_ptr() == out.data_ptr()
        got = _bits(base)
        np.testing.assert_array_equal(got[lead:lead + n], ce.fpz_expected_bits(u, p))
        assert np.all(got[:lead] == SENTINEL) and np.all(got[lead + n:] == SENTINEL)


@pytest.mark.parametrize("n", (1, 3, 4, 5, 257))
def test_encode_from_an_unaligned_view(dev, n):
    from decentralizepy_amd import codec
    u = ce.mixed_stream(2, 256, 23 + n)
    base = _dev_f32(u, dev)
    for lead in (1, 2, 3):
        x = base[lead:lead + n]
        assert x.data_ptr() % 16 == 4 * lead
        for p in (0, 11):
            enc = codec.fpz_encode(x, p)
            np.testing.assert_array_equal(
                enc.cpu().numpy(), ofpz.encode(u[lead:lead + n].view(np.float32), p))


@pytest.mark.parametrize("p", ce.FPZ_PRECISIONS)
def test_specials(dev, p):
    """NaN, Inf, zeros, denormals, NaN payloads: bit-exact against the truncation.  A NaN stays a
    NaN from p = 10; below 10 no mantissa bit is kept, so it becomes what the truncation gives
    (Inf), as the kernel's header comment says."""
    from decentralizepy_amd import codec
    u = SPECIALS.view(np.uint32)
    enc = codec.fpz_encode(torch.from_numpy(SPECIALS).to(dev), p)
    ref = ofpz.encode(SPECIALS, p)
    np.testing.assert_array_equal(enc.cpu().numpy(), ref)
    back = codec.fpz_decode(enc, SPECIALS.size, _header(ref)[1]).cpu().numpy()
    np.testing.assert_array_equal(back.view(np.uint32), ce.fpz_expected_bits(u, p))
    if p == 0 or p >= 10:
        assert np.array_equal(np.isnan(back), np.isnan(SPECIALS))
    elif p == 9:
        assert np.all(np.isinf(back[np.isnan(SPECIALS)]))


def test_precision_range(dev):
    """A negative precision is refused (ValueError); 1..9 are accepted (no mantissa bits), as in
    the oracle and EliasFpzipLossy."""
    from decentralizepy_amd import codec
    x = torch.from_numpy(SPECIALS).to(dev)
    enc = codec.fpz_encode(x, 0)
    for p in (-1, -16):
        with pytest.raises(ValueError):
            codec.fpz_encode(x, p)
        with pytest.raises(ValueError):
            codec.fpz_decode(enc, SPECIALS.size, p)
    for p in range(1, 10):
        e = codec.fpz_encode(x, p)
        np.testing.assert_array_equal(e.cpu().numpy(), ofpz.encode(SPECIALS, p))
        back = codec.fpz_decode(e, SPECIALS.size, p)
        np.testing.assert_array_equal(_bits(back),
                                      ce.fpz_expected_bits(SPECIALS.view(np.uint32), p))
