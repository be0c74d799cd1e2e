"""GPU: the device LZ4 frame codec (csrc/dpz_lz4.hip) at its block, chunk and length-code edges.
The frames and inputs are the tables of tests/lz4_frames.py (built from the library's own
geometry; tests/test_cpu_lz4_frames.py proves them against liblz4 and the oracle).  Decoder:
every valid frame decodes byte for byte, every malformed one is refused, by the parallel
decoder (DPZ_LZ4_PAR=1, the product's setting) and by the sequential one (DPZ_LZ4_PAR=0).
Encoder: every input's frame decodes everywhere and keeps the promises of the encoder's
block rules.  Every comparison is byte equality."""
import numpy as np
import pytest
import torch

from oracle import lz4 as olz4
from tests import lz4_frames as lf

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not olz4.available(), reason="liblz4 not in this image")]

PAR = ("1", "0")


def _ids(cases):
    return [c.name for c in cases]


def _host(t):
    return bytes(t.cpu().numpy().tobytes())


def _dev_bytes(b, dev, shift=0):
    """``b`` on the device, ``shift`` bytes into a larger buffer (an unaligned source)."""
    big = torch.empty(len(b) + shift + 1, dtype=torch.uint8, device=dev)
    view = big[shift:shift + len(b)]
    if b:
        view.copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    assert view.data_ptr() % 16 == shift % 16
    return view


# ---- decoder -------------------------------------------------------------------------------
@pytest.mark.parametrize("par", PAR)
@pytest.mark.parametrize("case", lf.valid_cases(), ids=_ids(lf.valid_cases()))
def test_valid_frame_decodes(dev, case, par, monkeypatch, diag_lib):
    monkeypatch.setenv("DPZ_LZ4_PAR", par)
    from decentralizepy_amd import codec
    assert _host(codec.lz4_decompress(case.frame, dev)) == case.expected


@pytest.mark.parametrize("case", lf.valid_sample(), ids=_ids(lf.valid_sample()))
def test_valid_frame_decodes_with_the_product_library(dev, case):
    """The library a node loads (no environment switch): a sample of every family."""
    from decentralizepy_amd import codec
    assert _host(codec.lz4_decompress(case.frame, dev)) == case.expected


@pytest.mark.parametrize("par", PAR)
@pytest.mark.parametrize("case", lf.empty_last_sequence_cases(),
                         ids=_ids(lf.empty_last_sequence_cases()))
def test_empty_last_sequence_decodes_in_both_decoders(dev, case, par, monkeypatch, diag_lib):
    """The well-formed neighbour of a match-terminated block (a lone 0x00 token after the match):
    the two decoders agree on it, with the content its sequence list stands for."""
    monkeypatch.setenv("DPZ_LZ4_PAR", par)
    from decentralizepy_amd import codec
    assert _host(codec.lz4_decompress(case.frame, dev)) == case.expected


@pytest.mark.parametrize("par", PAR)
@pytest.mark.parametrize("case", lf.malformed_cases(), ids=_ids(lf.malformed_cases()))
def test_malformed_frame_is_refused(dev, case, par, monkeypatch, diag_lib):
    """Neither decoder accepts what the other, liblz4 or the format refuses."""
    monkeypatch.setenv("DPZ_LZ4_PAR", par)
    from decentralizepy_amd import codec
    with pytest.raises(ValueError):
        codec.lz4_decompress(case.frame, dev)


@pytest.mark.parametrize("case", [c for c in lf.malformed_cases() if "match_ends_block" in c.name],
                         ids=lambda c: c.name)
def test_match_terminated_block_is_refused_by_the_product_library(dev, case):
    from decentralizepy_amd import codec
    with pytest.raises(ValueError):
        codec.lz4_decompress(case.frame, dev)


@pytest.mark.parametrize("par", PAR)
@pytest.mark.parametrize("case", [c for c in lf.valid_cases() if "no_content_size" in c.name],
                         ids=lambda c: c.name)
def test_frame_without_content_size_and_max_size(dev, case, par, monkeypatch, diag_lib):
    """max_size bounds the output of a frame that stores no size: the exact size decodes, one
    byte less is refused (the content does not fit), nothing is written past the bound."""
    monkeypatch.setenv("DPZ_LZ4_PAR", par)
    from decentralizepy_amd import _lib, codec
    n = len(case.expected)
    assert codec.lz4_frame_info(case.frame)[0] == -1
    assert _host(codec.lz4_decompress(case.frame, dev, max_size=n)) == case.expected
    out = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=dev)
    with pytest.raises((ValueError, _lib.CodecError)):
        codec.lz4_decompress(case.frame, dev, out=out[:n - 1], max_size=n - 1)
    torch.cuda.synchronize()
    assert _host(out[n - 1:]) == b"\xEE" * 65


@pytest.mark.parametrize("case", lf.liblz4_large_block_frames(),
                         ids=_ids(lf.liblz4_large_block_frames()))
def test_large_block_frame_is_refused_cleanly(dev, case):
    """liblz4's 256 KB / 1 MB / 4 MB block frames: DPZ_ERR_UNSUPPORTED (not a malformed-frame
    error) before anything is allocated on the device, which is inside the bound the frame's
    blocks give (nb * bmax); a stored content size past that bound is still a malformed frame."""
    import struct

    import xxhash

    from decentralizepy_amd import _lib, codec
    _, nb, _, bmax = codec.lz4_frame_info(case.frame)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    with pytest.raises(_lib.CodecError, match=str(_lib.DPZ_ERR_UNSUPPORTED)):
        codec.lz4_decompress(case.frame, dev)
    peak = torch.cuda.max_memory_allocated(dev) - before
    assert peak <= nb * bmax and peak == 0, peak
    assert bmax > 65536
    big = bytearray(case.frame)
    assert big[4] & 0x08
    big[6:14] = struct.pack("<Q", nb * bmax + 1)
    big[14] = (xxhash.xxh32(bytes(big[4:14])).intdigest() >> 8) & 0xFF
    with pytest.raises(ValueError):
        codec.lz4_decompress(bytes(big), dev)


# ---- encoder -------------------------------------------------------------------------------
_CONTENTS = lf.encoder_contents()


@pytest.mark.parametrize("n", lf.encoder_lengths())
@pytest.mark.parametrize("content", list(_CONTENTS))
def test_encoder_input(dev, content, n, monkeypatch, diag_lib):
    from decentralizepy_amd import _lib, codec
    g = lf.geometry()
    data = _CONTENTS[content](n)
    assert len(data) == n
    frame = _host(codec.lz4_compress(_dev_bytes(data, dev)))
    # the same bytes from an unaligned source (lz_stage's byte path): the same frame
    for shift in (1, 3):
        assert _host(codec.lz4_compress(_dev_bytes(data, dev, shift))) == frame, shift
    assert len(frame) <= int(_lib.lib().dpz_lz4_max_bytes(n))
    assert olz4.ref_decompress(frame) == data
    assert olz4.decode_frame(frame) == data
    for par in PAR:
        monkeypatch.setenv("DPZ_LZ4_PAR", par)
        assert _host(codec.lz4_decompress(frame, dev)) == data, par
    blocks = lf.check_encoder_frame(frame, n)
    full = [b for b in blocks[1:] if b.decoded_len == g["blk"]]
    if content == "constant":
        # lf.constant_block: at 2 KB blocks, matches of 1024 and 1019 and five literals, 20 bytes
        want = lf.constant_block(g["blk"])
        assert all((len(b.seqs), b.csize) == want and not b.raw for b in full), want
    if content in lf.SHORT_PERIODS:
        assert not any(b.raw for b in full)
    if content == "stored_between" and n >= 2 * g["blk"]:
        # the incompressible second block is stored in the linked frame ...
        assert blocks[1].raw and not blocks[0].raw
        if n >= 3 * g["blk"]:  # ... and the block after it has a match whose source lies in it
            b, p, hit = blocks[2], 0, False
            assert not b.raw
            for L, off, M in b.seqs:
                p += L
                if off is not None:
                    hit |= g["blk"] <= 2 * g["blk"] + p - off < 2 * g["blk"]
                    p += M
            assert hit


# ---- wrapper -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1])
def test_wrapper_of_no_and_one_index(dev, k):
    from decentralizepy_amd.compression.Lz4Wrapper import Lz4Wrapper
    c = Lz4Wrapper()
    a = np.array([123_456][:k], dtype=np.int32)
    frame = c.compress(a.copy())
    assert olz4.ref_decompress(frame) == a.tobytes()
    np.testing.assert_array_equal(olz4.wrapper_decompress(frame), a)
    out = c.decompress(frame)
    assert out.dtype == np.int64 and out.shape == (k,)
    np.testing.assert_array_equal(out, a)
    out = c.decompress(olz4.wrapper_compress(a.copy()))  # a reference node's frame
    assert out.dtype == np.int64 and out.shape == (k,)
    np.testing.assert_array_equal(out, a)


def test_wrapper_of_one_value(dev):
    from decentralizepy_amd.compression.Lz4Wrapper import Lz4Wrapper
    c = Lz4Wrapper(compress_data=True)
    v = np.array([-0.0123], dtype=np.float32)
    frame = c.compress_float(v)
    assert olz4.ref_decompress(frame) == v.tobytes()
    back = c.decompress_float(frame)
    assert back.dtype == np.float32 and back.tobytes() == v.tobytes()
    assert c.decompress_float(olz4.ref_compress(v.tobytes())).tobytes() == v.tobytes()
