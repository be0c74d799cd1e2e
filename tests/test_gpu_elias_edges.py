"""The Elias-gamma kernels (csrc/dpz_elias.hip) at their own structural sizes, every comparison
exact: stream lengths on every residue of 32 (the trailer in every byte lane of the word it
shares with the last code bits), encode blocks that end in mid-word next to their neighbours,
the decode chunk (1024 bits), super-map (64 chunks), resolve-pass (16 super maps) and scan-pass
(1024 chunks) edges, a long code starting on each of the last bits of a chunk for every code
length, the 2^26-bit limit, and a last code that overruns the stated end.  Cases:
tests/codec_edges.py; expected bytes: oracle/elias.py, pinned to the unmodified reference by
tests/golden/elias_edges.npz (tests/test_cpu_codec_edges.py)."""
import numpy as np
import pytest
import torch

from oracle import elias as oelias
from tests import codec_edges as ce

pytestmark = pytest.mark.gpu

_ENC = {}


def _oracle(name, idx):
    if name not in _ENC:
        _ENC[name] = oelias.encode(idx)
    return _ENC[name]


def _trailer(enc):
    return int(enc[-8:].view("<i8")[0]), int(enc[-16:-8].view("<i8")[0])


def _padded(enc, dev):
    """The stream on the device, padded to round_up(nbytes, 4) + 16 bytes of non-zero filler
    (the padding is readable, not zero, by the decoder's contract)."""
    nbytes = enc.size
    buf = np.full(((nbytes + 3) // 4) * 4 + 16, 0xA5, dtype=np.uint8)
    buf[:nbytes] = enc
    return torch.from_numpy(buf).to(dev), nbytes


def _decode_all(codec, ws, dev, name, idx, enc, sync64=True, run_async=True):
    """Decode ``enc`` through every entry point; the names of the ones that differ from idx."""
    buf, nbytes = _padded(enc, dev)
    nbits, first = _trailer(enc)
    want = torch.from_numpy(idx).to(dev)
    bad = []
    out = codec.elias_decode(buf, nbytes, nbits, first, nbits - 127, dtype=torch.int32,
                             workspace=ws)
    if out.dtype != torch.int32 or not torch.equal(out, want):
        bad.append(f"{name}:int32")
    if sync64:
        out = codec.elias_decode(buf, nbytes, nbits, first, nbits - 127, dtype=torch.int64,
                                 workspace=ws)
        if out.dtype != torch.int64 or not torch.equal(out, want.to(torch.int64)):
            bad.append(f"{name}:int64")
    if run_async:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        out = codec.elias_decode_async(buf, nbytes, nbits, first, idx.size, status,
                                       dtype=torch.int32, workspace=ws)
        if int(status.item()) != 0 or not torch.equal(out, want):
            bad.append(f"{name}:async")
    return bad


# ------------------------------------------------------------------------------ encode
def test_encode_bytes_guard_and_reuse(dev):
    """Every encode case into one 0xFF-filled buffer (dpz_elias_max_bytes(k) + a 64-byte guard is
    handed over) through one Workspace, in descending then ascending size: the bytes equal the
    oracle's, and every byte from round_up(nbytes, 4) to the buffer's end is still 0xFF.  A
    boundary or tail word that the scan kernel failed to zero before the pack kernel ORs into it
    comes out as 0xFF, and block tables left by a longer stream must not leak into a shorter."""
    from decentralizepy_amd import _lib, codec
    cases = sorted(ce.elias_encode_cases(), key=lambda c: c[1].size)
    cap = int(_lib.lib().dpz_elias_max_bytes(int(cases[-1][1].size))) + 64
    buf = torch.empty(cap, dtype=torch.uint8, device=dev)
    ws = codec.Workspace(dev)
    dev_idx = {name: torch.from_numpy(idx).to(dev) for name, idx in cases}
    dev_ref = {name: torch.from_numpy(_oracle(name, idx)).to(dev) for name, idx in cases}
    bad = []
    for order in (cases[::-1], cases):
        for name, idx in order:
            buf.fill_(0xFF)
            view = buf[:int(_lib.lib().dpz_elias_max_bytes(int(idx.size))) + 64]
            enc = codec.elias_encode(dev_idx[name], out=view, workspace=ws)
            ref = dev_ref[name]
            assert enc.data_ptr() == buf.data_ptr()
            if enc.numel() != ref.numel() or not torch.equal(enc, ref):
                bad.append(f"{name}:bytes")
            r4 = ((ref.numel() + 3) // 4) * 4
            if not bool((buf[r4:] == 0xFF).all()):
                bad.append(f"{name}:guard")
    assert not bad, bad


# ------------------------------------------------------------------------------ decode
def test_decode_encode_cases(dev):
    from decentralizepy_amd import codec
    ws = codec.Workspace(dev)
    bad = []
    for name, idx in ce.elias_encode_cases():
        bad += _decode_all(codec, ws, dev, name, idx, _oracle(name, idx))
    assert not bad, bad


def test_decode_fixture_cases(dev):
    """The reference's own bytes (small cases) and the oracle's bytes that hash to the
    reference's (large cases)."""
    from decentralizepy_amd import codec
    ws = codec.Workspace(dev)
    small, large = ce.load_golden()
    bad = []
    for c in small:
        bad += _decode_all(codec, ws, dev, c["name"], c["input"], c["bytes"])
    for c in large:
        enc = oelias.encode(c["input"])
        assert ce.sha256(enc) == c["sha256"], c["name"]
        bad += _decode_all(codec, ws, dev, c["name"], c["input"], enc)
    assert not bad, bad


@pytest.mark.parametrize("l", (0,) + ce.DECODE_LS)
def test_decode_chunk_super_and_pass_edges(dev, l):
    """L on both sides of one chunk, two chunks, one super map (65536 bits) and 16 super maps =
    1024 chunks (2^20 bits: the resolve pass edge and the scan pass edge together), with codes
    of 2l+1 bits so that the chunk entry offset moves from chunk to chunk."""
    from decentralizepy_amd import codec
    ws = codec.Workspace(dev)
    todo = [(name, L) for name, L, ll in ce.elias_decode_size_cases() if ll == l]
    assert todo and max(L for _, L in todo) > 65536
    bad = []
    for name, L in todo:
        idx = ce.build_size_case(L, l)
        bad += _decode_all(codec, ws, dev, name, idx, oelias.encode(idx))
    assert not bad, bad


@pytest.mark.parametrize("l", range(31))
def test_decode_every_straddle(dev, l):
    """A (2l+1)-bit code beginning s bits before the first chunk edge, for every s = 1..2l+1:
    every chunk exit offset 0..60, and a zero run that ends exactly at, before and after the
    edge.  int32 synchronously for all, asynchronously for s = l + 1."""
    from decentralizepy_amd import codec
    ws = codec.Workspace(dev)
    bad = []
    for s in range(1, 2 * l + 2):
        idx = ce.straddle(l, s)
        bad += _decode_all(codec, ws, dev, f"straddle_l{l}_s{s}", idx, oelias.encode(idx),
                           sync64=False, run_async=(s == l + 1))
    assert not bad, bad


# ------------------------------------------------------------------------------- limit
def test_the_decode_limit(dev):
    """2^26 code bits is the most a stream may hold: ones(2^26) (k = 2^26 + 1, built on the
    device) encodes to 2^23 bytes of 0xFF, int64 LE first = 0, int64 LE nbits = 2^26 + 128 (closed
    form, no oracle) and decodes back; a trailer claiming 2^26 + 1024 bits is refused as
    unsupported by both decode entry points before anything is launched."""
    from decentralizepy_amd import _lib, codec
    L = 2 ** 26
    ws = codec.Workspace(dev)
    idx = torch.arange(L + 1, dtype=torch.int32, device=dev)
    enc = codec.elias_encode(idx, workspace=ws)
    assert enc.numel() == L // 8 + 16
    assert bool((enc[:L // 8] == 0xFF).all())
    tail = enc[L // 8:].cpu().numpy()
    assert tail.tobytes() == np.array([0, L + 128], dtype="<i8").tobytes()
    buf = torch.zeros(enc.numel() + 16, dtype=torch.uint8, device=dev)
    buf[:enc.numel()] = enc
    nbytes = enc.numel()
    del enc
    out = codec.elias_decode(buf, nbytes, L + 128, 0, L + 1, dtype=torch.int32, workspace=ws)
    assert out.numel() == L + 1 and torch.equal(out, idx)
    del out, idx
    # one chunk more: zeros apart from the trailer
    L2 = L + 1024
    nbytes = L2 // 8 + 16
    big = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
    big[nbytes - 8:nbytes] = torch.from_numpy(
        np.frombuffer(np.int64(L2 + 128).tobytes(), dtype=np.uint8).copy()).to(dev)
    with pytest.raises(_lib.CodecError, match="unsupported"):
        codec.elias_decode(big, nbytes, L2 + 128, 0, 16, dtype=torch.int32, workspace=ws)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.CodecError, match="unsupported"):
        codec.elias_decode_async(big, nbytes, L2 + 128, 0, 16, status, workspace=ws)
    assert int(status.item()) == 0  # nothing ran


# ----------------------------------------------------------------------------- overrun
def _reversed_gaps(idx):
    g = np.diff(idx.astype(np.int64))[::-1]
    return ce.from_gaps(g, int(idx[0]))


def test_a_last_code_that_overruns_the_end(dev):
    """The true bytes with nbits - 1.  Two streams whose LAST code is a long one, so that it
    overruns the shortened end: filled(1025, 1) with its gaps in reverse order (two one-bit codes,
    then 341 three-bit codes; L = 1025 -> 1024, so the chunk count drops by one and the code at
    bit 1022 leaves chunk 0 one bit late) and straddle(15, 16) without its 40 trailing one-bit
    codes (the 31-bit code ends at bit 1039 in chunk 1, one past the end: the spec kernel's
    entry-beyond-the-end branch).  elias_decode raises ValueError, elias_decode_async leaves a
    non-zero status word, and a good decode through the same workspace is right afterwards.

    filled(1025, 1) and straddle(15, 16) exactly as built END in one-bit codes: shortened by one
    bit they are well-formed streams of one value fewer, which no decoder can tell from an
    intended one.  For those two the test asserts just that: the synchronous decode returns the
    first k - 1 indices, and the asynchronous one, told to expect k, flags the count."""
    from decentralizepy_amd import codec
    ws = codec.Workspace(dev)
    good = ce.ramp(1025)
    overrun = [("rfilled_L1025_l1", _reversed_gaps(ce.filled(1025, 1))),
               ("straddle_l15_s16_cut", ce.straddle(15, 16)[:-40])]
    assert ce.code_bits(overrun[0][1]) == 1025 and ce.code_bits(overrun[1][1]) == 1039
    for name, idx in overrun:
        enc = oelias.encode(idx)
        assert not _decode_all(codec, ws, dev, name, idx, enc)  # the true stream decodes
        buf, nbytes = _padded(enc, dev)
        nbits, first = _trailer(enc)
        with pytest.raises(ValueError):
            codec.elias_decode(buf, nbytes, nbits - 1, first, idx.size, dtype=torch.int32,
                               workspace=ws)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        codec.elias_decode_async(buf, nbytes, nbits - 1, first, idx.size, status, workspace=ws)
        assert int(status.item()) != 0, name
        status.zero_()
        codec.elias_decode_async(buf, nbytes, nbits - 1, first, idx.size - 1, status,
                                 workspace=ws)
        assert int(status.item()) != 0, name  # malformed, not merely a count mismatch
        assert not _decode_all(codec, ws, dev, "ramp_n1025", good, oelias.encode(good))
    for name, idx in (("filled_L1025_l1", ce.filled(1025, 1)),
                      ("straddle_l15_s16", ce.straddle(15, 16))):
        enc = oelias.encode(idx)
        buf, nbytes = _padded(enc, dev)
        nbits, first = _trailer(enc)
        out = codec.elias_decode(buf, nbytes, nbits - 1, first, idx.size, dtype=torch.int32,
                                 workspace=ws)
        assert torch.equal(out, torch.from_numpy(idx[:-1]).to(dev)), name
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        codec.elias_decode_async(buf, nbytes, nbits - 1, first, idx.size, status, workspace=ws)
        assert int(status.item()) != 0, name
        assert not _decode_all(codec, ws, dev, "ramp_n1025", good, oelias.encode(good))
