"""CPU checks behind the codec edge tests (tests/test_gpu_{elias,fpz,fp16}_edges.py): the case
builders of tests/codec_edges.py hold what they claim, the Elias oracle (oracle/elias.py) equals
the unmodified reference on every fixture case (tests/golden/elias_edges.npz / .json), and the
float oracle (oracle/fpz.py) keeps the codec's contract, stated here without the format: a round
trip returns the top p bits of every bit pattern."""
import numpy as np
import pytest

from oracle import elias as oelias
from oracle import fpz as ofpz
from tests import codec_edges as ce


def _trailer_bits(enc):
    return int(enc[-8:].view("<i8")[0]) - 128


def _first_long_code_start(idx):
    """Bit position of the first code longer than one bit."""
    g = np.diff(idx.astype(np.int64))
    j = int(np.argmax(g > 1))
    assert g[j] > 1 and np.all(g[:j] == 1)
    return j


# ------------------------------------------------------------------------ the cases hold
def test_elias_builders_have_the_stated_bits():
    for L in (1, 31, 32, 33, 1023, 1024, 1025, 65537):
        assert ce.ones(L).size == L + 1
        assert _trailer_bits(oelias.encode(ce.ones(L))) == L
    for name, L, l in ce.elias_decode_size_cases():
        idx = ce.build_size_case(L, l)
        assert idx.dtype == np.int32 and int(idx[-1]) < 2 ** 31 and np.all(np.diff(idx) > 0), name
        assert ce.code_bits(idx) == L, name
        assert _trailer_bits(oelias.encode(idx)) == L, name
        if l:  # long codes of exactly 2l+1 bits, as many as fit
            g = np.diff(idx.astype(np.int64))
            assert int((g > 1).sum()) == L // (2 * l + 1) and g.max() < 2 ** (l + 1), name
    # every l from the decode list reaches past one super map (65536 bits) at least once
    for l in ce.DECODE_LS:
        assert any(ll == l and L > 65536 for _, L, ll in ce.elias_decode_size_cases())
    assert ce.code_bits(ce.ramp(1024)) == 3946 and 3946 % 32 == 10
    assert _trailer_bits(oelias.encode(ce.ramp(1024))) == 3946


def test_every_straddle_starts_its_long_code_before_the_chunk_edge():
    seen = set()
    for l in range(31):
        gaps = set()
        for s in range(1, 2 * l + 2):
            idx = ce.straddle(l, s)
            assert int(idx[-1]) < 2 ** 31
            g = np.diff(idx.astype(np.int64))
            if l:
                assert _first_long_code_start(idx) == 1024 - s
                assert int(g[1024 - s]).bit_length() == l + 1
                gaps.add(int(g[1024 - s]))
            assert ce.code_bits(idx) == ce.straddle_bits(l, s)
            seen.add(1024 - s + 2 * l + 1 - 1024)  # the chunk's exit offset
        if l >= 2:  # the smallest gap, the largest (clamped at l = 30) and one in between
            assert 2 ** l in gaps and (len(gaps) == 3 or l == 30)
            assert (2 ** (l + 1) - 1 in gaps) or l == 30
    assert seen == set(range(61))
    for l in ce.GOLDEN_STRADDLE_LS:
        enc = oelias.encode(ce.straddle(l, l + 1))
        assert _trailer_bits(enc) == ce.straddle_bits(l, l + 1)


def test_encode_cases_are_valid_and_cover_every_trailer_lane():
    cases = ce.elias_encode_cases()
    assert len({n for n, _ in cases}) == len(cases)
    res = set()
    for name, idx in cases:
        assert idx.dtype == np.int32 and idx.size >= 2 and np.all(np.diff(idx.astype(np.int64)) > 0)
        assert 0 <= int(idx[0]) and int(idx[-1]) < 2 ** 31, name
        res.add(ce.code_bits(idx) % 32)
    assert res == set(range(32))
    streams = ce.pow2_edges()
    gaps = sorted(int(g) for a in streams for g in np.diff(a.astype(np.int64)))
    assert gaps == sorted(g for l in range(1, 31) for g in (2 ** l - 1, 2 ** l, 2 ** l + 1))
    assert int(streams[-1][-1]) == 2 ** 31 - 1
    assert ce.code_bits(ce.three_59()) == 3 * 59 and ce.code_bits(ce.one_61()) == 61
    assert any(int(idx[0]) >= 128 for _, idx in cases)
    assert any(int(idx[0]) >= 2 ** 24 for _, idx in cases)


def test_fpz_blocks_get_the_intended_exponent_width():
    widths = set()
    for name, cnt, emin, span, u in ce.fpz_block_cases():
        assert u.dtype == np.uint32 and u.size == cnt
        enc = ofpz.encode(u.view(np.float32), 0).view("<u4")
        assert int(enc[3]) == 1
        meta = int(enc[4 + 2])  # header (4), table (2), then the block's meta word
        assert (meta >> 8) & 0xFF == ce.block_width(cnt, span), name
        assert meta >> 16 == 23
        if cnt > 1:
            assert meta & 0xFF == emin, name
            widths.add((meta >> 8) & 0xFF)
    assert widths == set(range(9))
    assert {ce.block_width(256, s) for s in ce.FPZ_SPANS} == set(range(9))
    for name, u in ce.fpz_stream_cases():
        nblk = int(name[1:].split("_")[0])
        assert (u.size + 255) // 256 == nblk, name
    assert any(u.size % 256 for _, u in ce.fpz_stream_cases())


def test_fp16_vector_holds_the_ties():
    x = ce.fp16_vector()
    assert x.dtype == np.float32
    have = set(x.view(np.uint32).tolist())
    for v in (2.0 ** -25, 65520.0, -(2.0 ** -25), -65520.0):  # a midpoint and its neighbours
        for w in (v, np.nextafter(np.float32(v), np.float32(0)),
                  np.nextafter(np.float32(v), np.float32(np.copysign(np.inf, v)))):
            assert int(np.float32(w).view(np.uint32)) in have
    for v in (65504.0, np.inf, -np.inf, 2.0 ** -24, 0.0, -0.0):
        assert int(np.float32(v).view(np.uint32)) in have
    for bits in (0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 1, 0x807FFFFF):
        assert bits in have
    h = ce.fp16_expected(np.array([2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)),
                                   65520.0, np.nextafter(np.float32(65520), np.float32(0)),
                                   2049.0, 2051.0], dtype=np.float32))
    assert h.tolist() == [0x0000, 0x0001, 0x7C00, 0x7BFF, 0x6800, 0x6802]  # ties go to even
    t = ce.fp16_tie_vector()
    assert t.size == 2 * 3 * 0x7C00


# ------------------------------------------------------------ oracle against the reference
def test_elias_oracle_equals_the_reference_on_every_fixture_case():
    small, large = ce.load_golden()
    assert len(small) == 31 and len(large) == 5
    for c in small:
        name, idx = c["name"], c["input"]
        assert idx.dtype == np.int32 and int(idx[-1]) < 2 ** 31
        np.testing.assert_array_equal(idx, ce.golden_small_cases()[name], err_msg=name)
        enc = oelias.encode(idx)
        np.testing.assert_array_equal(enc, c["bytes"], err_msg=name)
        L = ce.golden_bits(name)
        assert L is None or _trailer_bits(c["bytes"]) == L, name
        if c["decoded"] is None:  # stored as a digest; the oracle's per-bit decode is too slow
            assert c["decoded_count"] == idx.size
            assert ce.sha256(idx.astype(np.int64)) == c["decoded_sha256"], name
        else:
            assert c["decoded"].dtype == np.int64
            np.testing.assert_array_equal(c["decoded"], idx.astype(np.int64), err_msg=name)
            np.testing.assert_array_equal(oelias.decode(c["bytes"]), c["decoded"], err_msg=name)
    for c in large:
        enc = oelias.encode(c["input"])
        assert c["input"].size == c["k"] and enc.size == c["nbytes"], c["name"]
        assert ce.sha256(enc) == c["sha256"], c["name"]
        assert _trailer_bits(enc) == ce.golden_bits(c["name"]), c["name"]


# ------------------------------------------------------------------------- the fpz contract
@pytest.mark.parametrize("p", ce.FPZ_PRECISIONS)
def test_fpz_oracle_round_trip_is_the_top_p_bits(p):
    for name, cnt, emin, span, u in ce.fpz_block_cases():
        y = ofpz.decode(ofpz.encode(u.view(np.float32), p)).view(np.uint32)
        mask = np.uint32(0xFFFFFFFF if p == 0 or p >= 32 else (0xFFFFFFFF << (32 - p)) & 0xFFFFFFFF)
        want = u & mask
        if 10 <= p < 32:  # a NaN whose kept mantissa is zero also gets the quiet bit
            nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
            want = np.where(nan & ((want & 0x007FFFFF) == 0), want | np.uint32(0x00400000), want)
        np.testing.assert_array_equal(y, want, err_msg=f"{name} p={p}")
        np.testing.assert_array_equal(ce.fpz_expected_bits(u, p), want, err_msg=name)
    for name, u in ce.fpz_stream_cases():
        if u.size > 2000 and p not in (0, 9, 16):
            continue
        y = ofpz.decode(ofpz.encode(u.view(np.float32), p)).view(np.uint32)
        np.testing.assert_array_equal(y, ce.fpz_expected_bits(u, p), err_msg=f"{name} p={p}")
