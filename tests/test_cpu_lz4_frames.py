"""CPU: the LZ4 frame assembler and case tables of tests/lz4_frames.py against liblz4 1.9.3 and
the oracle's frame restatement (every valid case decodes to the content its sequence lists
stand for, every malformed one is refused), the walker's round trip through liblz4's own frames,
and the host frame walk of the library (dpz_lz4_frame_info) on every assembled frame and on
every proper prefix of three of them."""
import collections

import pytest

from oracle import lz4 as olz4
from tests import lz4_frames as lf
from tests.test_oracle_lz4 import _cases

pytestmark = pytest.mark.skipif(not olz4.available(), reason="liblz4 not in this image")


def _ids(cases):
    return [c.name for c in cases]


def test_geometry_export():
    """The figures the tables are built from, and the relations the builders rely on."""
    g = lf.geometry()
    assert set(g) == {"blk", "win", "par_max", "par_cmax", "chunk"}
    assert g["blk"] >= 256 and g["blk"] % 64 == 0 and g["win"] % 64 == 0
    assert g["win"] + g["blk"] < 65536 and g["par_cmax"] > g["par_max"] >= 2 * g["blk"]
    assert g["par_max"] * 16 == 65536 and g["chunk"] == 64


def test_constant_block_figure():
    """The derivation in lf.constant_block at the shipped 2 KB block: three sequences, 20 bytes."""
    assert lf.constant_block(2048) == (3, 20)
    assert lf.constant_block(4096) == (5, 7 + 7 + 7 + 7 + 6)  # 1024 * 3, 1019, five literals


def test_family_sizes():
    """The tables are enumerated, not swept: pin how many cases each family holds."""
    n = collections.Counter(c.name.split("/")[0] for c in lf.valid_cases())
    assert dict(n) == {"run_length": 20, "length_codes": 6, "chunks": 16, "size_gates": 10,
                 "staging": 32, "linked_par": 4, "linked_seq": 6, "frame_options": 8,
                 "liblz4_small": 104}, n
    assert len(lf.malformed_cases()) == 17
    assert len(lf.encoder_lengths()) == 27 and len(lf.encoder_contents()) == 13
    assert max(len(c.frame) for c in lf.valid_cases()) < 300_000
    sample = collections.Counter(c.name.split("/")[0] for c in lf.valid_sample())
    assert set(sample) == set(n) and all(sample[f] == -(-n[f] // 7) for f in n)


def test_match_terminated_cases_reach_both_checks():
    """The nibble-form case has no 15 in its token (the parallel decoder's step-1 fast path);
    the other two have a literal nibble of 15 (its full parse); each block ends on its match."""
    toks = {}
    for c in lf.malformed_cases():
        if "match_ends_block" in c.name:
            at = lf.header(c.frame).data_pos + 4
            toks[c.name] = c.frame[at]
            assert c.frame[-4:] == bytes(4) and not c.name.startswith("match_ends_block_nibble") \
                or (c.frame[at] >> 4 != 15 and c.frame[at] & 15 != 15)
    assert len(toks) == 6
    assert all((t >> 4 == 15) == ("nibble" not in name) for name, t in toks.items()), toks


@pytest.mark.parametrize("case", lf.valid_cases(), ids=_ids(lf.valid_cases()))
def test_valid_case_decodes_to_its_sequence_lists(case):
    assert olz4.ref_decompress(case.frame) == case.expected
    assert olz4.decode_frame(case.frame) == case.expected
    assert b"".join(b.data for b in lf.walk(case.frame)) == case.expected


# liblz4 1.9.3 checks a match's source against the start of its window only, so it decodes an
# offset of 0 (it copies what its output buffer held); the format forbids the value ("0 is an
# invalid offset value"), the oracle's restatement refuses it and so must the device decoders.
LIBLZ4_DOES_NOT_CHECK = ("offset_0",)


@pytest.mark.parametrize("case", lf.malformed_cases(), ids=_ids(lf.malformed_cases()))
def test_liblz4_rejects_malformed_case(case):
    if case.name in LIBLZ4_DOES_NOT_CHECK:
        with pytest.raises(ValueError, match="match offset out of range"):
            olz4.decode_frame(case.frame)
        return
    with pytest.raises(ValueError):
        olz4.ref_decompress(case.frame)


@pytest.mark.parametrize("case", lf.empty_last_sequence_cases(),
                         ids=_ids(lf.empty_last_sequence_cases()))
def test_empty_last_sequence_is_format_valid_and_refused_by_liblz4(case):
    assert olz4.decode_frame(case.frame) == case.expected
    assert b"".join(b.data for b in lf.walk(case.frame)) == case.expected
    with pytest.raises(ValueError):
        olz4.ref_decompress(case.frame)


@pytest.mark.parametrize("case", lf.liblz4_large_block_frames(),
                         ids=_ids(lf.liblz4_large_block_frames()))
def test_large_block_frames_are_valid_frames(case):
    from decentralizepy_amd import codec
    assert olz4.ref_decompress(case.frame) == case.expected
    cs, nb, _, bmax = codec.lz4_frame_info(case.frame)
    assert cs == len(case.expected) and nb == 1 and bmax > 65536


@pytest.mark.parametrize("name", list(_cases()))
def test_walk_round_trip_of_liblz4_frames(name):
    data = _cases()[name]
    for linked in (True, False):
        frm = olz4.ref_compress(data, block_linked=linked)
        blocks = lf.walk(frm)
        assert b"".join(b.data for b in blocks) == data
        assert lf.reassemble(frm) == frm


@pytest.mark.parametrize("case", lf.valid_cases(), ids=_ids(lf.valid_cases()))
def test_frame_info_of_assembled_frames(case):
    from decentralizepy_amd import codec
    h = lf.header(case.frame)
    nb = len(lf.walk(case.frame))
    assert codec.lz4_frame_info(case.frame) == (
        -1 if h.content_size is None else len(case.expected), nb, h.linked, h.block_max)


@pytest.mark.parametrize("case", [c for c in lf.malformed_cases()
                                  if c.name in ("end_mark_missing", "block_size_past_frame")],
                         ids=lambda c: c.name)
def test_frame_info_rejects_broken_block_walk(case):
    from decentralizepy_amd import codec
    with pytest.raises(ValueError):
        codec.lz4_frame_info(case.frame)


PREFIX_FRAMES = ("frame_options/checksums_block1_content1-linked",
                 "length_codes/one_edge_per_block-indep", "linked_par/chain_47_blocks_deep-linked")


@pytest.mark.parametrize("name", PREFIX_FRAMES)
def test_frame_info_rejects_every_proper_prefix(name):
    """A cut frame is refused wherever the cut falls (header, a size field, block data, a block
    checksum, the end mark, the content checksum): never a count of the blocks seen so far."""
    from decentralizepy_amd import codec
    frm = {c.name: c for c in lf.valid_cases()}[name].frame
    assert codec.lz4_frame_info(frm)[1] == len(lf.walk(frm))
    for cut in range(len(frm)):
        with pytest.raises(ValueError):
            codec.lz4_frame_info(frm[:cut])
