"""An LZ4 frame assembler, a sequence walker and the case tables that place frames and encoder
inputs at the edges of the device codec (csrc/dpz_lz4.hip): its 2 KB encoder block and 14 KB
history, the parallel decoder's size gates and 64-byte walk chunk, the length-code extension
bytes, the 64 KB ring of the sequential decoder.  No GPU, no device code: plain byte
arithmetic shared by tests/test_cpu_lz4_frames.py and tests/test_gpu_lz4_edges.py.  The
geometry comes from the built library (``codec.lz4_geometry()``), not from literals.

The expected content of every valid case follows from the assembler's own sequence lists
(``Builder``), never from a decoder; the CPU module proves that liblz4 and the oracle's
``decode_frame`` both return it.
"""
import collections
import functools
import struct

import numpy as np
import xxhash

MAGIC = 0x184D2204
MINMATCH = 4
MAXM = 1024       # the encoder's match cap
MFLIMIT = 12      # a match starts at least 12 bytes before its block's end
LASTLIT = 5       # the last 5 bytes of a block are literals

Case = collections.namedtuple("Case", "name frame expected")
Block = collections.namedtuple("Block", "raw seqs decoded_len data csize")
Header = collections.namedtuple("Header", "linked content_size block_checksum content_checksum "
                                          "bd block_max data_pos")


class Stored(bytes):
    """Block data that goes into the frame uncompressed (high bit of the size field)."""


@functools.lru_cache(maxsize=None)
def geometry():
    from decentralizepy_amd import codec
    return codec.lz4_geometry()


def _xxh32(b):
    return xxhash.xxh32(bytes(b), seed=0).intdigest()


def _rand(seed, n):
    """n random bytes, none of them zero (a byte the decoder failed to resolve reads as 0)."""
    return np.random.default_rng(seed).integers(1, 256, n, dtype=np.uint8).tobytes()


# ---- the assembler -------------------------------------------------------------------------
def _ext(n):
    """The extension bytes of a length whose nibble is 15: 255 ..., r with 15 + sum = n."""
    out = bytearray()
    n -= 15
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)
    return bytes(out)


def seq_bytes(literals, offset, match_len):
    """One sequence; ``offset`` None: literals only (the form of a block's last sequence)."""
    L = len(literals)
    m = 0 if offset is None else match_len - MINMATCH
    assert m >= 0 and (offset is None or 0 <= offset <= 0xFFFF)
    out = bytearray([(min(L, 15) << 4) | min(m, 15)])
    if L >= 15:
        out += _ext(L)
    out += literals
    if offset is not None:
        out += struct.pack("<H", offset)
        if m >= 15:
            out += _ext(m)
    return bytes(out)


def block(seqs, raw_tail=True):
    """LZ4 block bytes of ``[(literals, offset | None, match_len), ...]``.  The last sequence is
    literals only: when the list ends on a match an empty one is appended, unless
    ``raw_tail=False`` (malformed on purpose: the block then ends on its match)."""
    seqs = list(seqs)
    assert all(s[1] is not None for s in seqs[:-1]), "only the last sequence is literal-only"
    if raw_tail and (not seqs or seqs[-1][1] is not None):
        seqs.append((b"", None, 0))
    return b"".join(seq_bytes(*s) for s in seqs)


def token_positions(seqs):
    """Compressed position of every sequence's token."""
    pos, out = 0, []
    for s in seqs:
        out.append(pos)
        pos += len(seq_bytes(*s))
    return out


def frame(blocks, linked=True, content_size=None, block_checksum=False, content_checksum=False,
          bd=4, content=None, end_mark=True):
    """An LZ4 frame around ``blocks`` (bytes: a compressed block, ``Stored``: an uncompressed
    one): magic, FLG / BD, optional content size, HC = xxh32(descriptor) >> 8, size-prefixed
    blocks with optional per-block xxh32, end mark, optional xxh32 of ``content``."""
    flg = 0x40 | (0 if linked else 0x20) | (0x10 if block_checksum else 0) | \
        (0x08 if content_size is not None else 0) | (0x04 if content_checksum else 0)
    desc = bytearray([flg, bd << 4])
    if content_size is not None:
        desc += struct.pack("<Q", content_size)
    out = bytearray(struct.pack("<I", MAGIC)) + desc
    out.append((_xxh32(desc) >> 8) & 0xFF)
    for b in blocks:
        out += struct.pack("<I", len(b) | (0x80000000 if isinstance(b, Stored) else 0))
        out += b
        if block_checksum:
            out += struct.pack("<I", _xxh32(b))
    if end_mark:
        out += struct.pack("<I", 0)
        if content_checksum:
            out += struct.pack("<I", _xxh32(content))
    return bytes(out)


# ---- the walker ----------------------------------------------------------------------------
def header(frm):
    b = bytes(frm)
    assert struct.unpack_from("<I", b, 0)[0] == MAGIC
    flg, bd = b[4], b[5]
    assert flg >> 6 == 1 and not flg & 0x03, "version 01, no dictionary id"
    pos = 6
    cs = None
    if flg & 0x08:
        cs = struct.unpack_from("<Q", b, pos)[0]
        pos += 8
    assert (_xxh32(b[4:pos]) >> 8) & 0xFF == b[pos], "header checksum"
    bid = (bd >> 4) & 7
    return Header(not flg & 0x20, cs, bool(flg & 0x10), bool(flg & 0x04), bid, 1 << (8 + 2 * bid),
                  pos + 1)


def walk(frm):
    """Per block of a well-formed frame: ``Block(raw, [(lit_len, offset, match_len), ...],
    decoded_len, data, csize)``; the last sequence of a compressed block reads (lit_len, None, 0).
    A format walker (it asserts what the format requires), used to state properties of what the
    device encoder emits and to take liblz4's frames apart."""
    b = bytes(frm)
    h = header(b)
    pos = h.data_pos
    out = bytearray()
    blocks = []
    while True:
        sz = struct.unpack_from("<I", b, pos)[0]
        pos += 4
        if sz == 0:
            break
        n = sz & 0x7FFFFFFF
        src = b[pos:pos + n]
        assert len(src) == n
        pos += n
        if h.block_checksum:
            assert struct.unpack_from("<I", b, pos)[0] == _xxh32(src)
            pos += 4
        start = len(out)
        seqs = []
        if sz >> 31:
            out += src
        else:
            i = 0
            while True:
                tok = src[i]
                i += 1
                L = tok >> 4
                if L == 15:
                    while True:
                        x = src[i]
                        i += 1
                        L += x
                        if x != 255:
                            break
                assert i + L <= n
                out += src[i:i + L]
                i += L
                if i == n:
                    seqs.append((L, None, 0))
                    break
                off = src[i] | (src[i + 1] << 8)
                i += 2
                M = tok & 15
                if M == 15:
                    while True:
                        x = src[i]
                        i += 1
                        M += x
                        if x != 255:
                            break
                M += MINMATCH
                assert i < n, "a match ends the block"
                p = len(out) - off
                assert off >= 1 and p >= (0 if h.linked else start)
                for t in range(M):
                    out.append(out[p + t])
                seqs.append((L, off, M))
        blocks.append(Block(bool(sz >> 31), seqs, len(out) - start, bytes(out[start:]), n))
    if h.content_checksum:
        assert struct.unpack_from("<I", b, pos)[0] == _xxh32(out)
        pos += 4
    assert pos == len(b) and (h.content_size is None or h.content_size == len(out))
    return blocks


def reassemble(frm):
    """``frame(block(...))`` of what ``walk`` read: the same bytes for a canonically coded frame."""
    h = header(frm)
    blocks, content = [], bytearray()
    for blk in walk(frm):
        if blk.raw:
            blocks.append(Stored(blk.data))
        else:
            seqs, p = [], 0
            for L, off, M in blk.seqs:
                seqs.append((blk.data[p:p + L], off, M))
                p += L + M
            blocks.append(block(seqs))
        content += blk.data
    return frame(blocks, h.linked, h.content_size, h.block_checksum, h.content_checksum, h.bd,
                 bytes(content))


# ---- content from sequence lists -----------------------------------------------------------
class Builder:
    """Blocks and, from the same sequence lists, the content they stand for."""

    def __init__(self, linked):
        self.linked = linked
        self.blocks = []
        self.out = bytearray()

    def stored(self, data):
        self.blocks.append(Stored(data))
        self.out += data
        return self

    def comp(self, seqs):
        start = 0 if self.linked else len(self.out)
        for lit, off, M in seqs:
            self.out += lit
            if off is not None:
                p = len(self.out) - off
                assert off >= 1 and p >= start and M >= MINMATCH, (off, p, start, M)
                for t in range(M):
                    self.out.append(self.out[p + t])
        self.blocks.append(block(seqs))
        return self

    def case(self, name, size=True, **opts):
        content = bytes(self.out)
        name = f"{name}-{'linked' if self.linked else 'indep'}"
        frm = frame(self.blocks, self.linked, len(content) if size else None, content=content,
                    **opts)
        assert len(frm) < 300_000, name
        return Case(name, frm, content)


def _both(fn):
    """The case(s) ``fn(builder)`` builds, as a linked and as an independent frame."""
    out = []
    for linked in (True, False):
        r = fn(Builder(linked))
        out += r if isinstance(r, list) else [r]
    return out


def _sized_seq(seed, size, off, M):
    """A sequence with a match whose compressed form is exactly ``size`` bytes."""
    for L in range(size):
        s = (_rand(seed, L), off, M)
        if len(seq_bytes(*s)) == size:
            return s
    raise AssertionError(size)


TAIL = 5  # literals after a block's last match (the format's LASTLITERALS)


def _tail(seed, n=TAIL):
    return (_rand(seed, n), None, 0)


# ---- decoder: valid frames -----------------------------------------------------------------
def run_length_cases():
    """Non-zero run-length data at the parallel decoder's decoded-size gate, and short periods
    whose copy is longer than its offset (pointer jumping; the ``t % off`` copy)."""
    g = geometry()
    pm = g["par_max"]
    out = []
    for total in (pm - 1, pm, pm + 1):  # one literal, one offset-1 match, five literals
        out += _both(lambda b, total=total: b.comp(
            [(b"\xAB", 1, total - 1 - TAIL), _tail(1)]).case(f"rle1_decodes_{total}"))
    # one match longer than the parallel decoder's block (its LZ_BIG marker)
    out += _both(lambda b: b.comp([(b"\xAB", 1, pm + 1), _tail(2)]).case("rle1_big_match"))
    for off in (2, 3, 5, 63, 64, 65):
        assert pm - off - TAIL > max(64, off)
        out += _both(lambda b, off=off: b.comp(
            [(_rand(10 + off, off), off, pm - off - TAIL), _tail(3)]).case(f"period_{off}"))
    return out


LIT_EDGES = (14, 15, 16, 269, 270, 271, 524, 525)
MATCH_EDGES = (18, 19, 20, 273, 274, 275, 1024, 1025)


def length_code_cases():
    """Literal runs and match lengths where the nibble fills (15 / 19) and where the first and
    the second extension byte fill (270, 525 / 274, 529-1): random literals, so a mis-sized run
    shows in every byte after it."""
    def lits(b):
        return b.comp([(_rand(20 + i, L), 7 + i, 4 + i) for i, L in enumerate(LIT_EDGES)] +
                      [_tail(4)]).case("literal_runs")

    def matches(b):
        return b.comp([(_rand(40 + i, 9), 9 - (i % 3), M) for i, M in enumerate(MATCH_EDGES)] +
                      [_tail(5)]).case("match_lengths")

    def each(b):  # every edge in a block of its own, so a block BEGINS with each code
        for i, L in enumerate(LIT_EDGES):
            b.comp([(_rand(60 + i, L), L, 4), _tail(6)])
        for i, M in enumerate(MATCH_EDGES):
            b.comp([(_rand(80 + i, 3), 2, M), _tail(7)])
        return b.case("one_edge_per_block")
    return _both(lits) + _both(matches) + _both(each)


def empty_last_sequence_cases():
    """A match, then the lone token 0x00 as the block's last byte: the nearest well-formed
    neighbour of a block that ends on its match (the parallel decoder's step-1 fast path for 9
    literals, lz_parse_at for 20).  NOT in the valid tables: liblz4 1.9.3 refuses it (it takes a
    literal run with fewer than 8 bytes after it for the block's last and wants the block to end
    there), the block format's parse and both device decoders read it.  It pins that the two
    device decoders agree right next to the refusal."""
    def one(b, n):
        seqs = [(_rand(90 + n, n), 5, 8)]
        blk = block(seqs)
        assert blk[-1] == 0 and blk[:-1] == block(seqs, raw_tail=False)
        return b.comp(seqs).case(f"empty_last_sequence_after_{n}_literals")
    return _both(lambda b: one(b, 9)) + _both(lambda b: one(b, 20))


def chunk_cases():
    """Where the compressed bytes fall against the parallel decoder's walk chunk."""
    ch = geometry()["chunk"]
    out = []
    for k in (ch - 1, ch, ch + 1):  # the second token at compressed position k
        seqs = [_sized_seq(100 + k, k, 3, 9), (_rand(101, 6), 11, 7), _tail(8)]
        assert token_positions(seqs)[1] == k
        out += _both(lambda b, s=seqs, k=k: b.comp(s).case(f"token_at_{k}"))
    # a literal-length extension (255, r) on the chunk edge: the token two bytes before it
    seqs = [_sized_seq(110, ch - 2, 5, 6), (_rand(111, 300), 17, 5), _tail(9)]
    assert token_positions(seqs)[1] == ch - 2 and seq_bytes(*seqs[1])[1] == 255
    out += _both(lambda b: b.comp(seqs).case("literal_ext_straddles"))
    # a match-length extension (255, r) on the chunk edge: token, 10 literals, offset, 255 | r
    mseqs = [_sized_seq(112, ch - 14, 5, 6), (_rand(113, 10), 13, 19 + 255 + 30), _tail(10)]
    assert token_positions(mseqs)[1] + 1 + 10 + 2 == ch - 1
    out += _both(lambda b: b.comp(mseqs).case("match_ext_straddles"))
    # the two offset bytes on the chunk edge (offset >= 256: both bytes count)
    oseqs = [(_rand(114, 8), 8, 400), _sized_seq(115, ch - 24, 2, 5)]
    oseqs.append((_rand(116, ch - 2 - token_positions(oseqs + [(b"", None, 0)])[2]), 0x0123, 9))
    oseqs.append(_tail(11))
    t2 = token_positions(oseqs)[2]
    assert t2 + 1 + len(oseqs[2][0]) == ch - 1 and len(oseqs[2][0]) < 15
    out += _both(lambda b: b.comp(oseqs).case("offset_straddles"))
    # a literal run that jumps over whole chunks (their entry[] stays unset), tokens after it
    jseqs = [(_rand(117, 6), 4, 8), (_rand(118, 4 * ch - 6), 100, 40), (_rand(119, 3), 2, 70),
             _tail(12)]
    t = token_positions(jseqs)
    assert t[1] // ch == 0 and t[2] // ch >= 3
    out += _both(lambda b: b.comp(jseqs).case("literals_skip_chunks"))
    # the densest token stream: (no literals, match 4), three compressed bytes a sequence
    dseqs = [(_rand(120, 8), 8, 4)] + [(b"", 1 + (7 * i) % 11, 4) for i in range(600)] + [_tail(13)]
    assert len(block(dseqs)) > 20 * ch
    out += _both(lambda b: b.comp(dseqs).case("dense_tokens"))
    return out


def _block_of_csize(seed, csize):
    """Sequences of a block of exactly ``csize`` compressed bytes: 16-byte sequences (13 random
    literals, a 5-byte match), the first and the last run sized to land on ``csize``."""
    n = (csize - 80) // 16
    mid = [(_rand(seed + 1 + i, 13), 13, 5) for i in range(n)]
    for l0 in range(13, 60):
        for lt in range(TAIL, 60):
            first, last = (_rand(seed, l0), 3, 5), _tail(seed + 7, lt)
            if len(seq_bytes(*first)) + 16 * n + len(seq_bytes(*last)) == csize:
                seqs = [first] + mid + [last]
                assert len(block(seqs)) == csize
                return seqs
    raise AssertionError(csize)


def size_gate_cases():
    """The parallel decoder's gates: a compressed block of LZ_PAR_CMAX - 1 / + 0 / + 1 bytes
    (LZ4 expands by at most ~0.4 %, so all three decode past LZ_PAR_MAX: the first two enter the
    parallel kernel and leave it for the sequential one, the third never enters), stored blocks
    of LZ_PAR_MAX and + 1 bytes in a linked frame, a zero-length stored block."""
    g = geometry()
    pm, cm = g["par_max"], g["par_cmax"]
    out = []
    for cs in (cm - 1, cm, cm + 1):
        seqs = _block_of_csize(200 + cs, cs)
        out += _both(lambda b, s=seqs, cs=cs: b.comp([_tail(14, 40)]).comp(s).comp(
            [(_rand(15, 20), 20, 30), _tail(15)]).case(f"csize_{cs}"))
    for n in (pm, pm + 1):
        b = Builder(True).stored(_rand(220 + n, n)).comp([(_rand(16, 3), n, 60), _tail(17)])
        out.append(b.case(f"stored_{n}"))
    out += _both(lambda b: b.stored(b"").comp([(_rand(18, 9), 4, 30), _tail(19)]).case(
        "zero_length_stored_block"))
    return out


def staging_cases():
    """The compressed block's address modulo 16 (16-byte loads or the byte path of lz_stage, per
    1 KB wave slice): a stored block of r bytes, a compressed block of more than 3 KB (all four
    slices stage), a short block after it."""
    pm = geometry()["par_max"]
    out = []
    for r in range(16):
        def build(b, r=r):
            b.stored(_rand(300 + r, r))
            seqs = [(_rand(320 + r, 1500), 700, 200), (_rand(340 + r, 1600), 1, 100), _tail(20, 50)]
            assert 3072 < len(block(seqs)) and 1500 + 200 + 1600 + 100 + 50 <= pm
            b.comp(seqs).comp([(_rand(21, 2), 2 if not b.linked else 1000, 25), _tail(22)])
            c = b.case(f"second_block_at_{r}")
            assert (header(c.frame).data_pos + 4 + r + 4) % 16 == (23 + r) % 16
            return c
        out += _both(build)
    return out


def linked_par_cases():
    """Linked frames whose every block fits the parallel decoder: references into earlier blocks
    (LZ_EXT), placed and resolved over the whole frame."""
    pm = geometry()["par_max"]
    out = []
    b = Builder(True).comp([_tail(30, 100)]).comp([(_rand(31, 3), 103, 50), _tail(32)])
    out.append(b.case("match_reaches_frame_byte_0"))
    b = Builder(True)
    for i in range(16):
        b.stored(_rand(400 + i, 65536 // 16))
    assert 65536 // 16 <= pm and len(b.out) == 65536
    b.comp([(b"", 65535, 100), _tail(33)])
    out.append(b.case("offset_65535_over_16_stored_blocks"))
    b = Builder(True).comp([_tail(34, 50)]).comp([(b"", 10, 40), _tail(35)])
    out.append(b.case("match_runs_on_into_its_block"))
    b = Builder(True).comp([_tail(36, 100)])
    for i in range(47):  # block i + 1: a copy of block i, five literals: a chain 47 blocks deep
        n = 100 + TAIL * i
        b.comp([(b"", n, n), _tail(500 + i)])
    assert len(b.blocks) == 48
    out.append(b.case("chain_47_blocks_deep"))
    return out


def linked_seq_cases():
    """Linked frames with a block above LZ_PAR_CMAX (one workgroup, the 64 KB LDS ring): the
    largest offset and the shortest ones across the ring's wrap.  The first block is STORED:
    liblz4 refuses a compressed block above the frame's 64 KB block maximum."""
    out = []
    for lead in (0, 1, 2):  # the match starts at output position 65535 + lead
        b = Builder(True).stored(_rand(600 + lead, 65535))
        b.comp([(_rand(610 + lead, lead), 65535, 130 + lead), _tail(40)])
        out.append(b.case(f"offset_65535_at_{65535 + lead}"))
    for off in (1, 2, 3):
        b = Builder(True).stored(_rand(620 + off, 65500))
        b.comp([(_rand(630 + off, 3), off, 200), _tail(41)])
        assert len(b.out) > 65536 + 100
        out.append(b.case(f"offset_{off}_across_the_wrap"))
    return out


def _option_body(b):
    b.comp([(_rand(50, 40), 7, 90), _tail(51, 9)])
    b.stored(_rand(52, 33))
    return b.comp([(_rand(53, 5), 3 if not b.linked else 60, 500), _tail(54)])


def frame_option_cases():
    """Block checksums, a content checksum, both; and no content size."""
    out = []
    for bc, cc in ((True, False), (False, True), (True, True)):
        out += _both(lambda b, bc=bc, cc=cc: _option_body(b).case(
            f"checksums_block{int(bc)}_content{int(cc)}", block_checksum=bc, content_checksum=cc))
    out += _both(lambda b: _option_body(b).case("no_content_size", size=False))
    return out


SMALL_LENGTHS = tuple(range(1, 21)) + (63, 64, 65, 4095, 4096, 4097)


def liblz4_small_cases():
    """liblz4's own parse of small inputs, compressible and random."""
    from oracle import lz4 as olz4
    out = []
    if not olz4.available():  # (the modules that use the tables skip as a whole without liblz4)
        return out
    for n in SMALL_LENGTHS:
        for kind, data in (("text", (b"abcab" * (n // 5 + 1))[:n]), ("random", _rand(700 + n, n))):
            for linked in (True, False):
                out.append(Case(f"liblz4_{kind}_{n}-{'linked' if linked else 'indep'}",
                                olz4.ref_compress(data, block_linked=linked), data))
    return out


def liblz4_large_block_frames():
    """liblz4's frames with 256 KB, 1 MB and 4 MB blocks: not supported, refused cleanly."""
    from oracle import lz4 as olz4
    if not olz4.available():
        return []
    data = (_rand(800, 700) * 100)[:70_000]
    return [Case(f"liblz4_block_size_id_{i}", olz4.ref_compress(data, block_size_id=i), data)
            for i in (5, 6, 7)]


VALID_FAMILIES = collections.OrderedDict([
    ("run_length", run_length_cases), ("length_codes", length_code_cases),
    ("chunks", chunk_cases), ("size_gates", size_gate_cases), ("staging", staging_cases),
    ("linked_par", linked_par_cases), ("linked_seq", linked_seq_cases),
    ("frame_options", frame_option_cases), ("liblz4_small", liblz4_small_cases)])


def valid_sample(step=7):
    """Every ``step``-th case of EVERY family, the first of each included."""
    fams = collections.OrderedDict()
    for c in valid_cases():
        fams.setdefault(c.name.split("/")[0], []).append(c)
    assert list(fams) == list(VALID_FAMILIES)
    return tuple(c for cases in fams.values() for c in cases[::step])


@functools.lru_cache(maxsize=None)
def valid_cases():
    out = []
    for fam, fn in VALID_FAMILIES.items():
        out += [Case(f"{fam}/{c.name}", c.frame, c.expected) for c in fn()]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


# ---- decoder: malformed frames -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def malformed_cases():
    """Frames every decoder must refuse (expected is None).  Each names the check in
    csrc/dpz_lz4.hip it relies on: S = the sequential lz4_decode_kernel, P = lz_parse_at / the
    steps of lz4_decode_par_kernel, H = the host's dpz_lz4_frame_info / dpz_lz4_decompress."""
    lit = _rand(900, 20)
    tail = _tail(901)
    out = []

    def add(name, blocks, linked=False, size=None, **kw):
        out.append(Case(name, frame(blocks, linked, size, **kw), None))

    for linked in (False, True):
        w = "linked" if linked else "indep"
        # 1. the last sequence carries a match.  S: `if (ip >= cs) bad` at the next token.
        # P, nibble form (9 literals, match 8: the token 0x94 has no 15 in it): step 1's fast
        # path, `ip + 2 >= cs ? LZ_BAD`.  P, 20 literals (the token's literal nibble is 15) and
        # the match-length extension byte that ends the block: both positions are LZ_SLOW, so
        # lz_parse_at's `if (ip >= cs) return q` (kind 2 -> LZ_BAD).  Either way no sequence with
        # a match ends the block, and step 3 finds no chain to cs.
        add(f"match_ends_block_nibble-{w}", [block([(lit[:9], 5, 8)], raw_tail=False)], linked)
        add(f"match_ends_block_long_literals-{w}", [block([(lit, 5, 8)], raw_tail=False)], linked)
        add(f"match_ends_block_extension-{w}", [block([(lit, 5, 30)], raw_tail=False)], linked)
    # 2. offset 0.  S: `off == 0`.  P: step 6 `q.off == 0`.
    add("offset_0", [block([(lit, 0, 8), tail])])
    # 3. one past the history of an independent frame's first block.  S: `off > hist` with
    # hist = opos - start.  P: step 6 `!linked && q.off > o + q.L`.
    add("offset_past_block_start", [block([(lit, 21, 8), tail])])
    # 4. one before the frame's start, from the third block of a linked frame.  S: `off > hist`
    # with hist = opos.  P: lz4_link_place_kernel's `s < 0`.
    add("offset_before_frame_start",
        [block([_tail(902, 30)]), block([_tail(903, 30)]), block([(lit[:4], 65, 8), tail])], True)
    # 5. a length extension of 255s that runs to the block's end.  S: `if (ip >= cs) bad` inside
    # both extension loops.  P: lz_parse_at's `ip >= cs` in its loops (kind 2 -> LZ_BAD).
    add("literal_extension_runs_out", [bytes([0xF0]) + b"\xff" * 12])
    add("match_extension_runs_out", [bytes([0x3F]) + lit[:3] + b"\x02\x00" + b"\xff" * 12])
    # 6. a literal run one byte past the block.  S: `ip + L > cs`.  P: step 1's `ip > cs ?
    # LZ_BAD` (lz_parse_at's `ip + L > cs` for extended lengths).
    add("literals_past_block", [bytes([0xA0]) + lit[:9]])
    add("long_literals_past_block", [bytes([0xF0, 0x05]) + lit[:19]])
    # 7. a content size one more / one less than the blocks decode to.  H: dpz_lz4_decompress's
    # `cs >= 0 && tot != cs`.
    good = [block([(lit, 5, 8), tail])]
    n = len(lit) + 8 + TAIL
    add("content_size_plus_1", good, size=n + 1)
    add("content_size_minus_1", good, size=n - 1)
    # 8. no end mark.  H: dpz_lz4_frame_info's `nbytes < pos + 4` in its block walk.
    add("end_mark_missing", good, size=n, end_mark=False)
    # 9. a block size field larger than the bytes that remain.  H: dpz_lz4_frame_info's
    # `pos > nbytes` after each block.
    f = bytearray(frame(good, False, n))
    at = header(f).data_pos
    f[at:at + 4] = struct.pack("<I", len(good[0]) + 8)
    out.append(Case("block_size_past_frame", bytes(f), None))
    return tuple(out)


# ---- encoder inputs ------------------------------------------------------------------------
def encoder_lengths():
    g = geometry()
    blk, win = g["blk"], g["win"]
    return tuple(range(1, 14)) + (blk - 1, blk, blk + 1, blk + MFLIMIT - 1, blk + MFLIMIT,
                                  blk + MFLIMIT + 1, 2 * blk, win - 1, win, win + 1,
                                  win + blk - 1, win + blk, win + blk + 1, 65536 + 7)


def _periodic(seed, period, n):
    p = _rand(seed, period)
    return (p * (n // period + 1))[:n]


def _runs_between_copies(n):
    """Copies of earlier content with random literal runs of 14 / 15 / 16 / 270 between them."""
    base = _rand(1000, 96)
    out = bytearray(base)
    i = 0
    while len(out) < n:
        out += _rand(1001 + i, (14, 15, 16, 270)[i % 4])
        s = (37 * i) % (len(base) - 40)
        out += base[s:s + 40 + i % 9]
        i += 1
    return bytes(out[:n])


def _stored_between(n):
    """An incompressible block between compressible ones, the blocks after it matching into it."""
    blk = geometry()["blk"]
    noise = np.random.default_rng(1100).integers(0, 256, blk, dtype=np.uint8).tobytes()
    out = _periodic(1101, 5, blk) + noise
    while len(out) < n:
        out += noise[100:700] + _periodic(1102, 3, 300) + noise[900:1600]
    return out[:n]


def encoder_contents():
    """name -> f(n): the first n bytes of a content."""
    g = geometry()
    blk, win = g["blk"], g["win"]
    out = collections.OrderedDict()
    out["constant"] = lambda n: b"\xC3" * n
    for p in (2, 3, 5, 7):
        out[f"period_{p}"] = lambda n, p=p: _periodic(1200 + p, p, n)
    for p in (blk - 1, blk, blk + 1):  # the match sits one block back
        out[f"period_{p}"] = lambda n, p=p: _periodic(1300 + p, p, n)
    for p in (win, win + 64):  # at, and just past, what the history reaches
        out[f"period_{p}"] = lambda n, p=p: _periodic(1400 + p, p, n)
    out["repeat_3000"] = lambda n: _periodic(1500, 3000, n)  # longer than the match cap
    out["runs_between_copies"] = _runs_between_copies
    out["stored_between"] = _stored_between
    return out


SHORT_PERIODS = ("period_2", "period_3", "period_5", "period_7")


def constant_block(blk):
    """What the encoder's rules give for a full block of a constant byte whose history holds the
    same byte: a match at every position, each taken as long as the cap (MAXM) and the last five
    literals (mend = len - 5) allow, no match starting past len - 12.  For blk = 2048: matches of
    1024 and 1019 (2043 = 2048 - 5 > 2036 = 2048 - 12 ends the search), five literals: three
    sequences of 7 + 7 + 6 = 20 bytes.  Returns (number of sequences, compressed bytes)."""
    seqs, p = [], 0
    while p <= blk - MFLIMIT:
        m = min(blk - LASTLIT - p, MAXM)
        seqs.append((b"", 1, m))
        p += m
    seqs.append((b"\xC3" * (blk - p), None, 0))
    return len(seqs), len(block(seqs))


def check_encoder_frame(frm, n):
    """What the device encoder promises about its frames, read off ``walk``."""
    g = geometry()
    blk, win = g["blk"], g["win"]
    h = header(frm)
    assert h.linked and h.content_size == n and not h.block_checksum and not h.content_checksum
    blocks = walk(frm)
    assert len(blocks) == -(-n // blk)
    start = 0
    for i, b in enumerate(blocks):
        assert b.decoded_len == (blk if i + 1 < len(blocks) else n - start), (i, b.decoded_len)
        if not b.raw:  # stored iff the compressed form is no shorter: a compressed one is shorter
            assert b.csize < b.decoded_len, (i, b.csize, b.decoded_len)
            p = 0
            for L, off, M in b.seqs:
                p += L
                if off is None:
                    continue
                assert MINMATCH <= M <= MAXM, (i, p, M)
                assert 1 <= off <= min(start, win) + p, (i, p, off)
                assert p <= b.decoded_len - MFLIMIT and p + M <= b.decoded_len - LASTLIT, (i, p, M)
                p += M
            assert p == b.decoded_len
        start += b.decoded_len
    return blocks
