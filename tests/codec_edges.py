"""Case builders for the payload codecs' structural edges — numpy only (no torch, no GPU).

Elias-gamma index arrays (csrc/dpz_elias.hip: 1024 codes per encode block, 1024 bits per decode
chunk, 64 chunks per super map, 16 super maps per resolve pass, 1024 chunks per scan pass), fp32
blocks of a chosen exponent width (csrc/dpz_fpz.hip: 256 values per block, width =
bit_length(emax - emin)) and the fp32 vector that pins round-to-nearest-even to half
(csrc/dpz_misc.hip).  The case lists are shared by the fixture generator
(tests/golden/make_golden_elias_edges.py) and the CPU and GPU edge tests.
"""
import numpy as np

INT32_END = 2 ** 31          # every index is below this
CHUNK = 1024                 # decode chunk, bits
FIRSTS = (0xC8, 0x01A2B3C4)  # >= 128 and >= 2^24: trailer bytes next to the code bits non-zero


# --------------------------------------------------------------------------------------- Elias
def from_gaps(gaps, first=0):
    g = np.asarray(gaps, dtype=np.int64)
    assert g.size >= 1 and g.min() >= 1
    a = np.concatenate([[first], first + np.cumsum(g)])
    assert a[-1] < INT32_END, "last index must stay below 2^31"
    return a.astype(np.int32)


def code_bits(idx):
    """Code bits L of an index array (sum of 2 * floor(log2 gap) + 1), in integer arithmetic."""
    g = np.diff(np.asarray(idx, dtype=np.int64))
    return sum(2 * (int(v).bit_length() - 1) + 1 for v in g.tolist())


def ones(L, first=0):
    """L one-bit codes: k = L + 1 consecutive indices."""
    return from_gaps(np.ones(L, dtype=np.int64), first)


def _filled_gaps(L, l):
    clen = 2 * l + 1
    n = L // clen
    alt = np.where(np.arange(n) % 2 == 0, 2 ** l, 2 ** (l + 1) - 1).astype(np.int64)
    tail = np.ones(L - n * clen, dtype=np.int64)
    return n, alt, tail


def filled_fits(L, l, first=0):
    n, _, tail = _filled_gaps(L, l)
    return first + n * 2 ** l + tail.size < INT32_END


def filled(L, l, first=0):
    """As many (2l+1)-bit codes as fit into L bits (gaps alternating 2^l and 2^(l+1) - 1 where
    the index sum allows, else constant 2^l), then one-bit codes up to exactly L bits.  1024 is
    no multiple of 2l+1, so the chunk entry offset moves from chunk to chunk."""
    n, alt, tail = _filled_gaps(L, l)
    if first + int(alt.sum()) + tail.size >= INT32_END:
        alt = np.full(n, 2 ** l, dtype=np.int64)
    return from_gaps(np.concatenate([alt, tail]), first)


def straddle_gap(l, which):
    """A gap of code length 2l+1: the smallest, the largest, or one in between."""
    lo, hi = 2 ** l, 2 ** (l + 1) - 1
    return (lo, hi, lo | (0x2AAAAAAA & (lo - 1)))[which % 3]


def straddle(l, s, which=None, first=0):
    """1024 - s one-bit codes, one (2l+1)-bit code that begins s bits before the first chunk
    edge (1 <= s <= 2l+1), then 40 one-bit codes."""
    assert 0 <= l <= 30 and 1 <= s <= 2 * l + 1
    g = straddle_gap(l, s if which is None else which)
    g = min(g, INT32_END - 1 - first - (CHUNK - s) - 40)  # l = 30: the last index is 2^31 - 1
    assert g.bit_length() == l + 1
    return from_gaps(np.concatenate([np.ones(CHUNK - s, np.int64), [g], np.ones(40, np.int64)]),
                     first)


def straddle_bits(l, s):
    return CHUNK - s + 2 * l + 1 + 40


def ramp(ncodes, first=0):
    """Gaps 1 + (i mod 7): code lengths 1, 3, 3, 5, 5, 5, 5.  1024 of them are 3946 bits and
    3946 mod 32 = 10, so encode blocks end in mid-word and neighbours share boundary words."""
    return from_gaps(1 + np.arange(ncodes, dtype=np.int64) % 7, first)


def pow2_edges():
    """Gaps 2^l - 1, 2^l, 2^l + 1 for l = 1..30, split greedily over as many streams as the 2^31
    bound needs; the last stream (the 61-bit code of gap 2^30 + 1) gets the ``first`` that puts
    its last index on 2^31 - 1 exactly."""
    gaps = [g for l in range(1, 31) for g in (2 ** l - 1, 2 ** l, 2 ** l + 1)]
    streams, cur = [], []
    for g in gaps:
        if sum(cur) + g >= INT32_END:
            streams.append(cur)
            cur = []
        cur.append(g)
    streams.append(cur)
    out = [from_gaps(s) for s in streams[:-1]]
    out.append(from_gaps(streams[-1], first=INT32_END - 1 - sum(streams[-1])))
    assert int(out[-1][-1]) == INT32_END - 1
    return out


def three_59(first=0):
    """Three back-to-back 59-bit codes (gap 2^29)."""
    return from_gaps([2 ** 29] * 3, first)


def one_61(first=0):
    """The single 61-bit code: [first, 2^31 - 1]."""
    return np.array([first, INT32_END - 1], dtype=np.int32)


ENCODE_COUNTS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 37)


def elias_encode_cases():
    """(name, indices) of every encode case: all residues of L mod 32 (the trailer in every byte
    lane of the word it shares with the last code bits), the encode block edges, mid-word block
    ends, the longest codes, and the same shapes with a non-zero ``first``."""
    cases = [(f"ones_L{L}", ones(L)) for L in range(1, 131)]
    cases += [(f"ones_n{n}", ones(n)) for n in ENCODE_COUNTS if n > 130]
    cases += [(f"ramp_n{n}", ramp(n)) for n in ENCODE_COUNTS]
    cases += [(f"pow2_{i}", a) for i, a in enumerate(pow2_edges())]
    cases += [("three_59", three_59()), ("one_61", one_61())]
    for f in FIRSTS:
        cases += [(f"ones_L{L}_first{f}", ones(L, f)) for L in (1, 7, 8, 9, 24, 25, 31, 32, 33)]
        cases += [(f"ones_n{n}_first{f}", ones(n, f)) for n in (1023, 1024, 1025)]
        cases += [(f"ramp_n{n}_first{f}", ramp(n, f)) for n in (1, 5, 1024, 1025, 3 * 1024 + 37)]
        cases += [(f"three_59_first{f}", three_59(f)), (f"one_61_first{f}", one_61(f)),
                  (f"straddle_l15_s16_first{f}", straddle(15, 16, first=f))]
    return cases


DECODE_LS = (1, 2, 3, 7, 15, 19)
DECODE_BITS = (1023, 1024, 1025, 2047, 2048, 2049, 65535, 65536, 65537,
               2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1)


def elias_decode_size_cases():
    """(name, L, l) of the decode-only size cases (l = 0: ``ones``): the chunk edge, the
    super-map edge and 16 super maps = 1024 chunks, for every code length whose indices fit."""
    cases = [(f"ones_L{L}", L, 0) for L in DECODE_BITS]
    cases += [(f"filled_L{L}_l{l}", L, l) for l in DECODE_LS for L in DECODE_BITS
              if filled_fits(L, l)]
    return cases


def build_size_case(L, l):
    return ones(L) if l == 0 else filled(L, l)


GOLDEN_STRADDLE_LS = (0, 1, 15, 29, 30)


def golden_small_cases():
    """name -> indices of the fixture's small cases (L <= 70 000 bits; input, reference bytes and
    reference decode are stored)."""
    cases = {f"ones_L{L}": ones(L)
             for L in (1, 31, 32, 33, 1023, 1024, 1025, 65535, 65536, 65537)}
    cases["filled_L65537_l3"] = filled(65537, 3)
    cases["filled_L67584_l15"] = filled(67584, 15)
    for l in GOLDEN_STRADDLE_LS:
        for s in sorted({1, l + 1, 2 * l + 1}):
            cases[f"straddle_l{l}_s{s}"] = straddle(l, s)
    cases["ramp_n1025"] = ramp(1025)
    cases[f"ramp_n{3 * 1024 + 37}"] = ramp(3 * 1024 + 37)
    for i, a in enumerate(pow2_edges()):
        cases[f"pow2_{i}"] = a
    return cases


def golden_large_cases():
    """name -> indices of the fixture's large cases (only the sha256 of the reference's bytes and
    the value count are stored)."""
    return {"ones_L1048575": ones(2 ** 20 - 1), "ones_L1048576": ones(2 ** 20),
            "ones_L1048577": ones(2 ** 20 + 1), "filled_L1048577_l1": filled(2 ** 20 + 1, 1),
            "filled_L1048576_l2": filled(2 ** 20, 2)}


def golden_bits(name):
    """The code bits a fixture case is built to have (None: not stated in its name)."""
    parts = name.split("_")
    if parts[0] in ("ones", "filled"):
        return int(parts[1][1:])
    if parts[0] == "straddle":
        return straddle_bits(int(parts[1][1:]), int(parts[2][1:]))
    return None


# ----------------------------------------------------------------------------------------- fpz
FPZ_SPANS = (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 254, 255)
FPZ_EMINS = (0, 1, 127)
FPZ_COUNTS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 255, 256)
FPZ_PRECISIONS = (0, 1, 8, 9, 10, 11, 16, 31, 32, 40)


def block(cnt, emin, span, seed):
    """``cnt`` fp32 bit patterns (uint32) whose exponents are uniform in [emin, emin + span], with
    elements 0 and -1 pinned to the two ends; random signs and 23-bit mantissas.  Exponent 0
    gives denormals, exponent 255 Inf / NaN."""
    assert 1 <= cnt <= 256 and 0 <= emin and emin + span <= 255
    rng = np.random.default_rng(seed)
    e = rng.integers(emin, emin + span + 1, size=cnt).astype(np.uint32)
    e[0] = emin
    e[-1] = emin + span
    sign = rng.integers(0, 2, size=cnt).astype(np.uint32)
    mant = rng.integers(0, 2 ** 23, size=cnt).astype(np.uint32)
    return ((sign << 31) | (e << 23) | mant).astype(np.uint32)


def block_width(cnt, span):
    """The exponent width a ``block`` is built to get at precision 0 (one value: one exponent)."""
    return 0 if cnt == 1 else int(span).bit_length()


def fpz_block_cases():
    """(name, cnt, emin, span, bits) for every count, span and the exponent bases it allows."""
    cases = []
    for span in FPZ_SPANS:
        for emin in FPZ_EMINS:
            if emin + span > 255:
                continue
            for cnt in FPZ_COUNTS:
                seed = (span * 256 + emin) * 512 + cnt
                cases.append((f"c{cnt}_e{emin}_s{span}", cnt, emin, span,
                              block(cnt, emin, span, seed)))
    return cases


def stream(blocks):
    return np.concatenate(blocks).astype(np.uint32)


def mixed_stream(nblk, last_cnt, seed):
    """``nblk`` blocks of different widths back to back (spans and bases cycle), the last one of
    ``last_cnt`` values."""
    blocks = []
    for b in range(nblk):
        span = FPZ_SPANS[(b + seed) % len(FPZ_SPANS)]
        ok = [e for e in FPZ_EMINS if e + span <= 255]
        emin = ok[(b // len(FPZ_SPANS)) % len(ok)]
        cnt = last_cnt if b == nblk - 1 else 256
        blocks.append(block(cnt, emin, span, seed * 4099 + b))
    return stream(blocks)


def fpz_stream_cases():
    """(name, bits): 1 block; one grid block of 4 waves - 1, exact and + 1; one scan pass of 1024
    blocks + 1; full and short last blocks."""
    return [("b1_full", mixed_stream(1, 256, 1)), ("b1_short", mixed_stream(1, 77, 2)),
            ("b3_short", mixed_stream(3, 255, 3)), ("b4_full", mixed_stream(4, 256, 4)),
            ("b4_short", mixed_stream(4, 1, 5)), ("b5_full", mixed_stream(5, 256, 6)),
            ("b5_short", mixed_stream(5, 33, 7)), ("b1025_short", mixed_stream(1025, 5, 8)),
            ("b1025_full", mixed_stream(1025, 256, 9))]


def topmask(p):
    """Mask of the top ``p`` bits of a 32-bit pattern (0 or >= 32: all of them)."""
    return 0xFFFFFFFF if p == 0 or p >= 32 else (0xFFFFFFFF << (32 - p)) & 0xFFFFFFFF


def fpz_expected_bits(u, p):
    """The float codec's contract, stated without the format: the top ``p`` bits of every bit
    pattern; from p = 10 on a NaN whose kept mantissa is zero also gets the quiet bit."""
    u = np.asarray(u, dtype=np.uint32)
    t = u & np.uint32(topmask(p))
    if 10 <= p < 32:
        nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
        t = np.where(nan & ((t & 0x007FFFFF) == 0), t | np.uint32(0x00400000), t)
    return t.astype(np.uint32)


# ---------------------------------------------------------------------------------------- fp16
def fp16_all_patterns():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16)


def fp16_tie_vector():
    """fp32 inputs that pin round-to-nearest-even to half: the midpoint of every pair of adjacent
    finite halves of either sign (exact in fp32) and its two fp32 neighbours, the pairs
    (0, 2^-24) and (65504, 65536) included, so 2^-25 and 65520 with their neighbours are there."""
    h = np.arange(0x7C00, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)
    grid = np.concatenate([h, np.array([65536.0], dtype=np.float32)])  # 0 .. 65504, 65536
    mid = ((grid[:-1].astype(np.float64) + grid[1:].astype(np.float64)) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64) * 2,
                          grid[:-1].astype(np.float64) + grid[1:].astype(np.float64))
    below = np.nextafter(mid, np.float32(-np.inf))
    above = np.nextafter(mid, np.float32(np.inf))
    pos = np.stack([below, mid, above], axis=1).ravel()
    return np.concatenate([pos, -pos]).astype(np.float32)


def fp16_vector():
    """Every half pattern widened to fp32, the tie vector, +-Inf, NaNs of three payloads,
    +-FLT_MAX and fp32 denormals."""
    with np.errstate(invalid="ignore"):
        wide = fp16_all_patterns().view(np.float16).astype(np.float32)
    spec = np.array([0x7F800000, 0xFF800000, 0x7F800001, 0x7FC00000, 0xFFFFFFFF,
                     0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                     0x00400000, 0x80400000], dtype=np.uint32).view(np.float32)
    return np.concatenate([wide, fp16_tie_vector(), spec]).astype(np.float32)


def fp16_expected(x):
    """numpy's software round-to-nearest-even, the same on every machine (uint16 patterns)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


# ------------------------------------------------------------------------------------- fixture
def sha256(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


_GOLDEN = None


def load_golden():
    """(small, large) of tests/golden/elias_edges.{npz,json}, recorded from the unmodified
    reference.  small: dicts with name, input, bytes and decoded (the three cases stored as
    digests rebuild their input here, check it against its digest and carry ``decoded_sha256``
    with ``decoded`` None).  large: dicts with name, input (rebuilt), k, nbytes, sha256."""
    global _GOLDEN
    if _GOLDEN is None:
        import json
        import os
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        arrays = dict(np.load(os.path.join(here, "elias_edges.npz")))
        with open(os.path.join(here, "elias_edges.json")) as f:
            meta = json.load(f)
        built = golden_small_cases()
        small = []
        for rec in meta["small"]:
            name = rec["name"]
            c = dict(rec, bytes=arrays[f"{name}_bytes"], decoded=None)
            if "input_sha256" in rec:
                c["input"] = built[name]
                assert sha256(c["input"]) == rec["input_sha256"], name
            else:
                c["input"] = arrays[f"{name}_input"]
                c["decoded"] = arrays[f"{name}_decoded"]
            small.append(c)
        built = golden_large_cases()
        large = [dict(rec, input=built[rec["name"]]) for rec in meta["large"]]
        _GOLDEN = (small, large)
    return _GOLDEN
