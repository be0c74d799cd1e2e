"""Case builders for the sparse fold's structural edges — numpy only (no torch, no GPU).

The receive-side fold (dpz_decode_average: csrc/dpz_fold.hip, dpz_fold_tile.hip,
dpz_fold_walk.hip, dpz_fold_merge.hip, dpz_fold_patch.hip, dpz_replace.h) branches on exact
counts: entries of one payload in one tile against a 64- / 128-entry window, a tile's entry total
against the classic kernel's preload and hit-chain capacities, a wave's hit total against its
value slots, an element's hit count against the 2- / 3-hit fast paths.  Every builder here states
its shape in those constants and returns

    Case(name, n, local, payloads, weights, w_self, flags)

with payloads a list of (sorted unique int32 idx, fp32 vals).  flags is a dict: what the case
claims about itself ("claims", recomputed from the arrays by tests/test_cpu_fold_edges.py), the
flag variants it runs under ("variants"), element offsets of the device views ("local_off",
"idx_off", "val_off") and "nan" (NaN inputs: compared by position).  The case lists are shared by
tests/test_cpu_fold_edges.py and tests/test_gpu_fold_edges.py.
"""
import collections
import functools
import itertools
import zlib

import numpy as np

from oracle import fold as ofold

# ---- the engines' constants (the library exports none of them; dpz_debug_fold_plan reports the
# chosen epl / ept only) -----------------------------------------------------------------------
FOLD_TILE = 4096            # csrc/dpz_fold.h:12        FOLD_TILE = 1 << DPZ_FOLD_TS (12)
FOLD_MAXP = 16              # csrc/dpz_fold.h:13        payloads per launch, longer lists chained
FG_CAP = 6144               # csrc/dpz_fold.h:15        4-slot group kernel: entries per round
FOLD_PRELOAD = 2048         # csrc/dpz_fold_tile.hip:29,33  FOLD_THREADS (512) * FOLD_EQ (4)
FOLD_POOL = 64              # csrc/dpz_fold_tile.hip:34 hit-chain path: rows of >= 3-hit elements
FOLD_CAP = 2816             # csrc/dpz_fold_tile.hip:39 FOLD_TILE / 16 * 11: hit-chain capacity
FM_THREADS = 256            # csrc/dpz_fold_merge.hip:28    merge TE = 256 * EPT, WE = 64 * EPT
MERGE_MIN_N = 1024          # csrc/dpz_fold.hip:84      merge_ok: n >= 1024
WALK_VEC_MIN_N = 1024       # csrc/dpz_fold.hip:101     the walk's float4 build: n >= 1024
WINDOW = 64                 # csrc/dpz_fold_cursor.h:10 fw_lead: a window is one wave of entries
PT_CAP = 1024               # csrc/dpz_fold_patch.hip:64    patch: entries staged per pass
RP_E = 16                   # csrc/dpz_replace.h:18     replace: payload entries per chunk

# dpz_debug_fold_plan's engine codes (include/dpz_codec.h DPZ_FOLD_ENGINE_*)
NONE, CLASSIC, GROUP, WALK, WALK_GROUPS, MERGE, REPLACE, PATCH1, PATCH = 0, 1, 2, 4, 5, 8, 9, 10, 11

Case = collections.namedtuple("Case", "name n local payloads weights w_self flags")


def merge_te(ept):
    return FM_THREADS * ept


def merge_we(ept):
    return 64 * ept


def merge_wave_elems(ept, wave):
    """Tile-relative elements of wave `wave` (fm_elem, csrc/dpz_fold_merge.hip:39: thread t's
    element e is (e / 4) * 1024 + 4 t + e % 4, threads 64 wave .. 64 wave + 63)."""
    return np.concatenate([c * 4 * FM_THREADS + 256 * wave + np.arange(256)
                           for c in range(ept // 4)])


def merge_wave_of(ept, rel):
    """Wave that owns tile-relative element(s) rel."""
    return (np.asarray(rel) % (4 * FM_THREADS)) // 256


# ---- the engines a case runs on ---------------------------------------------------------------
# name -> (environment of the diagnostic build, tile T, plan engines that count as "ran as named").
# The block-count switches make one block (the walk: four waves) cover every tile, so look-ahead
# loads, the LDS double buffer and the cursor carry are exercised at these sizes.
Engine = collections.namedtuple("Engine", "name env T family engines")


def _walk(epl, win=64, dist=3):
    name = f"walk-epl{epl}" + ("" if (win, dist) == (64, 3) else f"-w{win}-d{dist}")
    return Engine(name, {"DPZ_FOLD_KIND": "4", "DPZ_FOLD_WALK_EPL": str(epl), "DPZ_FOLD_WIN": str(win),
                         "DPZ_FOLD_DIST": str(dist), "DPZ_WALK_BLOCKS": "1"},
                  64 * epl, "walk", (WALK, WALK_GROUPS))


ENGINES = collections.OrderedDict((e.name, e) for e in [
    Engine("classic", {"DPZ_FOLD_KIND": "1", "DPZ_FOLD_BLOCKS": "1"}, FOLD_TILE, "classic", (CLASSIC,)),
    Engine("phase", {"DPZ_FOLD_KIND": "1", "DPZ_FOLD_PHASES": "1", "DPZ_FOLD_BLOCKS": "1"},
           FOLD_TILE, "classic", (CLASSIC,)),
    Engine("group", {"DPZ_FOLD_KIND": "2", "DPZ_FOLD_BLOCKS": "1"}, FOLD_TILE, "classic", (GROUP,)),
    _walk(2), _walk(4), _walk(8), _walk(16),
    # window width and look-ahead distance forced (the window-edge cases only)
    _walk(2, 128, 1), _walk(4, 128, 3), _walk(8, 64, 1), _walk(16, 128, 3), _walk(16, 128, 1),
    Engine("merge-ept4", {"DPZ_FOLD_KIND": "8", "DPZ_MERGE_EPT": "4", "DPZ_MERGE_BLOCKS": "1"},
           merge_te(4), "merge", (MERGE,)),
    Engine("merge-ept8", {"DPZ_FOLD_KIND": "8", "DPZ_MERGE_EPT": "8", "DPZ_MERGE_BLOCKS": "1"},
           merge_te(8), "merge", (MERGE,)),
    Engine("merge-ept16", {"DPZ_FOLD_KIND": "8", "DPZ_MERGE_EPT": "16", "DPZ_MERGE_BLOCKS": "1"},
           merge_te(16), "merge", (MERGE,)),
    Engine("product", None, None, "product", None),   # the product library, nothing forced
])


# ---- flag variants ------------------------------------------------------------------------------
Variant = collections.namedtuple("Variant", "name w_self zero_base also_local accumulate")
ALL_VARIANTS = [Variant("-".join(filter(None, ["self" if s else "server", "zero" if z else "",
                                                "inplace" if a else "", "accum" if c else ""])),
                        s, z, a, c)
                for s, z, a, c in itertools.product((True, False), repeat=4)]
BASIC_VARIANTS = [v for v in ALL_VARIANTS
                  if v.name in ("self", "server", "server-zero", "self-inplace", "server-zero-accum")]


def variants_of(case, engine):
    """The variants `engine` accepts: the walk and the merge fold fresh totals only."""
    vs = ALL_VARIANTS if case.flags.get("variants") == "all" else BASIC_VARIANTS
    if engine.family in ("walk", "merge"):
        vs = [v for v in vs if not v.accumulate]
    return vs


def fold_flags(v):
    return ((0x1 if v.w_self else 0) | (0x4 if v.zero_base else 0) | (0x10 if v.accumulate else 0)
            | (0x20 if v.also_local else 0))


def start_total(case):
    """The running total an accumulate variant continues (normal values)."""
    return _rng(case.name + "/start").standard_normal(case.n).astype(np.float32)


def expected(case, v):
    """The fold of `case` under variant v: oracle.fold, or its zero-base / accumulate
    restatement (the one tests/test_gpu_codec.py::test_fold_paths_forced uses)."""
    w_self = case.w_self if v.w_self else None
    with np.errstate(all="ignore"):
        if not v.zero_base and not v.accumulate:
            return ofold.fold(case.local, case.payloads, case.weights, w_self)
        base = np.zeros(case.n, np.float32) if v.zero_base else case.local
        total = start_total(case) if v.accumulate else None
        for (idx, vals), w in zip(case.payloads, case.weights):
            term = ofold.replace(base, idx, vals) * np.float32(w)
            if total is None:
                total = (np.float32(0) + term) if v.zero_base else term
            else:
                total = total + term
        if total is None:
            total = np.zeros(case.n, np.float32)
        if w_self is not None:
            total = total + case.local * np.float32(w_self)
        return total


def groups_of(case):
    """The launches' payload groups (FOLD_MAXP at a time)."""
    np_ = len(case.payloads)
    return [list(range(b, min(b + FOLD_MAXP, np_))) for b in range(0, max(np_, 1), FOLD_MAXP)]


def expect_plan(case, engine, v, group=0):
    """What dpz_debug_fold_plan must report for group `group` of the case on a forced engine:
    {field: value} (fold_plan, csrc/dpz_fold.hip:51).  Groups after the first continue a total:
    the classic kernel (the group kernel under DPZ_FOLD_KIND=2)."""
    np_ = len(groups_of(case)[group])
    aligned = case.flags.get("local_off", 0) % 4 == 0
    if group > 0 and engine.family != "classic":
        return {"engine": CLASSIC, "offsets": 1}
    if engine.name == "classic":
        return {"engine": CLASSIC, "chains": 1, "offsets": 1, "vec": int(aligned)}
    if engine.name == "phase":
        return {"engine": CLASSIC, "chains": 0, "offsets": 1, "vec": int(aligned)}
    if engine.name == "group":
        return {"engine": GROUP, "offsets": 1, "vec": int(aligned)}
    if engine.family == "walk":
        win, dist = int(engine.env["DPZ_FOLD_WIN"]), int(engine.env["DPZ_FOLD_DIST"])
        return {"engine": WALK if np_ <= 4 else WALK_GROUPS, "offsets": 0,
                "epl": int(engine.env["DPZ_FOLD_WALK_EPL"]),
                "vec": int(aligned and case.n >= WALK_VEC_MIN_N),
                "win": 128 if (np_ > 4 and win == 128) else 64,
                "dist": 3 if (np_ > 12 and dist != 1) else 1}
    if engine.family == "merge":
        eqw = int(all(np.float32(w) == np.float32(case.weights[0]) for w in case.weights[:np_]))
        return {"engine": MERGE, "offsets": 0, "ept": int(engine.env["DPZ_MERGE_EPT"]), "eqw": eqw}
    raise ValueError(engine.name)


PLAN_FIELDS = ("engine", "vec", "epl", "dist", "win", "ept", "eqw", "offsets", "chains")


def plan_of(case, lib, flags, group=0, fresh=None, aligned=None):
    """dpz_debug_fold_plan of one payload group of the case on library `lib` (a ctypes handle;
    the diagnostic build reads its DPZ_* switches from the environment at the call)."""
    import ctypes
    g = groups_of(case)[group]
    ks = [int(case.payloads[p][0].size) for p in g]
    ws = [float(case.weights[p]) for p in g]
    out = (ctypes.c_int * len(PLAN_FIELDS))()
    m = max(len(g), 1)
    if fresh is None:
        fresh = int(group == 0 and not flags & 0x10)
    if aligned is None:
        aligned = case.flags.get("local_off", 0) % 4 == 0
    rc = lib.dpz_debug_fold_plan(case.n, len(g), (ctypes.c_int64 * m)(*ks), (ctypes.c_int * m)(),
                                 (ctypes.c_float * m)(*ws), flags, fresh, int(aligned), out)
    assert rc == 0
    return dict(zip(PLAN_FIELDS, out))


def can_take(case, engine):
    """Whether a forced engine folds the case's first group (else it would run the classic
    kernel under the engine's name: such pairs are never parametrised)."""
    if engine.family == "merge":
        return case.n >= MERGE_MIN_N and case.flags.get("local_off", 0) % 4 == 0
    return True


# ---- builders -----------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


_MAGS = np.array([0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000],
                 dtype=np.uint32)   # 0, smallest / largest subnormal, FLT_MIN, FLT_MAX, inf
SPECIAL_BITS = np.concatenate([_MAGS, _MAGS | np.uint32(0x80000000)])


def _specialise(vals, elems, rng):
    """Half the values replaced by special ones.  FLT_MAX and infinity take their sign from the
    element's parity, so no element ever sums opposite infinities: the inputs hold no NaN and
    neither does the exact fold."""
    vals = vals.copy()
    take = rng.random(vals.size) < 0.5
    pick = rng.integers(0, _MAGS.size, size=vals.size)
    sign = np.where(pick >= 4, np.asarray(elems) & 1, rng.integers(0, 2, size=vals.size))
    bits = _MAGS[pick] | (sign.astype(np.uint32) << np.uint32(31))
    vals.view(np.uint32)[take] = bits[take]
    return vals


def _mk(name, n, idxs, eq=False, special=False, nan=False, claims=None, **flags):
    rng = _rng(name)
    local = rng.standard_normal(n).astype(np.float32)
    if special:
        local = _specialise(local, np.arange(n), rng)
    if nan:
        local[rng.choice(n, size=max(1, n // 50), replace=False)] = np.nan
    pays = []
    for ix in idxs:
        ix = np.asarray(ix, dtype=np.int64).reshape(-1)
        assert ix.size == 0 or (ix[0] >= 0 and ix[-1] < n and np.all(np.diff(ix) > 0)), name
        vals = rng.standard_normal(ix.size).astype(np.float32)
        if special:
            vals = _specialise(vals, ix, rng)
        if nan and ix.size:
            vals[rng.choice(ix.size, size=max(1, ix.size // 10), replace=False)] = np.nan
        pays.append((ix.astype(np.int32), vals))
    np_ = len(pays)
    if eq:   # a regular graph's Metro-Hastings weights: the merge's EQW form
        weights = [1 / (np_ + 1)] * np_
    else:
        weights = [ofold.mh_weight(np_, int(d)) for d in rng.integers(1, 20, size=np_)]
    w_self = 1 - sum(weights)
    flags["claims"] = claims or {}
    flags["nan"] = nan
    return Case(name, n, local, pays, weights, w_self, flags)


def _union(a, extra):
    return np.unique(np.concatenate([np.asarray(a, np.int64), np.asarray(extra, np.int64)]))


def _scatter(rng, n, k, np_):
    return [np.sort(rng.choice(n, size=min(n, k), replace=False)) for _ in range(np_)]


def size_case(T, n, np_=6):
    """n = T q + r (or a small n): np_ random payloads; the first and last payload name n - 1,
    the second names 0."""
    name = f"size-n{n}-p{np_}"
    idxs = _scatter(_rng(name + "/i"), n, max(1, n // 16), np_)
    idxs[0] = _union(idxs[0], [n - 1])
    idxs[-1] = _union(idxs[-1], [n - 1])
    idxs[1] = _union(idxs[1], [0])
    return _mk(name, n, idxs, claims={"n": n, "first_last": True})


def tile_edge_case(T):
    """Four whole tiles and a 5-element tail.  Payload 0 names {t T - 1, t T} at every tile
    boundary, 1 only element 0, 2 only n - 1, 3 the whole of tile 1 and nothing else, 4 entries
    of tiles 0 and 3 only (two whole tiles skipped), 5 the tail only."""
    n = 4 * T + 5
    rng = _rng(f"tile-edges-T{T}")
    b = np.concatenate([[t * T - 1, t * T] for t in range(1, 5)])
    skip = np.concatenate([np.sort(rng.choice(T, 5, replace=False)),
                           3 * T + np.sort(rng.choice(T, 5, replace=False))])
    idxs = [b, [0], [n - 1], np.arange(T, 2 * T), skip, np.arange(4 * T + 1, n)]
    return _mk(f"tile-edges-T{T}", n, idxs, claims={"tile_edges": T})


def window_case(T, c, np_, last):
    """Payload 0 holds exactly c entries inside one tile (tile 1 of three and a tail, or the
    ragged last tile) and its next entry in the next tile; the others hold a few entries."""
    if last:
        r = c + 3
        if r >= T:
            return None
        n, dense = 2 * T + r, 2
    else:
        if c > T:
            return None
        n, dense = 3 * T + 5, 1
    name = f"window-T{T}-c{c}-p{np_}-{'last' if last else 'mid'}"
    rng = _rng(name + "/i")
    lo, hi = dense * T, min((dense + 1) * T, n)
    inner = lo + np.sort(rng.choice(hi - lo, size=c, replace=False))
    p0 = _union(inner, [3] + ([] if last else [hi + 7]))
    idxs = [p0] + _scatter(rng, n, 3, np_ - 1)
    if np_ > 1:
        idxs[1] = _union(idxs[1], inner[::7])   # shared elements: two hits across the window
    return _mk(name, n, idxs, eq=bool(c & 1), claims={"window": (0, T, dense, c)})


HITS = (1, 2, 3, 4, 5, "np")


def hits_case(T, np_, variant):
    """Four whole tiles and a tail; for every h in 1, 2, 3, 4, 5, np and for payload 0 inside /
    outside the subset one element named by exactly h payloads, at the first, a middle or the
    last element of a tile (the three variants rotate the positions over the combinations)."""
    n = 4 * T + 5
    name = f"hits-T{T}-p{np_}-v{variant}"
    rng = _rng(name + "/i")
    combos = [(h if h != "np" else np_, w0) for h in HITS for w0 in (True, False)]
    combos = [(h, w0) for h, w0 in dict.fromkeys(combos) if h <= np_ and (w0 or h < np_)]
    used = {0: 0, 1: 0, 2: 0}
    hits = {}
    for c, (h, w0) in enumerate(combos):
        kind = (c + variant) % 3
        tile = used[kind] % 4
        used[kind] += 1
        elem = (tile * T, tile * T + T // 2 + used[kind], tile * T + T - 1)[kind]
        rest = rng.permutation(np.arange(1, np_))
        sub = ([0] + rest[:h - 1].tolist()) if w0 else rest[:h].tolist()
        assert elem not in hits
        hits[elem] = tuple(sorted(sub))
    free = np.setdiff1d(np.arange(n), np.fromiter(hits, dtype=np.int64))
    extra = rng.choice(free, size=2 * np_, replace=False)   # two private entries per payload
    idxs = [_union([e for e, s in hits.items() if p in s], extra[2 * p:2 * p + 2]) for p in range(np_)]
    return _mk(name, n, idxs, eq=bool(variant == 1), claims={"hits": hits, "T": T})


def pool_case(total):
    """Classic hit-chain path: 70 elements of tile 1 named by three payloads each (more than
    FOLD_POOL rows: the rows past the pool take the per-payload walk), the tile's entry total
    exactly `total` <= FOLD_CAP; tiles 0 and 2 sparse."""
    T, np_ = FOLD_TILE, 6
    n = 3 * T + 5
    name = f"pool-total{total}"
    rng = _rng(name + "/i")
    assert 70 * 3 + 20 * 2 <= total <= FOLD_CAP
    elems = T + np.sort(rng.choice(T, size=90, replace=False))
    sets = [set() for _ in range(np_)]
    for i, e in enumerate(elems[:70]):           # triples (i, i + 1, i + 2) mod 6
        for d in range(3):
            sets[(i + d) % np_].add(int(e))
    for i, e in enumerate(elems[70:]):           # twenty two-hit elements
        for d in range(2):
            sets[(i + d) % np_].add(int(e))
    free = np.setdiff1d(np.arange(T, 2 * T), elems)
    single = rng.choice(free, size=total - 70 * 3 - 20 * 2, replace=False)
    for i, e in enumerate(single):
        sets[i % np_].add(int(e))
    out = _scatter(rng, T, 4, np_)               # tile 0
    idxs = [_union(sorted(sets[p]), np.concatenate([out[p], [2 * T + 11 * p + 1]])) for p in range(np_)]
    idxs[0] = _union(idxs[0], [n - 1])
    return _mk(name, n, idxs, claims={"tile_total": (T, 1, total), "pool_rows": (T, 1, 70)})


def switch_case(total, np_=16):
    """Sixteen payloads whose entries in tile 1 (of 4096 elements) total exactly `total`; tile 0,
    tile 2 and the tail are sparse, so one launch holds both sides of the classic kernel's
    preload bound (2048), of its hit-chain capacity (2816) and of the group kernel's rounds
    (FG_CAP = 6144 entries each)."""
    T = FOLD_TILE
    n = 3 * T + 5
    name = f"switch-total{total}"
    rng = _rng(name + "/i")
    idxs = []
    for p in range(np_):
        cnt = total // np_ + (1 if p < total % np_ else 0)
        inner = T + np.sort(rng.choice(T, size=cnt, replace=False))
        idxs.append(_union(inner, [7 * p + 1, 2 * T + 5 * p + 2] + ([n - 1] if p % 5 == 0 else [])))
    return _mk(name, n, idxs, eq=bool(total & 1), claims={"tile_total": (T, 1, total)})


def slot_case(ept, extra):
    """Merge: the hits on wave 0's elements of tile 1 (fm_elem layout) total exactly
    WE + extra — WE / 2 of its elements named by two payloads each, and `extra` more named once
    — the other waves sparse, and a normal tile 2 after it in the same block."""
    TE, WE, np_ = merge_te(ept), merge_we(ept), 6
    n = 3 * TE + 5
    name = f"slot-ept{ept}-WE+{extra}"
    rng = _rng(name + "/i")
    w0 = TE + merge_wave_elems(ept, 0)
    sets = [set() for _ in range(np_)]
    for i, e in enumerate(w0[:WE // 2]):
        sets[i % np_].add(int(e))
        sets[(i + 1 + i // np_ % (np_ - 1)) % np_].add(int(e))
    for i in range(extra):
        sets[2].add(int(w0[WE // 2 + 3 * i]))
    for w in (1, 2, 3):                          # the other waves: three entries each
        ew = TE + merge_wave_elems(ept, w)
        for i, e in enumerate(rng.choice(ew, size=3, replace=False)):
            sets[(w + i) % np_].add(int(e))
    t0, t2 = _scatter(rng, TE, 5, np_), _scatter(rng, TE, 9, np_)
    idxs = [_union(sorted(sets[p]), np.concatenate([t0[p], 2 * TE + t2[p], [n - 1 - p % 2]]))
            for p in range(np_)]
    return _mk(name, n, idxs, eq=bool(extra & 1), claims={"wave_total": (ept, 1, 0, WE + extra)})


def empty_case(T, np_, empties):
    """np_ payloads of which those at `empties` hold no entry (k = 0, null arrays)."""
    n = 2 * T + 5
    name = f"empty-T{T}-p{np_}-at{'_'.join(map(str, empties))}"
    idxs = _scatter(_rng(name + "/i"), n, max(2, n // 24), np_)
    for p in empties:
        idxs[p] = np.zeros(0, np.int64)
    return _mk(name, n, idxs, eq=np_ > 16, claims={"empty": tuple(empties)})


def align_case(T, local_off=0, idx_off=0, val_off=0):
    """Device views off 16-byte alignment: local / out, or every payload's idx / val array."""
    n = 2 * T + 6
    name = f"align-T{T}-l{local_off}-i{idx_off}-v{val_off}"
    idxs = _scatter(_rng(name + "/i"), n, max(9, n // 16), 6)
    return _mk(name, n, idxs, local_off=local_off, idx_off=idx_off, val_off=val_off,
               claims={"offsets": (local_off, idx_off, val_off)})


def kmod_case(T, k):
    """Payload 0 holds exactly k entries (k % 4 = 0 .. 3, k a multiple of 1024: the offsets
    pre-pass's sentinel thread and its int4 load); five more payloads are sparse."""
    n = max(3 * T + 5, k + k // 8 + 3)
    name = f"kmod-T{T}-k{k}"
    rng = _rng(name + "/i")
    idxs = [np.sort(rng.choice(n, size=k, replace=False))] + _scatter(rng, n, 11, 5)
    return _mk(name, n, idxs, claims={"k0": k})


def special_case(T, np_, eq, nan=False):
    """Special values in local and in the payloads (SPECIAL_BITS), every flag variant."""
    n = 2 * T + 3
    name = f"{'nan' if nan else 'special'}-T{T}-p{np_}-{'eq' if eq else 'mh'}"
    rng = _rng(name + "/i")
    idxs = _scatter(rng, n, max(3, n // 6), np_)
    idxs[0] = _union(idxs[0], [0, n - 1])
    return _mk(name, n, idxs, eq=eq, special=True, nan=nan, variants="all",
               claims={"special": True})


# ---- the case lists -----------------------------------------------------------------------------
SMALL_N = (1, 2, 3, 5, 63, 64, 65, 1023)          # walk, classic: the scalar builds
MERGE_SMALL_N = (1024, 1025, 1026, 1027)          # merge: below TE at EPT 8 and 16


def _builders(T, family, windows_only=False):
    """[(name, thunk)] for one tile size and engine family."""
    out = []

    def add(f, *a, **kw):
        out.append(functools.partial(f, *a, **kw))

    np_windows = (1, 4, 5, 13, 16) if family == "walk" else (6,)
    for c in (63, 64, 65, 127, 128, 129):
        for last in (False, True):
            for np_ in np_windows:
                add(window_case, T, c, np_, last)
    if windows_only:
        return out
    for q in (1, 2, 3):
        for r in (0, 1, 2, 3, 5, T - 1):
            add(size_case, T, T * q + r)
    add(size_case, T, 2 * T + 2, 3)
    add(size_case, T, 3 * T - 1, 3)
    if family == "walk":
        add(size_case, T, 9 * T + 2)             # a wave of the one block walks three tiles
        add(size_case, T, 9 * T + 2, 16)
    if family in ("walk", "classic"):
        for n in SMALL_N:
            add(size_case, T, n, 3)
            add(size_case, T, n, 6)
    if family == "merge":
        for n in MERGE_SMALL_N:
            add(size_case, T, n)
    add(tile_edge_case, T)
    for np_ in (6, 16):
        for v in range(3):
            add(hits_case, T, np_, v)
    for empties in ((0,), (3,), (5,)):
        add(empty_case, T, 6, empties)
    add(empty_case, T, 3, (1,))
    add(empty_case, T, 17, ())
    add(empty_case, T, 20, (18,))
    add(align_case, T, local_off=1)
    for off in (1, 2, 3):
        add(align_case, T, idx_off=off, val_off=(off + 1) % 4)
    for k in (1021, 1022, 1023, 1024, 2048):
        add(kmod_case, T, k)
    for np_, eq in ((6, True), (6, False), (3, False), (16, True)):
        add(special_case, T, np_, eq)
    add(special_case, T, 6, False, nan=True)
    add(special_case, T, 6, True, nan=True)
    if T == FOLD_TILE:
        for total in (300, FOLD_CAP):
            add(pool_case, total)
        for total in (FOLD_PRELOAD, FOLD_PRELOAD + 1, FOLD_CAP, FOLD_CAP + 1,
                      FG_CAP - 1, FG_CAP, FG_CAP + 1, 2 * FG_CAP, 2 * FG_CAP + 1):
            add(switch_case, total)
    if family == "merge":
        for extra in (0, 1):
            add(slot_case, T // FM_THREADS, extra)
    return out


WINDOW_ONLY = ("walk-epl2-w128-d1", "walk-epl4-w128-d3", "walk-epl8-w64-d1", "walk-epl16-w128-d3",
                "walk-epl16-w128-d1")


@functools.lru_cache(maxsize=None)
def _case_table(engine_name):
    """{case name: thunk} of one engine, in order."""
    e = ENGINES[engine_name]
    if e.family == "product":   # one tile size of each family
        bs = (_builders(FOLD_TILE, "classic") + _builders(merge_te(8), "merge")
              + _builders(64 * 8, "walk"))
    else:
        bs = _builders(e.T, e.family, windows_only=engine_name in WINDOW_ONLY)
    table = collections.OrderedDict()
    for b in bs:
        c = b()
        if c is not None and c.name not in table and (e.family == "product" or can_take(c, e)):
            table[c.name] = b
    return table


def case_names(engine_name):
    return list(_case_table(engine_name))


@functools.lru_cache(maxsize=64)
def get_case(engine_name, case_name):
    return _case_table(engine_name)[case_name]()


def all_pairs():
    """Every (engine name, case name) the GPU suite runs."""
    return [(e, c) for e in ENGINES for c in case_names(e)]


# ---- patch and replace engines ------------------------------------------------------------------
PATCH_K = (1, 2, 255, 256, 257)


def patch_cases():
    """Cases of the base-ready patch fold (<= 16 sparse payloads, the plain Metro-Hastings form)
    and of the one-payload replace / add: the size and tile-edge cases at the 4096-element tile,
    payloads of k in PATCH_K, and a tile whose runs exceed the patch's LDS stage (PT_CAP).
    n starts at 1023: the base comes from topk_encode(fold_base=...), which the suite does not
    run below n = 1000."""
    T = FOLD_TILE
    out = [size_case(T, n, 3) for n in (1023, T, T + 1, T + 2, 2 * T + 3, 3 * T - 1)]
    out.append(tile_edge_case(T))
    out += [switch_case(t) for t in (PT_CAP, PT_CAP + 1, FOLD_CAP + 1)]
    out += [hits_case(T, 16, 0), empty_case(T, 6, (0,)), empty_case(T, 6, (5,))]
    for k in PATCH_K:
        for np_ in (1, 3):
            name = f"patch-k{k}-p{np_}"
            n = 2 * T + 2
            rng = _rng(name + "/i")
            idxs = [_union(np.sort(rng.choice(np.arange(1, n - 1), size=k - 1, replace=False)),
                           [(0, n - 1)[p % 2]]) for p in range(np_)]
            out.append(_mk(name, n, idxs, claims={"k": k}))
    return out
