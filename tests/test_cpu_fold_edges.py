"""CPU: the sparse fold's edge cases (tests/fold_edges.py) are what they claim, the oracle they
are held to agrees with a scalar restatement of the reference, and every (engine, case) pair of
tests/test_gpu_fold_edges.py plans the engine it names.

* Every builder's claims — per-tile and per-wave entry totals, window counts, hit multiplicities,
  empty payloads, alignment offsets — are recomputed here from the returned arrays with plain
  numpy: a GPU case cannot quietly test nothing.
* oracle/fold.py is compared bit for bit, on every case, with a per-element loop in np.float32
  written from the reference (sharing/Sharing.py:156-190: total = T_0 w_0, total += T_i w_i,
  total += (1 - sum w) local; sharing/PartialModel.py:292-295: T = local, T[idx] = params); the
  special-value cases also under every flag variant.
* dpz_debug_fold_plan, as in tests/test_cpu_fold_plan.py: the product library with no switch set,
  and the diagnostic library under each engine's switches where it is built.

Run with -s to see each case's counted properties and expected plan."""
import os

import numpy as np
import pytest

from decentralizepy_amd import _lib
from oracle import fold as ofold
from tests import fold_edges as fe

FIELDS = fe.PLAN_FIELDS

_UNIQUE = {}
for _e, _c in fe.all_pairs():
    _UNIQUE.setdefault(_c, _e)
UNIQUE = sorted(_UNIQUE.items())
PATCH_CASES = {c.name: c for c in fe.patch_cases()}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


plan_of = fe.plan_of


# ---- the claims ---------------------------------------------------------------------------------
def _tile_counts(idx, T, n):
    return np.bincount(np.asarray(idx, np.int64) // T, minlength=-(-n // T))


def _hit_count(case):
    h = np.zeros(case.n, np.int64)
    for idx, _ in case.payloads:
        h[idx] += 1
    return h


def _check_claims(case):
    """Recount every claim; returns the counted properties (printed)."""
    seen = {"n": case.n, "np": len(case.payloads), "k": [int(i.size) for i, _ in case.payloads]}
    assert case.local.dtype == np.float32 and case.local.shape == (case.n,)
    assert len(case.weights) == len(case.payloads)
    for idx, vals in case.payloads:
        assert idx.dtype == np.int32 and vals.dtype == np.float32 and idx.shape == vals.shape
        if idx.size:
            assert idx[0] >= 0 and idx[-1] < case.n and np.all(np.diff(idx.astype(np.int64)) > 0)
    cl = case.flags["claims"]
    hc = _hit_count(case)
    if "first_last" in cl:
        assert hc[0] >= 1 and hc[case.n - 1] >= 2
        seen["hits_at_0_and_last"] = (int(hc[0]), int(hc[-1]))
    if "tile_edges" in cl:
        T = cl["tile_edges"]
        p = [i for i, _ in case.payloads]
        assert p[0].tolist() == [v for t in range(1, 5) for v in (t * T - 1, t * T)]
        assert p[1].tolist() == [0] and p[2].tolist() == [case.n - 1]
        assert p[3].tolist() == list(range(T, 2 * T))
        c4 = _tile_counts(p[4], T, case.n)
        assert c4[0] > 0 and c4[1] == 0 and c4[2] == 0 and c4[3] > 0 and c4[4] == 0
        c5 = _tile_counts(p[5], T, case.n)
        assert c5[:4].sum() == 0 and c5[4] > 0
        seen["tile_counts"] = [_tile_counts(i, T, case.n).tolist() for i in p]
    if "window" in cl:
        p, T, tile, c = cl["window"]
        cnt = _tile_counts(case.payloads[p][0], T, case.n)
        assert cnt[tile] == c
        last = tile == len(cnt) - 1
        assert last == (case.n % T != 0 and tile == case.n // T)
        if not last:
            assert cnt[tile + 1] >= 1          # the next entry lies in the next tile
        else:
            assert case.n - tile * T < T       # the dense tile is the ragged one
        assert cnt[0] >= 1                     # and the cursor enters the tile from an earlier one
        seen["window"] = {"payload": p, "tile": tile, "entries": int(cnt[tile]), "last": bool(last)}
    if "hits" in cl:
        T = cl["T"]
        kinds = set()
        for elem, sub in cl["hits"].items():
            named = tuple(p for p, (idx, _) in enumerate(case.payloads) if elem in idx)
            assert named == sub and hc[elem] == len(sub)
            kinds.add((len(sub), 0 in sub, {0: "first", T - 1: "last"}.get(elem % T, "middle")))
        np_ = len(case.payloads)
        for h in (1, 2, 3, 4, 5, np_):
            assert {w0 for hh, w0, _ in kinds if hh == h} == ({True, False} if h < np_ else {True})
        assert {k for _, _, k in kinds} == {"first", "middle", "last"}
        assert hc.max() == np_ and set(np.unique(hc)) >= {0, 1, 2, 3, 4, 5}
        seen["hits"] = sorted(kinds)
    if "tile_total" in cl:
        T, tile, total = cl["tile_total"]
        tot = sum(_tile_counts(i, T, case.n) for i, _ in case.payloads)
        assert tot[tile] == total
        others = np.delete(tot, tile)
        assert others.max() < 64 * len(case.payloads) and others.min() >= 1   # the neighbours: sparse
        seen["tile_totals"] = tot.tolist()
    if "pool_rows" in cl:
        T, tile, rows = cl["pool_rows"]
        three = np.count_nonzero(hc[tile * T:(tile + 1) * T] >= 3)
        assert three == rows and rows > fe.FOLD_POOL
        assert np.count_nonzero(hc[tile * T:(tile + 1) * T] == 2) >= 1
        seen["elements_with_3_hits"] = int(three)
    if "wave_total" in cl:
        ept, tile, wave, total = cl["wave_total"]
        TE = fe.merge_te(ept)
        rel = np.arange(TE)
        per_wave = [int(hc[tile * TE:(tile + 1) * TE][fe.merge_wave_of(ept, rel) == w].sum())
                    for w in range(4)]
        assert per_wave[wave] == total
        assert all(t <= 8 for w, t in enumerate(per_wave) if w != wave)
        nxt = [int(hc[(tile + 1) * TE:(tile + 2) * TE][fe.merge_wave_of(ept, rel) == w].sum())
               for w in range(4)]
        assert 0 < sum(nxt) and max(nxt) <= fe.merge_we(ept)   # a normal tile follows
        assert sorted(np.concatenate([fe.merge_wave_elems(ept, w) for w in range(4)])) == list(rel)
        seen["wave_totals"] = {"tile": per_wave, "next_tile": nxt, "WE": fe.merge_we(ept)}
    if "empty" in cl:
        empt = tuple(p for p, (i, _) in enumerate(case.payloads) if i.size == 0)
        assert empt == cl["empty"]
        assert sum(i.size for i, _ in case.payloads) > 0
        seen["empty"] = empt
    if "offsets" in cl:
        assert cl["offsets"] == (case.flags.get("local_off", 0), case.flags.get("idx_off", 0),
                                 case.flags.get("val_off", 0))
        assert any(o % 4 for o in cl["offsets"])
        seen["view_offsets"] = cl["offsets"]
    if "k0" in cl:
        assert case.payloads[0][0].size == cl["k0"]
        seen["k0_mod_4"] = cl["k0"] % 4
    if "k" in cl:
        assert all(i.size == cl["k"] for i, _ in case.payloads)
    if "special" in cl:
        allv = np.concatenate([case.local] + [v for _, v in case.payloads])
        have = set(_bits(allv).tolist())
        assert have >= set(fe.SPECIAL_BITS.tolist())
        assert np.isnan(allv).any() == case.flags["nan"]
        if case.flags["nan"]:
            assert np.isnan(case.local).any() and any(np.isnan(v).any() for _, v in case.payloads)
        seen["special_values"] = int(np.isin(_bits(allv), fe.SPECIAL_BITS).sum())
        seen["nan_inputs"] = int(np.isnan(allv).sum())
    return seen


@pytest.mark.parametrize("case_name,engine", UNIQUE)
def test_case_delivers_what_it_claims(case_name, engine):
    case = fe.get_case(engine, case_name)
    assert case.name == case_name
    print(case_name, _check_claims(case))


@pytest.mark.parametrize("case_name", sorted(PATCH_CASES))
def test_patch_case_delivers_what_it_claims(case_name):
    print(case_name, _check_claims(PATCH_CASES[case_name]))


def test_case_lists_cover_every_edge():
    """Sizes, windows, hit counts, totals and offsets the issue lists, per engine family."""
    for name, e in fe.ENGINES.items():
        names = fe.case_names(name)
        assert names, name
        if e.family == "product" or name in fe.WINDOW_ONLY:
            continue
        T = e.T
        ns = {fe.get_case(name, c).n for c in names if c.startswith("size-")}
        assert ns >= {T * q + r for q in (1, 2, 3) for r in (0, 1, 2, 3, 5, T - 1)}
        assert {n % 4 for n in ns} == {0, 1, 2, 3}
        if e.family == "merge":
            assert ns >= set(fe.MERGE_SMALL_N)
            assert any(c.startswith("slot-") for c in names)
            assert not any("align" in c and "-l1-" in c for c in names)
        else:
            assert ns >= set(fe.SMALL_N)
    for name in fe.ENGINES:
        if fe.ENGINES[name].family in ("walk", "merge"):
            T = fe.ENGINES[name].T
            cs = {c for c in (63, 64, 65, 127, 128, 129) for last in ("mid", "last")
                  if any(n.startswith(f"window-T{T}-c{c}-") and n.endswith(last)
                         for n in fe.case_names(name))}
            assert cs >= {c for c in (63, 64, 65, 127, 128, 129) if c + 3 < T}, name
    classic = fe.case_names("classic")
    for t in (2048, 2049, 2816, 2817, 6143, 6144, 6145, 12288, 12289):
        assert f"switch-total{t}" in classic and f"switch-total{t}" in fe.case_names("group")
    assert "pool-total2816" in classic


# ---- the oracle against a scalar restatement ------------------------------------------------------
def scalar_fold(local, payloads, weights, w_self, zero_base=False, start=None):
    """One element at a time, in the reference's order, every product and sum one np.float32
    operation.  Sharing.py:175-183: data = deserialized_model(msg) (PartialModel.py:292-295:
    T = local state, T[indices] = params), total = data * weight for the first message,
    total += data * weight for the others; Sharing.py:185-186: total += (1 - weight_total) *
    local.  zero_base: T = zeros and the total starts from +0.0; start: the total continues."""
    n = len(local)
    zero = np.float32(0)
    maps = [dict(zip(idx.tolist(), list(vals))) for idx, vals in payloads]
    ws = [np.float32(w) for w in weights]
    wself = None if w_self is None else np.float32(w_self)
    out = np.empty(n, np.float32)
    loc = list(local)
    st = None if start is None else list(start)
    with np.errstate(all="ignore"):
        for i in range(n):
            x = loc[i]
            b = zero if zero_base else x
            tot = None if st is None else st[i]
            for m, w in zip(maps, ws):
                term = m.get(i, b) * w
                if tot is None:
                    tot = (zero + term) if zero_base else term
                else:
                    tot = tot + term
            if tot is None:
                tot = zero
            if wself is not None:
                tot = tot + wself * x
            out[i] = tot
    return out


def _same(got, want, nan):
    if nan:
        assert np.array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        return np.array_equal(_bits(got)[ok], _bits(want)[ok])
    assert not np.isnan(want).any()
    return np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("case_name,engine", UNIQUE)
def test_oracle_matches_scalar_restatement(case_name, engine):
    case = fe.get_case(engine, case_name)
    nan = case.flags["nan"]
    with np.errstate(all="ignore"):
        got = ofold.fold(case.local, case.payloads, case.weights, case.w_self)
    assert _same(got, scalar_fold(case.local, case.payloads, case.weights, case.w_self), nan)
    if case.flags.get("variants") != "all":
        return
    for v in fe.ALL_VARIANTS:   # the special values: every variant the GPU cases are held to
        want = scalar_fold(case.local, case.payloads, case.weights,
                           case.w_self if v.w_self else None, v.zero_base,
                           fe.start_total(case) if v.accumulate else None)
        assert _same(fe.expected(case, v), want, nan), v.name
    if not nan:   # overflow to infinity and -0 are really in the expected outputs
        e = _bits(fe.expected(case, fe.ALL_VARIANTS[0]))
        assert (e == 0x7F800000).any() and (e == 0xFF800000).any()
        z = _bits(fe.expected(case, [v for v in fe.ALL_VARIANTS if v.name == "server"][0]))
        assert (z == 0x80000000).any()


@pytest.mark.parametrize("case_name", sorted(PATCH_CASES))
def test_oracle_matches_scalar_restatement_patch(case_name):
    case = PATCH_CASES[case_name]
    got = ofold.fold(case.local, case.payloads, case.weights, case.w_self)
    assert _same(got, scalar_fold(case.local, case.payloads, case.weights, case.w_self), False)


# ---- the plans ----------------------------------------------------------------------------------
def _diag():
    if not os.path.exists(_lib.DIAG_PATH):
        pytest.skip("libdpzcodec_diag.so not built (make -C decentralizepy_amd/csrc diag-lib)")
    return _lib.diag_lib()


def check_plans(case, engine, lib):
    """Every group of every variant plans what fold_edges.expect_plan says; returns the first
    group's plan of the first variant."""
    first = None
    for v in fe.variants_of(case, engine):
        for g in range(len(fe.groups_of(case))):
            p = plan_of(case, lib, fe.fold_flags(v), g)
            want = fe.expect_plan(case, engine, v, g)
            assert not v.accumulate or engine.family == "classic"   # a continued total: tile kernels
            assert {f: p[f] for f in want} == want, (case.name, engine.name, v.name, g, p)
            if g == 0:
                assert p["engine"] in engine.engines
            first = first or p
    return first


@pytest.mark.parametrize("engine_name", [e for e in fe.ENGINES if e != "product"])
def test_forced_engine_plans_every_case(engine_name, monkeypatch):
    D = _diag()
    engine = fe.ENGINES[engine_name]
    for k, val in engine.env.items():
        monkeypatch.setenv(k, val)
    for c in fe.case_names(engine_name):
        p = check_plans(fe.get_case(engine_name, c), engine, D)
        print(engine_name, c, {f: p[f] for f in FIELDS})


def test_product_plans_every_case():
    """The product library reads no switch: the engines its own thresholds pick at these sizes
    (printed; the GPU test names the engine in its report), and at least the walk, the classic
    and the group kernel among them."""
    L = _lib.lib()
    seen = set()
    for c in fe.case_names("product"):
        case = fe.get_case("product", c)
        p = plan_of(case, L, 0x1)
        seen.add(p["engine"])
        print("product", c, {f: p[f] for f in FIELDS})
    assert seen >= {fe.CLASSIC, fe.WALK, fe.WALK_GROUPS, fe.MERGE}


def test_unaligned_rows_never_plan_the_merge(monkeypatch):
    D = _diag()
    for name in ("merge-ept4", "merge-ept8", "merge-ept16"):
        e = fe.ENGINES[name]
        for k, val in e.env.items():
            monkeypatch.setenv(k, val)
        case = fe.align_case(e.T, local_off=1)
        assert case.n >= fe.MERGE_MIN_N and not fe.can_take(case, e)
        assert plan_of(case, D, 0x1)["engine"] == fe.CLASSIC
        aligned = fe.align_case(e.T, idx_off=1, val_off=2)
        assert plan_of(aligned, D, 0x1)["engine"] == fe.MERGE


def test_patch_and_replace_plans():
    L = _lib.lib()
    base = _lib.DPZ_FOLD_BASE_READY | _lib.DPZ_FOLD_SELF
    for case in PATCH_CASES.values():
        np_ = len(case.payloads)
        p = plan_of(case, L, base, fresh=0)
        assert p["engine"] == (fe.PATCH1 if np_ == 1 else fe.PATCH) and p["offsets"] == int(np_ > 1)
        one = fe.Case(case.name, case.n, case.local, case.payloads[:1], case.weights[:1],
                      case.w_self, case.flags)
        if one.payloads[0][0].size:
            for fl in (_lib.DPZ_FOLD_REPLACE_ONLY, _lib.DPZ_FOLD_ADD_ONLY):
                assert plan_of(one, L, fl)["engine"] == fe.REPLACE
        print(case.name, {f: p[f] for f in FIELDS})
