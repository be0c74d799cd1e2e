"""GPU: the sparse fold engines at their tile, window and slot edges, bit for bit against
oracle/fold.py (tests/fold_edges.py builds the cases; tests/test_cpu_fold_edges.py proves each
case is what it claims, pins the oracle to a scalar restatement of the reference, and checks
every plan on the CPU).

Every (engine, case) pair runs the case's flag variants twice on one workspace.  Before each fold
dpz_debug_fold_plan, under the same switches, must name the engine of the test id with its
epl / win / dist / ept: a forced kind that cannot take a group would run the classic kernel, so
such pairs are not parametrised at all (merge below n = 1024 or on unaligned rows; continued
totals on the walk and the merge).  Checks: output bits (NaN inputs: NaN positions, every other
element bit for bit), local's bits after an in-place fold and its untouched bits otherwise, 64
sentinel guard elements on each side of out and local, and the second run's bits equal the first's.

edge                                   case name                        engines
-------------------------------------  -------------------------------  --------------------------
n = T q + r, r in 0 1 2 3 5 T-1        size-n<N>-p6                     all (T: the engine's tile)
n below one tile / the vector builds   size-n{1..1023}-p{3,6}           classic phase group walk-*
n = 1024..1027 (merge_ok floor)        size-n102{4..7}-p6               merge-ept{4,8,16}
a wave of one block walks 3 tiles      size-n<9T+2>-p{6,16}             walk-*
{tT-1, tT}, only 0, only n-1, a full   tile-edges-T<T>                  all
  tile, two tiles skipped, tail only
63/64/65/127/128/129 entries of one    window-T<T>-c<C>-p<NP>-mid|last  walk-* (np 1 4 5 13 16; also
  payload in one tile (mid, ragged)                                       -w128 / -d1), merge-*
1 2 3 4 5 np hits, payload 0 in / out, hits-T<T>-p{6,16}-v{0,1,2}       all
  first / middle / last of a tile
> FOLD_POOL three-hit rows in a tile   pool-total{300,2816}             classic phase group
                                                                          merge-ept16 product
tile total 2048/2049/2816/2817 and     switch-total<X>                  classic phase group
  6143..6145, 12288/12289 (FG_CAP)                                        merge-ept16 product
a wave's hits WE and WE + 1, then a    slot-ept<E>-WE+{0,1}             merge-ept<E>, product (8)
  normal tile in the same block
k = 0 first / middle / last of 6, in   empty-T<T>-p<NP>-at<..>          all
  3; groups of 17 and 20
local / out one element off 16 bytes   align-T<T>-l1-i0-v0              classic phase group walk-*
idx / val 1 2 3 elements off           align-T<T>-l0-i<o>-v<o>          all
k % 4 = 0..3, k = 1024, 2048           kmod-T<T>-k<K>                   all
-0, subnormals, FLT_MIN, FLT_MAX, inf  special-T<T>-p<NP>-eq|mh         all (16 flag variants;
  equal and unequal weights                                               fresh ones on walk / merge)
NaN in local and payloads              nan-T<T>-p6-eq|mh                all
base-ready patch, replace, add, slice  test_patch_* / test_replace_*    patch1 patch replace
"""
import ctypes

import numpy as np
import pytest
import torch

from decentralizepy_amd import _lib
from oracle import fold as ofold
from tests import fold_edges as fe

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x7FA55AA5   # a NaN pattern no fold produces: an unwritten output element shows too


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _guarded(dev, data, n, off=0):
    """(buffer, view): n floats `off` elements past a 16-byte boundary, 64 sentinel elements
    (and the offset's) before and 64 after; data=None leaves the view full of sentinels."""
    buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    view = buf.view(torch.float32)[GUARD + off:GUARD + off + n]
    assert view.data_ptr() % 16 == (4 * off) % 16
    if data is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(data)))
    return buf, view


def _split(buf, n, off=0):
    """(the view's bits, the guards' bits) of a guarded buffer, on the host."""
    b = buf.cpu().numpy().view(np.uint32)
    lo = GUARD + off
    return b[lo:lo + n], np.concatenate([b[:lo], b[lo + n:]])


def _off_view(dev, arr, off):
    if arr.size == 0:
        return torch.empty(0, dtype=torch.from_numpy(arr).dtype, device=dev)
    buf = torch.zeros(arr.size + off, dtype=torch.from_numpy(arr).dtype, device=dev)
    buf[off:].copy_(torch.from_numpy(arr))
    v = buf[off:]
    assert v.data_ptr() % 16 == (4 * off) % 16
    return v


def _device_payloads(dev, case):
    io, vo = case.flags.get("idx_off", 0), case.flags.get("val_off", 0)
    return [(_off_view(dev, i, io), _off_view(dev, v, vo)) for i, v in case.payloads]


def _assert_same(got_bits, want, nan, what):
    wb = _bits(want)
    if nan:
        gn = np.isnan(got_bits.view(np.float32))
        assert np.array_equal(gn, np.isnan(want)), (what, "NaN positions")
        ok = ~np.isnan(want)
        got_bits, wb = got_bits[ok], wb[ok]
    bad = np.flatnonzero(got_bits != wb)
    assert bad.size == 0, (what, bad[:8], got_bits[bad[:8]], wb[bad[:8]])


def _fold_once(codec, dev, case, v, tpays, ws):
    off = case.flags.get("local_off", 0)
    lbuf, tl = _guarded(dev, case.local, case.n, off)
    obuf, out = _guarded(dev, fe.start_total(case) if v.accumulate else None, case.n, off)
    codec.decode_average(tl, tpays, case.weights, case.w_self if v.w_self else None, out=out,
                         zero_base=v.zero_base, accumulate=v.accumulate,
                         also_local=v.also_local, workspace=ws)
    torch.cuda.synchronize()
    return _split(obuf, case.n, off), _split(lbuf, case.n, off)


def _run_case(dev, case, engine, lib):
    from decentralizepy_amd import codec
    tpays = _device_payloads(dev, case)
    ws = codec.Workspace(dev)
    nan = case.flags["nan"]
    sent = np.uint32(SENTINEL)
    planned = set()
    for v in fe.variants_of(case, engine):
        # the engine-ran-as-named check, under the environment the fold is about to run in
        for g in range(len(fe.groups_of(case))):
            p = fe.plan_of(case, lib, fe.fold_flags(v), g)
            if engine.family == "product":
                planned.add(p["engine"])
                continue
            want = fe.expect_plan(case, engine, v, g)
            assert {f: p[f] for f in want} == want, (case.name, engine.name, v.name, g, p)
            if g == 0:
                assert p["engine"] in engine.engines, (case.name, engine.name, v.name, p)
        want = fe.expected(case, v)
        first = None
        for rep in range(2):
            (ob, og), (lb, lg) = _fold_once(codec, dev, case, v, tpays, ws)
            what = (case.name, engine.name, v.name, "run", rep)
            _assert_same(ob, want, nan, what + ("out",))
            assert (og == sent).all(), what + ("out guards",)
            assert (lg == sent).all(), what + ("local guards",)
            if v.also_local:
                _assert_same(lb, want, nan, what + ("local",))
            else:
                assert np.array_equal(lb, _bits(case.local)), what + ("local changed",)
            if first is None:
                first = (ob, lb)
            else:   # state left in the workspace by the first run would show here
                assert np.array_equal(ob, first[0]) and np.array_equal(lb, first[1]), what
    return planned


@pytest.mark.parametrize("engine_name,case_name",
                         [pytest.param(e, c, id=f"{e}-{c}") for e, c in fe.all_pairs()])
def test_fold_edge(dev, request, monkeypatch, engine_name, case_name):
    engine = fe.ENGINES[engine_name]
    if engine.family == "product":
        lib = _lib.lib()
    else:
        lib = request.getfixturevalue("diag_lib")
        for k, val in engine.env.items():
            monkeypatch.setenv(k, val)
    case = fe.get_case(engine_name, case_name)
    planned = _run_case(dev, case, engine, lib)
    if planned:
        print(case_name, "product engines:", sorted(planned))


# ---- the patch and replace engines (the product library: no switch reaches them) ------------------
PATCH_CASES = {c.name: c for c in fe.patch_cases()}


@pytest.mark.parametrize("case_name", sorted(PATCH_CASES))
def test_patch_after_foldbase(dev, case_name):
    """DPZ_FOLD_BASE_READY over the base that topk_encode(fold_base=...) wrote: only the hit
    elements are rewritten, and the result is the oracle's fold."""
    from decentralizepy_amd import codec
    case = PATCH_CASES[case_name]
    n, np_ = case.n, len(case.payloads)
    p = fe.plan_of(case, _lib.lib(), _lib.DPZ_FOLD_BASE_READY | _lib.DPZ_FOLD_SELF, fresh=0)
    assert p["engine"] == (fe.PATCH1 if np_ == 1 else fe.PATCH)
    rng = np.random.default_rng(n)
    x0 = (case.local - 0.01 * rng.standard_normal(n)).astype(np.float32)
    tpays = _device_payloads(dev, case)
    ws = codec.Workspace(dev)
    want = ofold.fold(case.local, case.payloads, case.weights, case.w_self)
    empty = [(np.zeros(0, np.int32), np.zeros(0, np.float32))] * np_
    want_base = ofold.fold(case.local, empty, case.weights, case.w_self)
    first = None
    for rep in range(2):
        lbuf, tl = _guarded(dev, case.local, n)
        bbuf, base = _guarded(dev, None, n)
        codec.topk_encode(tl, max(1, n // 100), x0=torch.from_numpy(x0).to(dev),
                          fold_base=(base, case.weights, case.w_self))
        torch.cuda.synchronize()
        bb, bg = _split(bbuf, n)
        _assert_same(bb, want_base, False, (case_name, "base"))
        codec.decode_average(tl, tpays, case.weights, case.w_self, out=base, base_ready=True,
                             workspace=ws)
        torch.cuda.synchronize()
        ob, og = _split(bbuf, n)
        lb, lg = _split(lbuf, n)
        _assert_same(ob, want, False, (case_name, "patched", rep))
        assert (og == np.uint32(SENTINEL)).all() and (lg == np.uint32(SENTINEL)).all()
        assert np.array_equal(lb, _bits(case.local))
        first = ob if first is None else first
        assert np.array_equal(ob, first)


@pytest.mark.parametrize("case_name", sorted(PATCH_CASES))
def test_replace_add_and_slice(dev, case_name):
    """One sparse payload replaced (T = local; T[idx] = vals), added (local + T, T zero off its
    entries) and replaced over a slice at a non-zero offset (dpz_replace_slice): the
    range-partitioned chunk kernel of csrc/dpz_replace.h."""
    from decentralizepy_amd import codec
    case = PATCH_CASES[case_name]
    n = case.n
    sent = np.uint32(SENTINEL)
    ws = codec.Workspace(dev)
    for pi, (idx, vals) in enumerate(case.payloads[:3]):
        if idx.size == 0:
            continue
        one = fe.Case(case.name, n, case.local, [(idx, vals)], [1.0], None, case.flags)
        ti, tv = _off_view(dev, idx, 0), _off_view(dev, vals, 0)
        zeros = np.zeros(n, np.float32)
        for mode, flag, want in (
                ("replace", _lib.DPZ_FOLD_REPLACE_ONLY, ofold.replace(case.local, idx, vals)),
                ("add", _lib.DPZ_FOLD_ADD_ONLY, case.local + ofold.replace(zeros, idx, vals))):
            assert fe.plan_of(one, _lib.lib(), flag)["engine"] == fe.REPLACE
            for rep in range(2):
                lbuf, tl = _guarded(dev, case.local, n)
                obuf, out = _guarded(dev, None, n)
                codec.decode_average(tl, [(ti, tv)], out=out, replace_only=mode == "replace",
                                     add_only=mode == "add", workspace=ws)
                torch.cuda.synchronize()
                ob, og = _split(obuf, n)
                lb, lg = _split(lbuf, n)
                _assert_same(ob, want, False, (case_name, pi, mode, rep))
                assert (og == sent).all() and (lg == sent).all()
                assert np.array_equal(lb, _bits(case.local))
        # a rank's slice [off, off + m) of the model: indices stay global
        off = n // 3 + 1
        m = n - off - 1
        lbuf, tl = _guarded(dev, case.local[off:off + m], m)
        obuf, out = _guarded(dev, None, m)
        rc = _lib.lib().dpz_replace_slice(
            ctypes.c_void_p(tl.data_ptr()), m, off, ctypes.c_void_p(ti.data_ptr()),
            ctypes.c_void_p(tv.data_ptr()), idx.size, ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        ob, og = _split(obuf, m)
        _assert_same(ob, ofold.replace(case.local, idx, vals)[off:off + m], False,
                     (case_name, pi, "slice"))
        assert (og == sent).all()
