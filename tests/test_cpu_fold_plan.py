"""CPU: the sparse fold's kernel selection (csrc/dpz_fold.hip fold_plan, exported as
dpz_debug_fold_plan).  Every engine and every threshold of the selection is pinned on the product
library with one shape on each side, k at least one entry away from the boundary; the diagnostic
build's DPZ_* switches override the plan.  No GPU: the plan makes no device call."""
import ctypes
import os

import pytest

from decentralizepy_amd import _lib

NONE, CLASSIC, GROUP, WALK, WALK_GROUPS, MERGE, REPLACE, PATCH1, PATCH = 0, 1, 2, 4, 5, 8, 9, 10, 11
FIELDS = ("engine", "vec", "epl", "dist", "win", "ept", "eqw", "offsets", "chains")
N = 1_000_000          # 245 tiles of 4096 elements
NTILES = -(-N // 4096)
GROUP_LO, GROUP_HI = 1536 * NTILES, 2 * 6144 * NTILES  # the 4-slot group kernel's etot window


def plan(ks, n=N, dense=None, w=None, flags=0, fresh=1, aligned=1, lib=None):
    L = lib or _lib.lib()
    np_ = len(ks)
    out = (ctypes.c_int * len(FIELDS))()
    rc = L.dpz_debug_fold_plan(
        n, np_, (ctypes.c_int64 * max(np_, 1))(*ks),
        (ctypes.c_int * max(np_, 1))(*(dense or [0] * np_)),
        (ctypes.c_float * max(np_, 1))(*(w or [1.0 / (np_ + 1)] * np_)), flags, fresh, aligned, out)
    assert rc == 0
    return dict(zip(FIELDS, out))


def engine(ks, **kw):
    return plan(ks, **kw)["engine"]


def test_plan_validates_arguments():
    L = _lib.lib()
    out = (ctypes.c_int * len(FIELDS))()
    k = (ctypes.c_int64 * 17)(*([1] * 17))
    assert L.dpz_debug_fold_plan(N, 17, k, None, None, 0, 1, 1, out) == _lib.DPZ_ERR_ARG
    assert L.dpz_debug_fold_plan(0, 1, k, None, None, 0, 1, 1, out) == _lib.DPZ_ERR_ARG
    assert L.dpz_debug_fold_plan(N, 1, None, None, None, 0, 1, 1, out) == _lib.DPZ_ERR_ARG
    assert L.dpz_debug_fold_plan(N, 1, k, None, None, 0, 1, 1, None) == _lib.DPZ_ERR_ARG


def test_before_grouping():
    base = _lib.DPZ_FOLD_BASE_READY | _lib.DPZ_FOLD_SELF
    # a ready base: one payload patches alone, more go through the offsets pre-pass, none: nothing
    p = plan([1000], flags=base)
    assert (p["engine"], p["offsets"]) == (PATCH1, 0)
    p = plan([1000, 0, 10], flags=base)
    assert (p["engine"], p["offsets"]) == (PATCH, 1)
    assert engine([0, 0], flags=base) == NONE and engine([0], flags=base) == NONE
    # no payloads: the classic kernel alone
    for al in (0, 1):
        p = plan([], flags=_lib.DPZ_FOLD_SELF, aligned=al)
        assert (p["engine"], p["vec"], p["offsets"], p["chains"]) == (CLASSIC, al, 0, 0)
    # one non-empty sparse payload replaced / added over aligned rows: the chunk kernel
    for fl in (_lib.DPZ_FOLD_REPLACE_ONLY, _lib.DPZ_FOLD_ADD_ONLY):
        assert engine([100], flags=fl) == REPLACE
        assert engine([N], flags=fl, dense=[1]) == CLASSIC
    p = plan([100], flags=_lib.DPZ_FOLD_REPLACE_ONLY, aligned=0)
    assert (p["engine"], p["vec"], p["offsets"]) == (CLASSIC, 0, 1)
    assert engine([0], flags=_lib.DPZ_FOLD_REPLACE_ONLY) == CLASSIC
    # add-only that the chunk kernel cannot take folds with weight 1: a one-payload walk
    p = plan([100], flags=_lib.DPZ_FOLD_ADD_ONLY, aligned=0)
    assert (p["engine"], p["vec"]) == (WALK, 0)
    assert engine([0], flags=_lib.DPZ_FOLD_ADD_ONLY) == WALK


def test_merge_thresholds():
    k = N // 100
    p = plan([k] * 6)
    assert (p["engine"], p["ept"], p["eqw"], p["offsets"]) == (MERGE, 8, 1, 0)
    assert engine([k] * 5) == CLASSIC                     # np 5: avg 0.01 is below the walk's range
    assert plan([k] * 6, w=[0.1] * 5 + [0.2])["eqw"] == 0   # unequal weights
    assert plan([k] * 16, w=[0.05] * 16)["eqw"] == 1
    # etot around 0.33 n (np 6: 330,000 entries)
    assert engine([54_999] * 6) == MERGE
    assert engine([55_001] * 6) == WALK_GROUPS            # avg 0.055: the walk takes it
    # what merge requires: a fresh all-sparse total, aligned rows, 1024 <= n < 2^31 - 8192
    assert engine([k] * 6, aligned=0) == CLASSIC
    assert engine([k] * 6, fresh=0) == CLASSIC
    assert engine([k] * 5 + [N], dense=[0] * 5 + [1]) == CLASSIC
    assert engine([10] * 6, n=1023) == CLASSIC and engine([10] * 6, n=1024) == MERGE
    assert engine([10] * 6, n=2**31 - 8193) == MERGE and engine([10] * 6, n=2**31 - 8191) == CLASSIC


def test_walk_selection():
    # <= 4 payloads at any density; 5..16 only at 0.0175 <= avg <= 0.21
    p = plan([N // 10] * 4)
    assert (p["engine"], p["vec"], p["offsets"]) == (WALK, 1, 0)
    assert (p["epl"], p["win"], p["dist"]) == (8, 64, 1)
    assert engine([N // 10] * 5) == WALK_GROUPS
    assert engine([N // 1000] * 4) == WALK and engine([N // 1000] * 5) == CLASSIC
    assert engine([N // 2] * 4) == WALK
    assert engine([17_499] * 5) == CLASSIC and engine([17_501] * 5) == WALK_GROUPS
    assert engine([209_999] * 5) == WALK_GROUPS and engine([210_001] * 5) == CLASSIC
    assert engine([209_999] * 16) == WALK_GROUPS and engine([210_001] * 16) == CLASSIC
    # VEC: aligned and n >= 1024
    assert plan([10] * 3, n=1023)["vec"] == 0 and plan([10] * 3, n=1024)["vec"] == 1
    assert plan([N // 10] * 3, aligned=0)["vec"] == 0
    assert plan([N // 10] * 13, aligned=0)["engine"] == WALK_GROUPS
    # a fresh all-sparse total below 2^31 - 1024 elements
    assert engine([10] * 3, n=2**31 - 1025) == WALK and engine([10] * 3, n=2**31 - 1023) == CLASSIC
    p = plan([N // 10] * 3, fresh=0)
    assert (p["engine"], p["offsets"], p["chains"]) == (CLASSIC, 1, 1)
    p = plan([N // 10, N, N // 10], dense=[0, 1, 0])
    assert (p["engine"], p["offsets"], p["chains"]) == (CLASSIC, 1, 0)
    assert plan([N, N], dense=[1, 1])["offsets"] == 0


@pytest.mark.parametrize("np_, rest", [(4, 20_000), (5, 20_000), (12, 30_000)])
def test_walk_tile_size_up_to_12_payloads(np_, rest):
    """EPL from the densest payload; 64-entry windows one group ahead (rest: the other payloads'
    k, keeping avg inside the walk's range and etot above the merge fold's)."""
    want = WALK if np_ <= 4 else WALK_GROUPS
    for kd, epl in ((54_999, 16), (55_001, 8), (104_999, 8), (105_001, 4), (209_999, 4),
                    (210_001, 2)):
        p = plan([kd] + [rest] * (np_ - 1))
        assert (p["engine"], p["epl"], p["win"], p["dist"]) == (want, epl, 64, 1), (kd, p)


@pytest.mark.parametrize("np_", [13, 16])
def test_walk_tile_size_13_to_16_payloads(np_):
    """Windows three groups ahead; 128-entry windows at 0.055 < dens <= 0.21."""
    for kd, epl, win in ((54_999, 16, 64), (55_001, 16, 128), (104_999, 16, 128), (105_001, 8, 128),
                         (209_999, 8, 128), (210_001, 2, 64)):
        p = plan([kd] + [30_000] * (np_ - 1))
        assert (p["engine"], p["epl"], p["win"], p["dist"]) == (WALK_GROUPS, epl, win, 3), (kd, p)
    # np 12 / 13 at one density
    p12, p13 = plan([N // 10] * 12), plan([N // 10] * 13)
    assert (p12["dist"], p12["win"], p12["epl"]) == (1, 64, 8)
    assert (p13["dist"], p13["win"], p13["epl"]) == (3, 128, 16)


def test_group_kernel_window():
    """All sparse, not replace-only, >= 8 payloads, GROUP_LO < etot <= GROUP_HI (a continued
    total, so neither merge nor walk takes the group)."""
    assert GROUP_LO % 8 == 0 and GROUP_HI % 8 == 0
    p = plan([60_000] * 8, fresh=0)
    assert (p["engine"], p["vec"], p["offsets"]) == (GROUP, 1, 1)
    assert engine([60_000] * 7, fresh=0) == CLASSIC
    assert engine([GROUP_LO // 8 + 1] * 8, fresh=0) == GROUP
    assert engine([GROUP_LO // 8 - 1] * 8, fresh=0) == CLASSIC
    assert engine([GROUP_HI // 8 - 1] * 8, fresh=0) == GROUP
    assert engine([GROUP_HI // 8 + 1] * 8, fresh=0) == CLASSIC
    assert engine([60_000] * 7 + [N], dense=[0] * 7 + [1], fresh=0) == CLASSIC
    assert plan([60_000] * 8, fresh=0, aligned=0)["vec"] == 0
    # a fresh total too dense for the walk (avg 0.25) and too large for the merge
    assert engine([250_000] * 8) == GROUP


def test_diagnostic_switches_override_the_plan(monkeypatch):
    if not os.path.exists(_lib.DIAG_PATH):
        pytest.skip("libdpzcodec_diag.so not built (make -C decentralizepy_amd/csrc diag-lib)")
    D = _lib.diag_lib()
    k = N // 100
    assert engine([k] * 16, lib=D) == MERGE
    monkeypatch.setenv("DPZ_FOLD_KIND", "1")
    assert engine([k] * 16, lib=D) == CLASSIC and engine([k] * 3, lib=D) == CLASSIC
    assert engine([k] * 16) == MERGE                      # the product library reads no environment
    monkeypatch.setenv("DPZ_FOLD_KIND", "2")
    assert engine([k] * 16, lib=D) == GROUP
    assert engine([k] * 15 + [N], dense=[0] * 15 + [1], lib=D) == CLASSIC
    monkeypatch.setenv("DPZ_FOLD_KIND", "4")
    assert engine([k] * 16, lib=D) == WALK_GROUPS and engine([k] * 16, fresh=0, lib=D) == CLASSIC
    monkeypatch.setenv("DPZ_FOLD_KIND", "8")
    assert engine([N // 10] * 3, lib=D) == MERGE
    assert engine([N // 10] * 3, aligned=0, lib=D) == CLASSIC
    monkeypatch.setenv("DPZ_MERGE_EPT", "16")
    assert plan([k] * 16, lib=D)["ept"] == 16
    monkeypatch.setenv("DPZ_MERGE_EPT", "5")
    assert plan([k] * 16, lib=D)["ept"] == 8
    monkeypatch.setenv("DPZ_FOLD_KIND", "4")
    p = plan([N // 10] * 13, lib=D)
    assert (p["epl"], p["win"], p["dist"]) == (16, 128, 3)
    monkeypatch.setenv("DPZ_FOLD_WALK_EPL", "4")
    monkeypatch.setenv("DPZ_FOLD_WIN", "64")
    monkeypatch.setenv("DPZ_FOLD_DIST", "1")
    p = plan([N // 10] * 13, lib=D)
    assert (p["epl"], p["win"], p["dist"]) == (4, 64, 1)
    monkeypatch.setenv("DPZ_FOLD_WALK_EPL", "3")         # not a tile size: the measured default
    monkeypatch.setenv("DPZ_FOLD_WIN", "128")
    p = plan([N // 10] * 5, lib=D)
    assert (p["epl"], p["win"], p["dist"]) == (8, 128, 1)
    assert plan([N // 10] * 4, lib=D)["win"] == 64        # <= 4 payloads: always 64-entry windows
