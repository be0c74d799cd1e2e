"""The ``selection`` keyword of the batched engines on their CPU stand-ins, and the windowed entry
points' host checks, which come before any launch."""
import numpy as np
import pytest
import torch

from tests.test_cpu_topkacc_round import NP


def _topk(selection):
    from decentralizepy_amd.gossip_topkacc import TopKAccRound
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((3, 200)).astype(np.float32))
    return TopKAccRound([{1}, {0, 2}, {1}], x, 0.1, selection=selection, **NP)


def _jwins(selection):
    from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound
    from tests.jwins_ops import OracleJwinsOps
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((3, 300)).astype(np.float32))
    return JwinsBatchRound([{1}, {0, 2}, {1}], x, [0.1, 0.2, 1.0], ops=OracleJwinsOps(),
                           selection=selection)


def test_the_stand_ins_accept_the_keyword_and_select_exactly():
    a, b = _topk("window"), _topk("exact")
    j, k = _jwins("window"), _jwins("exact")
    for r in range(2):
        for e, f in ((a, b), (j, k)):
            e.x += 0.01
            f.x += 0.01
            e.step()
            f.step()
            assert torch.equal(e.x, f.x) and torch.equal(e.acc, f.acc)
            assert e.selection_status().tolist() == [0, 0, 0]


@pytest.mark.parametrize("make", [_topk, _jwins])
def test_another_selection_is_refused(make):
    with pytest.raises(ValueError, match="'exact' or 'window'"):
        make("sampled")


def test_entry_points_check_their_arguments_before_any_launch():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    ARG, UNSUP, WS = _lib.DPZ_ERR_ARG, _lib.DPZ_ERR_UNSUPPORTED, _lib.DPZ_ERR_WORKSPACE
    d, n, k = 4096, 20000, 2000  # d is never dereferenced: the checks come first
    need = L.dpz_topkacc_encode_window_workspace_bytes(3, n, k)
    assert need > L.dpz_topkacc_encode_workspace_bytes(3, n)
    assert need == L.dpz_jwins_encode_window_workspace_bytes(3, n, k)
    assert L.dpz_topkacc_encode_window_workspace_bytes(0, n, k) == 0
    assert L.dpz_jwins_encode_window_workspace_bytes(3, n, n + 1) == 0
    assert 1 <= L.dpz_jwins_window_slots() <= 16

    def acc(m=3, tab=d, n=n, k=k, mode=1, ws=d, wsb=need):
        return L.dpz_topkacc_encode_nodes_window(m, tab, n, k, mode, ws, wsb, None)

    def jw(m=3, tab=d, n=n, k=k, ws=d, wsb=need):
        return L.dpz_jwins_encode_nodes_window(m, tab, n, k, ws, wsb, None)

    for f in (acc, jw):
        for bad in (dict(m=0), dict(tab=None), dict(ws=None), dict(n=0), dict(n=1 << 31),
                    dict(k=0), dict(k=n + 1), dict(tab=d + 4), dict(ws=d + 16)):
            assert f(**bad) == ARG, bad
        assert f(wsb=need - 1) == WS and f(wsb=0) == WS
        assert f(m=65536, wsb=1 << 50) == UNSUP
    assert acc(mode=7) == ARG
