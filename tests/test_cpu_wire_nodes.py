"""CPU: what the batched wire coder (csrc/dpz_wire_nodes.hip) decides on the host: the slot bound
``dpz_elias_bound_bytes`` against the oracle's streams, the argument checks of
``dpz_wire_encode_nodes`` (made on the host table before anything is enqueued, so no device is
needed) and the engines' refusals.  The device path is covered by tests/test_gpu_wire_nodes.py."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import elias as oelias

KS = [2, 3, 1025, 1026, 2049, 5000]  # around the Elias block of 1024 codes


def index_list(kind, k, seed=0):
    """k ascending int32 indices: gaps all 1 ("ones"), equal gaps of 2^j ("pow<j>"), or
    log-uniform gaps in 2^0 .. 2^16 ("log": codes straddle words and blocks)."""
    if kind == "ones":
        gaps = np.ones(k - 1, dtype=np.int64)
    elif kind.startswith("pow"):
        gaps = np.full(k - 1, 1 << int(kind[3:]), dtype=np.int64)
    else:
        rng = np.random.default_rng(seed + k)
        gaps = np.floor(2.0 ** rng.uniform(0, 16, k - 1)).astype(np.int64)
    idx = np.concatenate([[0], np.cumsum(gaps)]) + (0 if kind != "log" else 5)
    assert idx[-1] < 2 ** 31
    return idx.astype(np.int32)


def slot_bytes(stream):
    """A stream's trailer bit count in the max_bytes convention: whole words + 16."""
    nbits = int(stream[-8:].view("<i8")[0])
    return (nbits + 31) // 32 * 4 + 16


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", ["ones", "pow5", "pow17", "log"])
def test_elias_bound_holds_and_is_tight_at_equal_power_of_two_gaps(kind, k):
    from decentralizepy_amd import _lib
    L = _lib.lib()
    idx = index_list(kind, k)
    n = int(idx[-1]) + 1
    real = slot_bytes(oelias.encode(idx))
    bound = L.dpz_elias_bound_bytes(k, n)
    assert real <= bound <= L.dpz_elias_max_bytes(k)
    if kind != "log":
        assert bound == real


def test_elias_bound_at_the_ends_of_the_range():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    wide = np.array([0, 2 ** 31 - 1], dtype=np.int32)  # one 61-bit code
    assert slot_bytes(oelias.encode(wide)) <= L.dpz_elias_bound_bytes(2, 2 ** 31) \
        <= L.dpz_elias_max_bytes(2)
    assert L.dpz_elias_bound_bytes(1, 100) == 0 and L.dpz_elias_bound_bytes(0, 100) == 0
    assert L.dpz_elias_bound_bytes(7, 3) == L.dpz_elias_max_bytes(7)  # no such list: the loose cap
    assert L.dpz_elias_bound_bytes(8984, 89841) < 8984  # alpha = 0.1: under a byte an index


def test_argument_validation_without_gpu():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    ARG, UNSUP, WS = _lib.DPZ_ERR_ARG, _lib.DPZ_ERR_UNSUPPORTED, _lib.DPZ_ERR_WORKSPACE
    d = 4096  # never dereferenced: every call here must stop at a check
    need = L.dpz_wire_nodes_workspace_bytes(2, 3000)
    assert need >= 2 * 3 * 48 and need % 8 == 0
    assert L.dpz_wire_nodes_workspace_bytes(4, 3000) > need
    for m, count in ((0, 10), (2, -1), (2, 2 ** 30 + 1)):
        assert L.dpz_wire_nodes_workspace_bytes(m, count) == 0
    good = [[256, 512, 3000, 1024, 2048, 64, 64, 0], [0, 512, 1, 0, 0, 0, 0, 0]]

    def call(rows=good, m=None, tab=d, host=True, prec=0, sizes=d, status=d, ws=d, wsb=need):
        h = np.array(rows, dtype=np.int64).reshape(-1, 8)
        return L.dpz_wire_encode_nodes(len(h) if m is None else m, tab,
                                       ctypes.c_void_p(h.ctypes.data) if host else None, prec,
                                       sizes, status, ws, wsb, None)

    for bad in (dict(m=0), dict(m=-1), dict(tab=None), dict(host=False), dict(sizes=None),
                dict(status=None), dict(tab=d + 4), dict(sizes=d + 4), dict(status=d + 2),
                dict(ws=d + 4)):
        assert call(**bad) == ARG, bad
    for col, val in ((2, -1), (2, 2 ** 30 + 1), (1, 0), (2, 1), (2, 0), (0, 258), (1, 514),
                     (3, 1026), (4, 2050), (5, -4), (6, -4), (7, 1)):
        row = list(good[0])
        row[col] = val
        assert call([row, good[1]]) == ARG, (col, val)
    assert call([good[0], [0, 512, 1, 1024, 0, 64, 0, 0]]) == ARG  # an index slot, no indices
    assert call(prec=-1) == UNSUP and call([good[1]] * 65536, wsb=1 << 40) == UNSUP
    assert call(ws=None) == WS and call(wsb=need - 1) == WS and call(wsb=0) == WS
    assert L.dpz_abi_version() == 2  # symbols were added, nothing changed


def test_engines_refuse_the_wire_layer_on_the_cpu_stand_in_and_for_one_index_shares():
    from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound
    from decentralizepy_amd.gossip_topkacc import TopKAccRound
    from tests.jwins_ops import OracleJwinsOps
    from tests.test_cpu_topkacc_round import NP
    adj = [{1, 2}, {0, 2}, {0, 1}]
    x = torch.randn(3, 50, generator=torch.Generator().manual_seed(3))
    cpu = torch.device("cpu")
    ops = OracleJwinsOps("sym2", 4)
    engines = [JwinsBatchRound(adj, x, [0.1, 1.0], device=cpu, ops=ops, float_precision=16),
               TopKAccRound(adj, x, 0.1, **NP)]
    assert [e.float_precision for e in engines] == [16, 0]
    for eng in engines:
        eng.step()
        with pytest.raises(NotImplementedError, match="HIP codec"):
            eng.wire_bytes()
        with pytest.raises(NotImplementedError, match="HIP codec"):
            eng.wire_payload(0)
        with pytest.raises(ValueError, match="not one of this rank's nodes"):
            eng.wire_payload(3)
    for eng in (JwinsBatchRound(adj, x, [0.02, 1.0], device=cpu, ops=ops),  # k = round(1.18)
                TopKAccRound(adj, x, 0.02, **NP)):
        with pytest.raises(ValueError, match="k = 1 indices"):
            eng.wire_bytes()
    with pytest.raises(ValueError, match="float_precision"):
        TopKAccRound(adj, x, 0.1, float_precision=-1, **NP)
    with pytest.raises(RuntimeError, match="encoded"):
        TopKAccRound(adj, x.to(cpu), 0.1).wire_bytes()  # the HIP engine before its first round
