"""CPU: what the batched wire decoder (csrc/dpz_wire_decode_nodes.hip) decides on the host: the
argument checks of ``dpz_wire_decode_nodes`` (made on the host table before anything is enqueued,
so no device is needed), the value slot bound ``dpz_fpz_bound_bytes`` and the refusals of
``TopKAccRound(coded_exchange=True)``.  The device path: tests/test_gpu_wire_decode_nodes.py."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import fpz as ofpz


def test_argument_validation_without_gpu():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    ARG, UNSUP, WS = _lib.DPZ_ERR_ARG, _lib.DPZ_ERR_UNSUPPORTED, _lib.DPZ_ERR_WORKSPACE
    d = 4096  # never dereferenced: every call here must stop at a check
    need = L.dpz_wire_decode_nodes_workspace_bytes(2, 6000, 3000)
    assert need >= 2 * 47 * 64 * 9 and need % 4 == 0
    assert L.dpz_wire_decode_nodes_workspace_bytes(4, 6000, 3000) > need
    big = 1024 * 64 * 128 + 4  # bytes of one chunk more than 1024 super maps
    for m, cap, count in ((0, 64, 10), (2, -1, 10), (2, 64, -1), (2, 64, 2 ** 30 + 1), (2, big, 10)):
        assert L.dpz_wire_decode_nodes_workspace_bytes(m, cap, count) == 0
    # {idx_in, val_in, count, idx_out, val_out, sizes, idx_cap, val_cap}; then a full share
    good = [[256, 512, 3000, 1024, 2048, 4096, 6000, 64], [0, 512, 1, 0, 2048, 4096, 0, 64]]

    def call(rows=good, m=None, tab=d, host=True, prec=0, status=d, ws=d, wsb=need):
        h = np.array(rows, dtype=np.int64).reshape(-1, 8)
        return L.dpz_wire_decode_nodes(len(h) if m is None else m, tab,
                                       ctypes.c_void_p(h.ctypes.data) if host else None, prec,
                                       status, ws, wsb, None)

    for bad in (dict(m=0), dict(m=-1), dict(tab=None), dict(host=False), dict(status=None),
                dict(tab=d + 4), dict(status=d + 2), dict(ws=d + 4)):
        assert call(**bad) == ARG, bad
    for col, val in ((2, -1), (2, 2 ** 30 + 1), (1, 0), (5, 0), (4, 0), (2, 1), (3, 0), (0, 258),
                     (1, 514), (3, 1026), (4, 2050), (5, 4100), (6, -4), (7, -4)):
        row = list(good[0])
        row[col] = val
        assert call([row, good[1]]) == ARG, (col, val)
    assert call([good[0], [0, 512, 1, 1024, 2048, 4096, 0, 64]]) == ARG  # a list, no stream
    assert call(prec=-1) == UNSUP and call([good[1]] * 65536, wsb=1 << 40) == UNSUP
    assert call([[256, 512, 3000, 1024, 2048, 4096, big, 64]], wsb=1 << 40) == UNSUP
    assert call(ws=None) == WS and call(wsb=need - 1) == WS and call(wsb=0) == WS
    assert L.dpz_abi_version() == 2  # symbols were added, nothing changed


@pytest.mark.parametrize("n", [1, 256, 257, 1500])
def test_fpz_bound_holds_for_blocks_spanning_all_exponent_bits(n):
    from decentralizepy_amd import _lib
    L = _lib.lib()
    assert L.dpz_fpz_bound_bytes(n, 0) == L.dpz_fpz_bound_bytes(n, 32) == L.dpz_fpz_max_bytes(n)
    assert L.dpz_fpz_bound_bytes(-1, 0) == 0 and L.dpz_fpz_bound_bytes(n, -1) == 0
    # exponents 0 and 255 in every block: the widest exponent plane (NaNs, infinities, denormals)
    bits = np.random.default_rng(n).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    bits[0::2] |= 0x7F800000
    bits[1::2] &= 0x807FFFFF
    for p in (9, 16):
        real = len(ofpz.encode(bits.view(np.float32), p))
        bound = L.dpz_fpz_bound_bytes(n, p)
        assert real <= bound < L.dpz_fpz_max_bytes(n)
        assert n % 256 or n == 1 or real == bound  # full blocks of 8-bit exponents: tight


def test_coded_exchange_refusals():
    from decentralizepy_amd.gossip_topkacc import TopKAccRound
    from tests.test_cpu_topkacc_round import NP
    adj = [{1, 2}, {0, 2}, {0, 1}]
    x = torch.zeros(3, 50)
    with pytest.raises(NotImplementedError, match="HIP codec"):
        TopKAccRound(adj, x, 0.1, coded_exchange=True, **NP)
    with pytest.raises(ValueError, match="k = 1 indices"):
        TopKAccRound(adj, x, 0.02, coded_exchange=True)
    with pytest.raises(ValueError, match="GossipRound") as err:
        TopKAccRound(adj, x, 0.1, compress=True, **NP)
    assert "compressed payloads" not in str(err.value)
    assert not TopKAccRound(adj, x, 0.1, **NP)._coded
