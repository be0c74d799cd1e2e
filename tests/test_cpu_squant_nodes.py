"""CPU: what the sparse rounds' quantiser (csrc/dpz_squant_nodes.hip) decides on the host: its
symbols, the argument checks (made on the host table before anything is enqueued), the row size,
and the refusals of the three engines' ``compression`` keyword."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

NAMES = ["dpz_squant_row_words", "dpz_squant_encode_nodes_workspace_bytes",
         "dpz_squant_encode_nodes", "dpz_squant_decode_nodes"]
ADJ = [{1, 2}, {0, 2}, {0, 1}]


def _engines():
    from decentralizepy_amd.gossip_jwins_batch import JwinsBatchRound, JwinsWaveletBatchRound
    from decentralizepy_amd.gossip_topkacc import TopKAccRound
    from tests.test_cpu_topkacc_round import NP
    x = torch.zeros(3, 64)
    return [(lambda **kw: TopKAccRound(ADJ, x, 0.1, **kw), NP),
            (lambda **kw: JwinsBatchRound(ADJ, x, [0.1, 1.0], level=2, **kw), dict(ops=object())),
            (lambda **kw: JwinsWaveletBatchRound(ADJ, x, [0.1, 1.0], wavelet="db4", level=2, **kw),
             dict(ops=object()))]


def test_symbols_and_abi():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include",
                               "dpz_codec.h")).read()
    declared = re.findall(r"^[a-z_0-9]+ (dpz_squant\w+)\(", header, re.M)
    assert sorted(declared) == sorted(NAMES) == sorted(n for n in _lib.SIGNATURES if "squant" in n)
    assert all(hasattr(L, n) for n in NAMES)
    assert L.dpz_abi_version() == 2  # symbols were added, nothing changed


@pytest.mark.parametrize("k, w", [(1, 2), (255, 9), (256, 10), (2 ** 30, 32)])
def test_row_words(k, w):
    from decentralizepy_amd import _lib
    L = _lib.lib()
    for count in (1, 33, 8193):
        assert L.dpz_squant_row_words(count, k) == 8 + -(-count * w // 32)
    for count, kk in ((0, k), (2 ** 30 + 1, k), (5, 0), (5, 2 ** 30 + 1)):
        assert L.dpz_squant_row_words(count, kk) == 0


def test_argument_validation_without_gpu():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    ARG, UNSUP, WS = _lib.DPZ_ERR_ARG, _lib.DPZ_ERR_UNSUPPORTED, _lib.DPZ_ERR_WORKSPACE
    d = 4096  # never dereferenced: every call here must stop at a check
    need = L.dpz_squant_encode_nodes_workspace_bytes(2, 3 * 8192 + 5)
    assert need == 2 * 4 * 8 and L.dpz_squant_encode_nodes_workspace_bytes(0, 10) == 0
    good = [[256, 3 * 8192 + 5, 1024, 8 + 8192], [260, 1, 2048, 8]]

    def enc(rows=good, m=None, tab=d, host=True, k=255, ws=d, wsb=need):
        h = np.array(rows, dtype=np.int64).reshape(-1, 4)
        return L.dpz_squant_encode_nodes(len(h) if m is None else m, tab,
                                         ctypes.c_void_p(h.ctypes.data) if host else None, k, ws,
                                         wsb, None)

    def dec(rows=good, m=None, tab=d, host=True, status=d):
        h = np.array(rows, dtype=np.int64).reshape(-1, 4)
        return L.dpz_squant_decode_nodes(len(h) if m is None else m, tab,
                                         ctypes.c_void_p(h.ctypes.data) if host else None, status,
                                         None)

    for bad in (dict(m=0), dict(m=-1), dict(tab=None), dict(host=False), dict(tab=d + 4)):
        assert enc(**bad) == ARG and dec(**bad) == ARG, bad
    for bad in (dict(k=0), dict(k=2 ** 30 + 1), dict(ws=d + 4)):
        assert enc(**bad) == ARG, bad
    for bad in (dict(status=None), dict(status=d + 2)):
        assert dec(**bad) == ARG, bad
    for col, val in ((0, 0), (0, 258), (2, 0), (2, 1026), (1, 0), (1, -1), (1, 2 ** 30 + 1),
                     (3, 7), (3, -1)):
        row = list(good[0])
        row[col] = val
        assert enc([row, good[1]]) == ARG and dec([good[1], row]) == ARG, (col, val)
    assert enc([good[1]] * 65536, wsb=1 << 40) == UNSUP and dec([good[1]] * 65536) == UNSUP
    assert enc(ws=None) == WS and enc(wsb=need - 1) == WS and enc(wsb=0) == WS


def test_engines_refuse_bad_configurations():
    for make, injected in _engines():
        with pytest.raises(ValueError, match="compression 'Lz4'"):
            make(compression="Lz4", **injected)
        for bad in (0, 2 ** 30 + 1):
            with pytest.raises(ValueError, match=r"\[1, 2\^30\]"):
                make(compression="EliasQuantization", float_precision=bad, **injected)
        for bad in (255.0, True, None):
            with pytest.raises(TypeError, match="must be an int"):
                make(compression="EliasQuantization", float_precision=bad, **injected)
        with pytest.raises(NotImplementedError, match="HIP codec"):
            make(compression="EliasQuantization", float_precision=255, **injected)


def test_default_construction_is_unchanged():
    for make, injected in _engines():
        eng = make(**injected)
        assert eng.compression is None and not eng._squant and not eng._coded
        assert eng.float_precision == 0
