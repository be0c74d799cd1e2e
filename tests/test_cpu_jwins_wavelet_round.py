"""CPU: ``JwinsWaveletBatchRound`` (decentralizepy_amd/gossip_jwins_batch.py) with the numpy oracle
standing in for the HIP kernels, against the reference semantics written out node by node
(tests/jwins_ops.direct_round_nodes), and its constructor's rules.  The device path is covered by
tests/test_gpu_wavelet_nodes.py."""
import numpy as np
import pytest
import torch

from oracle import wavelet as owav
from tests import jwins_round_ops as ops
from tests.jwins_ops import OracleJwinsOps, direct_round_nodes

CPU = torch.device("cpu")
ADJ = ops.adjacency(6, ops.EDGES_IRR6)


def _engine(x, wavelet, level, alphas=ops.TUTORIAL_ALPHAS):
    from decentralizepy_amd.gossip_jwins_batch import JwinsWaveletBatchRound
    return JwinsWaveletBatchRound(ADJ, torch.from_numpy(x), alphas, wavelet=wavelet, level=level,
                                  device=CPU, ops=OracleJwinsOps(wavelet, level))


@pytest.mark.parametrize("wavelet,level", [("db4", 4), ("db1", 2)])
def test_engine_equals_the_reference_node_by_node(wavelet, level):
    n, rounds = 1030, 3
    x = np.random.default_rng(40).standard_normal((6, n)).astype(np.float32)
    eng = _engine(x, wavelet, level)
    assert eng.M == owav.coeff_len(n, level, wavelet)
    for r in range(rounds):
        for u in range(6):
            eng.x[u] += torch.from_numpy(ops.perturbation(41, r, u, n))
        eng.step()
    nodes = direct_round_nodes(ADJ, x, ops.TUTORIAL_ALPHAS, rounds,
                               lambda r, u: ops.perturbation(41, r, u, n), level=level,
                               wavelet=wavelet)
    for u, nd in enumerate(nodes):
        for got, want in ((eng.x[u], nd.model), (eng.x0[u], nd.init), (eng.acc[u], nd.acc)):
            assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32)), u
        assert np.array_equal(eng.counter[u].numpy(), nd.counter), u


@pytest.mark.parametrize("wavelet,level", [("db1", 2), ("bior2.2", 3), ("db4", 4), ("sym2", 5),
                                           ("db10", 3), ("dmey", 1)])
def test_host_length_rule_equals_the_oracle(wavelet, level):
    from decentralizepy_amd import codec
    from decentralizepy_amd.gossip_jwins_batch import wavelet_coeff_len
    for n in (64, 101, 4100, 89834):
        assert wavelet_coeff_len(n, level, codec.filter_len(wavelet)) == owav.coeff_len(
            n, level, wavelet)


def test_engine_refuses_what_other_classes_serve():
    x = np.zeros((6, 40), np.float32)
    with pytest.raises(ValueError, match="JwinsBatchRound"):
        _engine(x, "sym2", 4, [0.1, 1.0])
    with pytest.raises(ValueError, match="JwinsRound"):
        _engine(x, "haar", 2, [0.1, 1.0])
    with pytest.raises(NotImplementedError, match="dmey level-1 wavedec unsupported for n=40"):
        _engine(x, "dmey", 1, [0.1, 1.0])  # 40 values, 62 taps
    with pytest.raises(NotImplementedError):
        _engine(x, "db4", 9, [0.1, 1.0])
    with pytest.raises(NotImplementedError, match="wavelet 'morl'"):
        _engine(x, "morl", 2, [0.1, 1.0])
    assert _engine(x, "sym2", 5, [0.1, 1.0]).M == owav.coeff_len(40, 5, "sym2")
