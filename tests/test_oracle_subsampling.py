"""CPU: the numpy restatement of SubSampling (tests/subsampling_ops.py) replays the reference's
own recorded runs (tests/golden/subsampling*.{json,npz}, make_golden_subsampling.py) bit-exactly,
and its mask rule is pinned against ``torch.rand`` directly."""
import numpy as np
import pytest
import torch

from tests import subsampling_ops as ops

ALPHAS = [0.0, 1e-8, 0.1, 5033165 / 2 ** 24 - 1e-9, 0.5, 1.0]
SEEDS = [0, 0xFFFFFFFF, 2 ** 32 + 5, 2 ** 63 + 12345]


def _torch_mask(seed, alpha, sizes):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.cat([torch.rand(size=(s,), generator=g) <= alpha for s in sizes]).numpy()


@pytest.mark.parametrize("name", ops.names())
def test_restatement_replays_reference_run(name):
    ops.replay_oracle(name)


@pytest.mark.parametrize("seed", SEEDS)
def test_mask_rule_matches_torch_rand(seed):
    n = 100_003
    for alpha in ALPHAS:
        ref = _torch_mask(seed, alpha, [n])
        np.testing.assert_array_equal(ops.mask(seed, alpha, n), ref, err_msg=str(alpha))
    # the fp32 rule, not the fp64 one: this alpha rounds up to 5033165 / 2^24 in fp32
    a = 5033165 / 2 ** 24 - 1e-9
    assert ops.threshold(a) == 5033165 and int(np.floor(a * 2 ** 24)) == 5033164
    assert ops.mask(seed, 0.0, n).sum() == (ops.raw_outputs(seed, n) & 0xFFFFFF == 0).sum()
    assert ops.mask(seed, 1.0, n).all() and ops.mask(seed, 2.0, n).all()
    assert not ops.mask(seed, -0.5, n).any() and not ops.mask(seed, float("nan"), n).any()


def test_layerwise_draws_the_flat_bit_string():
    """The generator's stream continues across calls: rand(a) then rand(b) is rand(a + b)."""
    for seed in (0, 2 ** 32 + 5):
        np.testing.assert_array_equal(_torch_mask(seed, 0.1, [19_900, 64, 37]),
                                      ops.mask(seed, 0.1, 20_001))


def test_seed_plus_round_carries_across_2_32():
    """curr_seed = seed + communication_round: only its low 32 bits seed the generator."""
    seed, n = 2 ** 32 - 1, 5_000
    for rnd in (0, 1, 2):
        np.testing.assert_array_equal(ops.mask(seed + rnd, 0.5, n),
                                      _torch_mask(seed + rnd, 0.5, [n]))
    np.testing.assert_array_equal(ops.mask(seed + 1, 0.5, n), ops.mask(0, 0.5, n))
    np.testing.assert_array_equal(ops.mask(seed + 2, 0.5, n), ops.mask(1, 0.5, n))


def test_pack_bit_order_and_length_check():
    m = np.zeros(70, bool)
    m[[0, 31, 32, 69]] = True
    np.testing.assert_array_equal(ops.pack(m), np.array([0x80000001, 1, 1 << 5], np.uint32))
    x = np.arange(1000, dtype=np.float32)
    p = ops.encode(x, 7, 0.5)
    np.testing.assert_array_equal(ops.replace(np.zeros(1000, np.float32), 7, 0.5, p),
                                  np.where(ops.mask(7, 0.5, 1000), x, 0))
    with pytest.raises(ValueError):
        ops.replace(x, 7, 0.5, p[:-1])
