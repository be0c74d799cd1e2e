"""GPU: SubSampling on the device.  The jump-ahead MT19937 mask (codec.mt_mask) against
``torch.rand(...) <= alpha`` on the CPU, the mask-ordered gather against ``x[mask]``, the
bit-mask fold against the numpy restatement (tests/subsampling_ops.py), and the plugin
(decentralizepy_amd/sharing/SubSampling.py) replaying the reference's recorded runs
(tests/golden/subsampling*, make_golden_subsampling.py) bit-exactly.  Sizes come from the
library's chunk queries: chunk edges, the 624-word state edges, and the two-level jump."""
from collections import deque

import numpy as np
import pytest
import torch

from tests import subsampling_ops as ops

pytestmark = pytest.mark.gpu

ALPHAS = [0.0, 1e-8, 0.1, 5033165 / 2 ** 24 - 1e-9, 0.5, 1.0]
SEEDS = [0, 0xFFFFFFFF, 2 ** 32 + 5, 2 ** 63 + 12345]


def _chunks():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    return int(L.dpz_mt_chunk_elems()), int(L.dpz_mt_coarse_chunks())


def _sizes():
    S, C = _chunks()
    sizes = [1, 31, 32, 33, 623, 624, 625, S - 1, S, S + 1, 3 * S + 17]
    if C:
        sizes += [C * S - 1, C * S + S + 5]
    return sizes


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _words(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("i,n", list(enumerate(_sizes())))
def test_mask_matches_torch_rand(dev, i, n):
    from decentralizepy_amd import codec
    S, _ = _chunks()
    everything = n == 3 * S + 17
    seeds = SEEDS if everything else [SEEDS[i % 4], SEEDS[(i + 1) % 4]]
    alphas = ALPHAS if everything else [ALPHAS[i % 6], ALPHAS[(i + 3) % 6]]
    ws = codec.Workspace(dev)
    for seed in seeds:
        g = torch.Generator()
        g.manual_seed(seed)
        u = torch.rand(size=(n,), generator=g)
        for alpha in alphas:
            ref = (u <= alpha).numpy()
            mask, _, count = codec.mt_mask(seed, alpha, n, dev, workspace=ws)
            assert int(count.item()) == int(ref.sum()), (n, seed, alpha)
            np.testing.assert_array_equal(_words(mask), ops.pack(ref), err_msg=str((n, seed, alpha)))


def test_mask_of_negative_or_nan_alpha_is_empty(dev):
    from decentralizepy_amd import codec
    for alpha in (-0.5, float("nan")):
        mask, _, count = codec.mt_mask(3, alpha, 1000, dev)
        assert int(count.item()) == 0 and not _words(mask).any()
    mask, _, count = codec.mt_mask(3, 2.0, 1000, dev)
    assert int(count.item()) == 1000
    np.testing.assert_array_equal(_words(mask), ops.pack(np.ones(1000, bool)))


@pytest.mark.parametrize("n", [33, None])
def test_gather_matches_boolean_index(dev, n):
    from decentralizepy_amd import codec
    S, _ = _chunks()
    n = n or 3 * S + 17
    x = ops.recipe(n, n)
    tx = torch.from_numpy(x).to(dev)
    counter = torch.zeros(n, dtype=torch.int32, device=dev)
    want = np.zeros(n, np.int32)
    for seed, alpha in ((5, 0.5), (6, 0.1)):  # the masks overlap: the counter reaches 2
        m = ops.mask(seed, alpha, n)
        mask, rank_tab, count = codec.mt_mask(seed, alpha, n, dev)
        k = int(count.item())
        assert k == m.sum()
        vals = torch.full((k + 3,), 7.0, dtype=torch.float32, device=dev)
        codec.mask_gather(tx, mask, rank_tab, vals, counter=counter)
        got = vals.cpu().numpy()
        np.testing.assert_array_equal(_bits(got[:k]), _bits(x[m]))
        assert (got[k:] == 7.0).all()  # nothing written past the count
        want += m
        np.testing.assert_array_equal(counter.cpu().numpy(), want)
    assert want.max() == 2 or n < 100
    # without a counter
    vals = torch.empty(max(k, 1), dtype=torch.float32, device=dev)
    codec.mask_gather(tx, mask, rank_tab, vals)
    np.testing.assert_array_equal(_bits(vals.cpu().numpy()[:k]), _bits(x[m]))
    np.testing.assert_array_equal(counter.cpu().numpy(), want)


@pytest.fixture(scope="module")
def fold_case(dev):
    """20 payloads at n = 3S + 17 with alphas mixed so that a nearly empty mask and a full one
    sit beside ordinary ones; shared by the fold tests (a prefix of it for fewer payloads)."""
    from decentralizepy_amd import codec
    S, _ = _chunks()
    n = 3 * S + 17
    rng = np.random.default_rng(16)
    local = rng.standard_normal(n).astype(np.float32)
    local[::7] = -0.0
    mix = [1e-8, 0.1, 0.5, 1.0]
    host, devp = [], []
    for p in range(20):
        seed, alpha = 1000 + 7 * p, mix[(p + 1) % 4]
        k = int(ops.mask(seed, alpha, n).sum())
        params = rng.standard_normal(k).astype(np.float32)
        params[::5] = -0.0
        mask, rank_tab, count = codec.mt_mask(seed, alpha, n, dev)
        assert int(count.item()) == k
        host.append((seed, alpha, params))
        devp.append((mask, rank_tab, torch.from_numpy(params).to(dev)))
    return local, torch.from_numpy(local).to(dev), host, devp


@pytest.mark.parametrize("npay", [1, 3, 16, 20])  # 20: two chained launches
@pytest.mark.parametrize("server", [False, True])
def test_fold_matches_restatement(dev, fold_case, npay, server):
    from decentralizepy_amd import codec
    local, tl, host, devp = fold_case
    if server:
        w, w_self = [1 / npay] * npay, None
    else:
        w = [1 / (max(npay, d) + 1) for d in range(2, 2 + npay)]
        wt = 0
        for v in w:
            wt += v
        w_self = 1 - wt
    out = codec.mask_decode_average(tl, devp[:npay], w, w_self).cpu().numpy()
    ref = ops.fold(local, host[:npay], w, w_self)
    np.testing.assert_array_equal(_bits(out), _bits(ref))


@pytest.mark.parametrize("name", ops.names())
def test_plugin_replays_reference_run(dev, tmp_path, name):
    ops.replay_plugin(name, tmp_path)


@pytest.mark.parametrize("name", ops.names())
def test_plugin_replays_reference_run_compressed(dev, tmp_path, name):
    """EliasFpzip's float leg is lossless: the same results with the params leg compressed."""
    ops.replay_plugin(name, tmp_path, compression_class="EliasFpzip")


def test_plugin_deserialized_model_and_short_payload(dev, tmp_path, monkeypatch):
    from decentralizepy_amd import codec
    from decentralizepy_amd.sharing.SubSampling import SubSampling
    from tests import scenario
    meta, arrays = ops.load("flat_a01")
    model = ops.make_model(meta["shape"])
    scenario.set_flat(model, arrays["x0"])
    plugin = SubSampling(0, 0, None, scenario._Mapping(), scenario._Graph([1, 2, 3]), model, None,
                         str(tmp_path), alpha=meta["alpha"])
    assert isinstance(plugin.seed, int) and plugin.save_shared is False
    assert plugin.init_model.shape == (meta["n"],)
    msgs = ops.neighbour_msgs(meta, arrays, 0)
    # deserialized_model: a state_dict of CPU tensors, the local model with the selection replaced
    m = {k: msgs[0][k] for k in ("seed", "alpha", "params")}
    sd = plugin.deserialized_model(dict(m))
    assert list(sd) == list(model.state_dict()) and not any(v.is_cuda for v in sd.values())
    flat = torch.cat([v.flatten() for v in sd.values()]).numpy()
    np.testing.assert_array_equal(
        _bits(flat), _bits(ops.replace(arrays["x0"], m["seed"], m["alpha"], m["params"])))
    # one element short: ValueError before any fold is launched, the model untouched
    calls = []
    real = codec.check  # called with the entry point's name after every native call
    monkeypatch.setattr(codec, "check", lambda rc, what: calls.append(what) or real(rc, what))
    msgs[1]["params"] = msgs[1]["params"][:-1]
    peers = {uid: deque([mm]) for uid, mm in zip([1, 2, 3], msgs)}
    with pytest.raises(ValueError):
        plugin._averaging(peers)
    assert "dpz_mask_decode_average" not in calls and "dpz_mt_mask" in calls
    np.testing.assert_array_equal(_bits(scenario.get_flat(model)), _bits(arrays["x0"]))


def test_codec_checks_lengths_against_counts(dev):
    """With the masks' counts in hand the codec layer refuses short or long vals on the host."""
    from decentralizepy_amd import codec
    n = 1000
    x = torch.zeros(n, device=dev)
    mask, rank_tab, count = codec.mt_mask(9, 0.5, n, dev)
    k = int(count.item())
    with pytest.raises(ValueError):
        codec.mask_gather(x, mask, rank_tab, torch.empty(k - 1, device=dev), count=k)
    for bad in (k - 1, k + 1):
        with pytest.raises(ValueError):
            codec.mask_decode_average(x, [(mask, rank_tab, torch.empty(bad, device=dev))], [1.0],
                                      counts=[k])
    out = codec.mask_decode_average(x, [(mask, rank_tab, torch.ones(k, device=dev))], [1.0],
                                    counts=[k])
    np.testing.assert_array_equal(out.cpu().numpy(), ops.mask(9, 0.5, n).astype(np.float32))
