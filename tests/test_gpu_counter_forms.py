"""GPU: every form of the ring flush (dpz_counter_flush: scatter, dense sweep, sparse sectors and
the AUTO rule), the batched call over several counters (dpz_counter_flush_batch) and the step
batch's per-stream ring flush, all against ``np.add.at`` on the host.

Reference: sharing/PartialModel.py:205-207 (``shared_parameters_counter[indices] += 1`` each
round).  The sparse form reads and writes only the 64-byte sectors an entry touches, so every
counter starts from random values: a sector written back wrongly, or one that should not have
been written, shows."""
import functools

import numpy as np
import pytest
import torch

from oracle import topk as otopk

pytestmark = pytest.mark.gpu

CT = 8192            # counters per tile of the tiled forms
N = 3 * CT + 5       # ragged last tile whose last sector is partial
K = 300


def _mode(name):
    from decentralizepy_amd import _lib
    return {"scatter": _lib.DPZ_COUNTER_SCATTER, "sweep": _lib.DPZ_COUNTER_SWEEP,
            "sparse": _lib.DPZ_COUNTER_SPARSE, "auto": _lib.DPZ_COUNTER_AUTO}[name]


@functools.lru_cache(maxsize=None)
def _rounds(n, k, m, seed):
    """m random rounds, four identical rounds, the tile and sector edges, an empty round and a
    round with entries >= n (skipped): the lists and the increments np.add.at gives."""
    rng = np.random.default_rng(seed)
    lists = [np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32) for _ in range(m)]
    same = np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32)
    lists += [same] * 4
    lists.append(np.array([e for e in (0, 15, 16, CT - 1, CT, n - 1) if e < n], dtype=np.int32))
    lists.append(np.zeros(0, dtype=np.int32))
    lists.append(np.array([7, n, n + 5, 2 ** 30], dtype=np.int32))
    inc = np.zeros(n, dtype=np.int32)
    for a in lists:
        np.add.at(inc, a[a < n], 1)
    ring = np.concatenate(lists)
    seg = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).tolist()
    return ring, seg, inc


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("m", [1, 5, 70])
@pytest.mark.parametrize("mode", ["scatter", "sweep", "sparse", "auto"])
def test_every_form_matches_numpy(dev, mode, m, offset):
    """70 rounds take two launches of a tiled form; offset 1: a counter view that is not 16-byte
    aligned (the element-wise tile path), with a guard word on either side of it."""
    from decentralizepy_amd import codec
    ring, seg, inc = _rounds(N, K, m, 40 + m)
    base = np.random.default_rng(5).integers(0, 1000, size=N + offset + 1).astype(np.int32)
    store = torch.from_numpy(base).to(dev)
    counter = store[offset:offset + N]
    codec.counter_flush(counter, torch.from_numpy(ring).to(dev), seg, mode=_mode(mode))
    got = store.cpu().numpy()
    np.testing.assert_array_equal(got[offset:offset + N], base[offset:offset + N] + inc)
    assert got[offset + N] == base[offset + N]  # the word after the view
    if offset:
        assert got[0] == base[0]                # the word before it


@pytest.mark.parametrize("mode", ["auto", "sparse", "sweep", "scatter"])
def test_flush_batch_equals_single_calls(dev, mode):
    """Three counters of different n in one call on a side stream: one with an empty ring, one
    with 70 rounds (0.7 entries per counter, enough for the dense form; two passes of a tiled
    form), one with three rounds at 1 % (the scatter form under AUTO); the result equals three
    single calls and np.add.at."""
    from decentralizepy_amd import codec
    rng = np.random.default_rng(9)
    spec = [(CT, 0, 0), (100_003, 1000, 70), (2 ** 18, 2621, 3)]
    items, singles, want = [], [], []
    for n, k, m in spec:
        lists = [np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32) for _ in range(m)]
        lists.append(np.zeros(0, dtype=np.int32))
        ring = torch.from_numpy(np.concatenate(lists)).to(dev)
        if ring.numel() == 0:
            ring = torch.zeros(1, dtype=torch.int32, device=dev)
        seg = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).tolist()
        base = rng.integers(0, 1000, size=n).astype(np.int32)
        w = base.copy()
        for a in lists:
            np.add.at(w, a, 1)
        want.append(w)
        items.append((torch.from_numpy(base).to(dev), ring, seg, None))
        singles.append((torch.from_numpy(base).to(dev), ring, seg))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        codec.counter_flush_batch(items, mode=_mode(mode))
    for c, ring, seg in singles:
        codec.counter_flush(c, ring, seg, mode=_mode(mode))
    torch.cuda.synchronize()
    for (c, _, _, _), (s, _, _), w in zip(items, singles, want):
        np.testing.assert_array_equal(c.cpu().numpy(), w)
        np.testing.assert_array_equal(s.cpu().numpy(), w)


def test_flush_batch_rejects_before_any_launch(dev):
    """A bad item anywhere in the table refuses the call with no counter changed."""
    from decentralizepy_amd import codec
    good = torch.zeros(100, dtype=torch.int32, device=dev)
    ring = torch.arange(10, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):
        codec.counter_flush_batch([(good, ring, [0, 10], None),
                                   (good.clone(), ring, [0, 6, 4], None)])
    torch.cuda.synchronize()
    assert int(good.sum().item()) == 0


def test_step_batch_flushes_rings_per_stream(dev):
    """NodeStepBatch with rings, 4 states on 2 streams: after 5 runs and flush_rings() every
    counter equals the oracle's (the states do not change, so every run sends the same indices);
    a second flush_rings() with nothing pending changes nothing."""
    from decentralizepy_amd import codec
    from decentralizepy_amd._device import RingCounter
    from decentralizepy_amd._lib import DPZ_BATCH_DECODE, DPZ_BATCH_ENCODE, DPZ_BATCH_HINT
    n, S, m = 2 ** 18, 2, 4
    k = n // 100
    nodes, want = [], []
    for j in range(m):
        g = torch.Generator().manual_seed(700 + j)
        x = torch.randn(n, generator=g)
        x0 = x - 0.01 * torch.randn(n, generator=g)
        oi, _ = otopk.encode(x.numpy(), x0.numpy(), None, 0, k)
        w = np.zeros(n, dtype=np.int32)
        w[oi] = 5
        want.append(w)
        nodes.append(dict(x=x.to(dev), x0=x0.to(dev),
                          counter=torch.zeros(n, dtype=torch.int32, device=dev),
                          idx=torch.arange(k, dtype=torch.int32, device=dev) * 7,
                          val=torch.zeros(k, dtype=torch.float32, device=dev),
                          out=torch.empty(n, dtype=torch.float32, device=dev)))
    rings = [RingCounter(d["counter"]) for d in nodes]
    b = codec.NodeStepBatch(nodes, n, k, [torch.cuda.Stream(dev) for _ in range(S)],
                            [codec.Workspace(dev) for _ in range(S)],
                            decode_src=lambda j: (j - S) % m, rings=rings)
    for _ in range(5):
        b.run(DPZ_BATCH_ENCODE | DPZ_BATCH_DECODE | DPZ_BATCH_HINT)
    assert all(r.pending_rounds() == 5 for r in rings)
    for _ in range(2):
        b.flush_rings()
        torch.cuda.synchronize()
        assert all(r.pending_rounds() == 0 for r in rings)
        for d, w in zip(nodes, want):
            np.testing.assert_array_equal(d["counter"].cpu().numpy(), w)
    assert b.sticky_status() == 0
