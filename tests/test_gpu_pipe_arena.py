"""GPU tests of the merged step kernel's LDS arena (pipe_step_kernel, dpz_topk_sampled.hip): the
filter, select and compact parts of a launch overlay one block of LDS, so a part that read a word
it had not written would see what another part's block left there.  DPZ_PIPE_POISON (diagnostic
build) fills the arena with all-ones before a block's part starts; with the switch on and off
the pipelined schedule (dpz_encode_replace_batch_ws) must give idx, val, out and counter bits
equal to the plain enqueue's (dpz_encode_replace_batch)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# n = 2^18 is the smallest sampled-path size: 256 wave segments, 64 filter blocks, so the tail's
# blocks outnumber the filter's in a merged launch.  k = n / 32 is the pipelined schedule's upper
# bound (the most candidates per segment); 2^18 + 3 has the ragged end (n % 4 != 0).
# The pipelined grid's cap of 4096 segments (1024 filter blocks, 4 per CU) holds from n = 2^24
# up: that size runs on one stream only (4 node states of 64 MiB), and n = 2^22, the smallest
# size that fills 4096 segments, runs on 1 and 3 streams with the cap forced (DPZ_WPIPE).
SIZES = [(1 << 18, (1 << 18) // 100, (1, 3), None), (1 << 18, (1 << 18) // 32, (1, 3), None),
         ((1 << 18) + 3, ((1 << 18) + 3) // 100, (1, 3), None),
         (1 << 22, (1 << 22) // 100, (1, 3), 4096), (1 << 24, (1 << 24) // 100, (1,), None)]
CASES = [pytest.param(n, k, S, wpipe, poison, id=f"{n}-{k}-{S}-{wpipe}-{poison}")
         for n, k, streams, wpipe in SIZES for S in streams for poison in (0, 1)]
PER_STREAM = 4  # filter only, filter + select, the full merged launch, then both drain launches
KEYS = ("idx", "val", "out", "counter")


@functools.lru_cache(maxsize=None)
def _host(n, k, m):
    """The node states of a case on the host, generated once and left unchanged."""
    g = torch.Generator().manual_seed(7000 + n % 1000 + k)
    out = []
    for _ in range(m):
        x = torch.randn(n, generator=g)
        out.append((x, x - 0.01 * torch.randn(n, generator=g)))
    return out


def _nodes(dev, n, k, m):
    nodes = []
    for x, x0 in _host(n, k, m):
        nodes.append(dict(x=x.to(dev), x0=x0.to(dev),
                          counter=torch.zeros(n, dtype=torch.int32, device=dev),
                          idx=torch.arange(k, dtype=torch.int32, device=dev) * 7,
                          val=torch.zeros(k, dtype=torch.float32, device=dev),
                          out=torch.empty(n, dtype=torch.float32, device=dev)))
    return nodes


def _batch(dev, nodes, n, k, S):
    from decentralizepy_amd import codec
    m = len(nodes)
    return codec.NodeStepBatch(nodes, n, k, [torch.cuda.Stream(dev) for _ in range(S)],
                               [codec.Workspace(dev) for _ in range(S)],
                               decode_src=lambda j: (j - S) % m)


def _bits(nodes):
    return [{key: d[key].cpu().numpy().view(np.uint32) for key in KEYS} for d in nodes]


@functools.lru_cache(maxsize=None)
def _plain(dev, n, k, S):
    """Two runs of the plain enqueue (the second with every encode hinted), computed once per
    case and left unchanged."""
    from decentralizepy_amd import _lib
    from decentralizepy_amd._lib import (DPZ_BATCH_DECODE, DPZ_BATCH_ENCODE, DPZ_BATCH_HINT,
                                         DPZ_BATCH_HINT_ALL)
    nodes = _nodes(dev, n, k, S * PER_STREAM)
    b = _batch(dev, nodes, n, k, S)
    b.sticky_status(clear=True)
    for hint in (DPZ_BATCH_HINT, DPZ_BATCH_HINT_ALL):
        rc = _lib.lib().dpz_encode_replace_batch(
            b.m, DPZ_BATCH_ENCODE | DPZ_BATCH_DECODE | hint, b._x, b._x0, b.n, b.k, b._cnt,
            b._idx, b._val, b._rl, b._ri, b._rv, b.k, b._ro, b._ws, b._ws_bytes, b._dws,
            b._dws_bytes, b._S, b._streams)
        assert rc == 0
        torch.cuda.synchronize()
    assert b.sticky_status() == 0
    return _bits(nodes)


@pytest.mark.parametrize("n,k,streams,wpipe,poison", CASES)
def test_pipelined_equals_plain_enqueue_with_poisoned_arena(dev, diag_lib, monkeypatch, n, k,
                                                            streams, wpipe, poison):
    from decentralizepy_amd._lib import DPZ_BATCH_DECODE, DPZ_BATCH_ENCODE, DPZ_BATCH_HINT
    ref = _plain(dev, n, k, streams)
    monkeypatch.setenv("DPZ_PIPE_POISON", str(poison))
    if wpipe:
        monkeypatch.setenv("DPZ_WPIPE", str(wpipe))
    m = streams * PER_STREAM
    nodes = _nodes(dev, n, k, m)
    b = _batch(dev, nodes, n, k, streams)
    b.sticky_status(clear=True)
    for _ in range(2):  # the first run primes the workspaces, the second is hinted throughout
        b.run(DPZ_BATCH_ENCODE | DPZ_BATCH_DECODE | DPZ_BATCH_HINT)
        assert b.pipelined == m
        torch.cuda.synchronize()
    assert b.sticky_status() == 0
    for j, (got, want) in enumerate(zip(_bits(nodes), ref)):
        for key in KEYS:
            np.testing.assert_array_equal(got[key], want[key], err_msg=f"node {j} {key}")
