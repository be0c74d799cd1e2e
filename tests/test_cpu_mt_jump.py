"""CPU: the GF(2) jump-ahead of MT19937 (csrc/dpz_gf2.cpp) against numpy's MT19937.
dpz_mt_raw_host reaches every window through the same jump tables the mask kernels use (a jump
to each enclosing chunk, then stepping), so the characteristic polynomial, t^J mod phi and both
table levels are checked here without a GPU.  Also the host-side argument validation of the
device entry points and the SubSampling plugin's keyword surface."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import subsampling_ops as ops

WINDOW = 1300


def _lib():
    from decentralizepy_amd import _lib
    return _lib.lib()


def _raw(seed, start, count):
    out = np.empty(count, np.uint32)
    assert _lib().dpz_mt_raw_host(seed, start, count, out.ctypes.data) == 0
    return out


def _starts():
    S, C = _lib().dpz_mt_chunk_elems(), _lib().dpz_mt_coarse_chunks()
    starts = [0, S - 3, 3 * S + 17, ((C or 4) - 1) * S + 600]
    if C:
        starts += [C * S - 5, 2 * C * S + S + 1]
    return starts


def test_chunk_queries():
    L = _lib()
    S, C = L.dpz_mt_chunk_elems(), L.dpz_mt_coarse_chunks()
    assert S >= 624 and S % 64 == 0 and C >= 0
    for n in (1, 63, 64, 65, S, S + 1, 3 * S + 17):
        assert L.dpz_mt_rank_entries(n) >= -(-n // S)
        assert L.dpz_mt_mask_workspace_bytes(n) > 0
    assert L.dpz_mt_rank_entries(0) == -1 and L.dpz_mt_mask_workspace_bytes(0) == 0


@pytest.mark.parametrize("seed", [5489, 0xFFFFFFFF])
def test_raw_host_matches_numpy(seed):
    ref = ops.raw_outputs(seed, max(_starts()) + WINDOW)  # numpy's stream up to the last window
    for start in _starts():
        got = _raw(seed, start, WINDOW)
        np.testing.assert_array_equal(got, ref[start:start + WINDOW], err_msg=f"start {start}")


def test_raw_host_validates_arguments():
    L = _lib()
    out = np.empty(4, np.uint32)
    assert L.dpz_mt_raw_host(1, -1, 4, out.ctypes.data) == 1001
    assert L.dpz_mt_raw_host(1, 0, -1, out.ctypes.data) == 1001
    assert L.dpz_mt_raw_host(1, 0, 4, None) == 1001
    assert L.dpz_mt_raw_host(1, 2 ** 31 - 2, 4, out.ctypes.data) == 1001
    assert L.dpz_mt_raw_host(1, 0, 0, out.ctypes.data) == 0


def test_device_entry_points_validate_before_any_device_call():
    L = _lib()
    d = 4096  # never dereferenced: the checks come first
    assert L.dpz_mt_mask(1, 0.5, 0, d, d, d, d, 1 << 20, None) == 1001
    assert L.dpz_mt_mask(1, 0.5, 10, None, d, d, d, 1 << 20, None) == 1001
    assert L.dpz_mt_mask(1, 0.5, 10, d, None, d, d, 1 << 20, None) == 1001
    assert L.dpz_mt_mask(1, 0.5, 10, d, d, None, d, 1 << 20, None) == 1001
    assert L.dpz_mt_mask(1, 0.5, 10, d, d, d, None, 1 << 20, None) == 1001
    assert L.dpz_mask_gather(d, 0, d, d, d, None, None) == 1001
    assert L.dpz_mask_gather(None, 10, d, d, d, None, None) == 1001
    assert L.dpz_mask_gather(d, 10, None, d, d, None, None) == 1001
    assert L.dpz_mask_gather(d, 10, d, None, d, None, None) == 1001
    assert L.dpz_mask_gather(d, 10, d, d, None, None, None) == 1001
    ptrs = (ctypes.c_void_p * 1)(d)
    null = (ctypes.c_void_p * 1)(None)
    w = (ctypes.c_float * 1)(1.0)
    args = lambda **kw: [kw.get("local", d), kw.get("n", 10), kw.get("np", 1),  # noqa: E731
                         kw.get("mask", ptrs), kw.get("rank", ptrs), kw.get("vals", ptrs),
                         kw.get("w", w), 0.0, kw.get("flags", 0), kw.get("out", d), None]
    for bad in (dict(n=0), dict(np=0), dict(local=None), dict(out=None), dict(mask=None),
                dict(rank=None), dict(vals=None), dict(w=None), dict(mask=null), dict(vals=null),
                dict(flags=0x2)):
        assert L.dpz_mask_decode_average(*args(**bad)) == 1001, bad


def test_plugin_keyword_surface():
    """Constructor keywords of the reference sharing/SubSampling.py, verbatim."""
    from decentralizepy_amd.sharing.SubSampling import SubSampling
    params = inspect.signature(SubSampling.__init__).parameters
    assert list(params)[:9] == ["self", "rank", "machine_id", "communication", "mapping", "graph",
                                "model", "dataset", "log_dir"]
    want = dict(alpha=1.0, dict_ordered=True, save_shared=False, metadata_cap=1.0, pickle=True,
                layerwise=False, compress=False, compression_package=None,
                compression_class=None, float_precision=None)
    assert {k: p.default for k, p in list(params.items())[9:]} == want
    assert list(params)[9:] == list(want)
