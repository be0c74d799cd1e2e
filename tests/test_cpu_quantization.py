"""CPU: the numpy restatement of the reference quantiser (tests/quantization_ops.py) equals the
reference's own recorded streams (tests/golden/quantization*.{json,npz},
make_golden_quantization.py) bit for bit, its summation order is numpy's, and the host side of the
device classes (header validation, constructor and argument errors) behaves without a GPU."""
import pickle

import numpy as np
import pytest

from tests import quantization_ops as ops


@pytest.mark.parametrize("name", ops.codec_ids())
def test_restatement_equals_reference_fixture(name):
    case, x, rec_to_send, rec_out = ops.load_case(name)
    scale, to_send = ops.encode(x, case["k"])
    ops.check_case(case, scale, to_send, ops.decode(scale, to_send), rec_to_send, rec_out)
    if rec_to_send is not None:  # and the restated decode reads the recorded stream itself
        out = ops.decode(np.array([case["scale_bits"]], np.uint32).view(np.float32)[0], rec_to_send)
        np.testing.assert_array_equal(out.view(np.uint32), rec_out.view(np.uint32))


def test_observed_widths():
    widths = {c["k"]: c["w"] for c in ops.codec_cases() if c["kind"] == "normal"}
    assert widths == {1: 2, 7: 4, 255: 9, 256: 10, 32767: 16, 2 ** 20: 22, 2 ** 30 - 1: 32}
    x = ops.recipe(1, 100, 0.01)
    assert ops.params(x, 2 ** 30)[3] == 32


@pytest.mark.parametrize("n", ops.SUM_SIZES)
def test_summation_order_is_numpys(n):
    for x in (ops.recipe(n, n, 0.01), ops.mixed(n, n) if n >= 3 else ops.recipe(n + 1, n)):
        a = np.abs(x)
        got, ref = ops.abs_sum(x), a.sum()
        assert ref.dtype == np.float32
        assert ops.bits_of(got) == ops.bits_of(ref), (n, got, ref)
        mean = np.float32(got / np.float32(n))
        assert ops.bits_of(mean) == ops.bits_of(np.mean(a))


def test_mixed_case_shows_the_chunked_order():
    """The fixture's input separates numpy's chunked order from one whole-array pairwise tree."""
    case, x, _, _ = ops.load_case("mixed")
    a = np.abs(x)
    assert ops.bits_of(ops.pairwise(a)) != ops.bits_of(ops.abs_sum(a))
    assert ops.bits_of(ops.abs_sum(a)) == ops.bits_of(a.sum())


def test_division_case_shows_the_division():
    case, x, _, _ = ops.load_case("division")
    norm = ops.params(x, case["k"])[1]
    assert np.any(np.rint(x * np.float32(np.float32(1) / norm)) != np.rint(x / norm))


def test_restatement_rejects_what_the_reference_rejects():
    for bad in (np.zeros(5, np.float32), np.array([1.0, np.nan], np.float32),
                np.array([1.0, np.inf], np.float32), np.zeros(0, np.float32)):
        with pytest.raises(ValueError):
            ops.encode(bad, 255)


# ---- the device classes, host side ---------------------------------------------------------------
def _stream(n=10, w=9, padding=None, scale=np.float32(0.5)):
    nbytes = (n * w + 7) // 8
    pad = (8 - (n * w) % 8) % 8 if padding is None else padding
    return scale, np.concatenate([np.array([pad, w], np.uint8), np.zeros(nbytes, np.uint8)])


def test_header_validation_accepts_a_good_stream():
    from decentralizepy_amd.compression.Quantization import parse_stream
    scale, to_send = _stream()
    s, x, n, w = parse_stream(pickle.dumps((scale, to_send)))
    assert (s, n, w) == (0.5, 10, 9) and x.size == to_send.size
    # a Python float scale (a sender that fixed the rescaling) is a real scalar too
    assert parse_stream(pickle.dumps((0.25, to_send)))[0] == 0.25
    case, _, rec, _ = ops.load_case("k7_n33")
    assert parse_stream(ops.wire(np.float32(1), rec))[2:] == (33, case["w"])


@pytest.mark.parametrize("what", ["not_pickle", "triple", "list", "scale_str", "scale_array",
                                  "scale_bool", "int8", "two_d", "short", "w1", "w33",
                                  "padding8", "ragged", "not_array"])
def test_header_validation_raises(what):
    from decentralizepy_amd.compression.EliasQuantization import EliasQuantization
    from decentralizepy_amd.compression.Quantization import Quantization, parse_stream
    scale, good = _stream()
    bad = {
        "not_pickle": b"\x00\x01 not a pickle",
        "triple": pickle.dumps((scale, good, 1)),
        "list": pickle.dumps([scale, good]),
        "scale_str": pickle.dumps(("0.5", good)),
        "scale_array": pickle.dumps((np.ones(2, np.float32), good)),
        "scale_bool": pickle.dumps((True, good)),
        "int8": pickle.dumps((scale, good.astype(np.int8))),
        "two_d": pickle.dumps((scale, good.reshape(2, -1))),
        "short": pickle.dumps((scale, good[:2])),
        "w1": pickle.dumps(_stream(w=1)),
        "w33": pickle.dumps(_stream(w=33)),
        "padding8": pickle.dumps(_stream(padding=8)),
        "ragged": pickle.dumps((scale, np.concatenate([good, np.zeros(1, np.uint8)]))),
        "not_array": pickle.dumps((scale, bytes(good))),
    }[what]
    with pytest.raises(ValueError):
        parse_stream(bad)
    # the classes validate before they touch the device, on the asynchronous path too
    for comp in (Quantization(), EliasQuantization()):
        with pytest.raises(ValueError):
            comp.decompress_float(bad)
        with pytest.raises(ValueError):
            comp.decompress_float_device(bad, status=object())
        with pytest.raises(ValueError):
            comp.value_count(bad)


def test_constructor_matches_the_reference():
    from decentralizepy_amd.compression.Compression import Compression
    from decentralizepy_amd.compression.Elias import Elias
    from decentralizepy_amd.compression.EliasQuantization import EliasQuantization
    from decentralizepy_amd.compression.Quantization import Quantization
    assert Quantization().k == 2 ** 15 - 1 and EliasQuantization().k == 2 ** 15 - 1
    assert Quantization(255).k == 255 and Quantization(float_precision=7).k == 7
    assert EliasQuantization(float_precision=7).k == 7
    assert Quantization(float_precision=None).k is None  # as Sharing builds it without the key
    assert issubclass(Quantization, Compression)
    assert EliasQuantization.__mro__[1:3] == (Elias, Quantization)
    q = EliasQuantization()
    assert q.async_decode is True
    for name in ("compress_device", "decompress_device", "compress_float_device",
                 "decompress_float_device", "compress_float", "decompress_float", "value_count"):
        assert callable(getattr(q, name))
    # the known reference bug (max-normalised, mean-rescaled) is stated where users read it
    import decentralizepy_amd.compression.Quantization as mod
    assert "do NOT round-trip" in mod.__doc__


def test_config_module_paths_load():
    """What a config.ini names: module path + class name, as Node.init_sharing resolves them."""
    import importlib
    import inspect

    from decentralizepy_amd.sharing.Sharing import Sharing
    for package, name in (("decentralizepy_amd.compression.Quantization", "Quantization"),
                          ("decentralizepy_amd.compression.EliasQuantization",
                           "EliasQuantization"),
                          ("decentralizepy_amd.sharing.PlainAverageSharing",
                           "PlainAverageSharing")):
        assert inspect.isclass(getattr(importlib.import_module(package), name))
    from decentralizepy_amd.sharing.PlainAverageSharing import PlainAverageSharing
    assert issubclass(PlainAverageSharing, Sharing)
    # the reference constructor: Sharing's own parameter list, in order, same defaults
    assert (inspect.signature(PlainAverageSharing.__init__)
            == inspect.signature(Sharing.__init__))
    assert list(inspect.signature(PlainAverageSharing.get_data_to_send).parameters) == \
        ["self", "args", "kwargs"]


def test_errors_raised_before_the_device():
    from decentralizepy_amd.compression.EliasQuantization import EliasQuantization
    from decentralizepy_amd.compression.Quantization import Quantization
    x = np.ones(4, np.float32)
    for cls in (Quantization, EliasQuantization):
        with pytest.raises(TypeError):
            cls(float_precision=None).compress_float(x)
        for k in (0, -1, 2 ** 30 + 1, 2 ** 31):
            with pytest.raises(ValueError):
                cls(k).compress_float(x)
        with pytest.raises(ValueError):
            cls().compress_float(np.zeros(0, np.float32))


def test_entry_points_validate_arguments():
    from decentralizepy_amd import _lib
    L = _lib.lib()
    d = 4096  # never dereferenced: the checks come first
    assert L.dpz_quant_block_elems() >= 32 and L.dpz_quant_block_elems() % 32 == 0
    assert L.dpz_quant_workspace_bytes(0) == 0
    assert L.dpz_quant_workspace_bytes(1) < L.dpz_quant_workspace_bytes(2 ** 24)
    assert L.dpz_quant_workspace_bytes(2 ** 24) >= 4 * 2048
    ws = L.dpz_quant_workspace_bytes(100)
    assert L.dpz_quant_encode(d, 0, 255, d, 4096, d, d, ws, None) == 1001
    assert L.dpz_quant_encode(d, -5, 255, d, 4096, d, d, ws, None) == 1001
    assert L.dpz_quant_encode(d, 100, 0, d, 4096, d, d, ws, None) == 1001
    assert L.dpz_quant_encode(d, 100, 2 ** 30 + 1, d, 4096, d, d, ws, None) == 1001
    assert L.dpz_quant_encode(None, 100, 255, d, 4096, d, d, ws, None) == 1001
    assert L.dpz_quant_encode(d, 100, 255, d, 4096, d, d, 0, None) == 1002
    assert L.dpz_quant_decode(d, 4096, 0, 9, 1.0, d, None) == 1001
    assert L.dpz_quant_decode(d, 4096, 100, 1, 1.0, d, None) == 1001
    assert L.dpz_quant_decode(d, 4096, 100, 33, 1.0, d, None) == 1001
    assert L.dpz_quant_decode(d, 10, 100, 9, 1.0, d, None) == 1001  # a body shorter than n * w
    assert L.dpz_quant_decode(None, 4096, 100, 9, 1.0, d, None) == 1001
    assert L.dpz_abi_version() == 2
