"""GPU: the reference quantiser on the device (csrc/dpz_quant.hip behind codec.quant_encode /
quant_decode and the Quantization / EliasQuantization classes) and PlainAverageSharing.  Everything
is compared bit for bit with the numpy restatement (tests/quantization_ops.py) and with the
reference's recorded streams and plugin runs (tests/golden/quantization*,
make_golden_quantization.py) — never with the numpy of the machine the test runs on."""
import pickle

import numpy as np
import pytest
import torch

from tests import quantization_ops as ops

pytestmark = pytest.mark.gpu

PACK_SIZES = [31, 32, 33, 63, 64, 65, 255, 256, 257]


def _block():
    from decentralizepy_amd import codec
    return codec.quant_block_elems()


def _stat_sizes():
    B = _block()
    return sorted(set(ops.SUM_SIZES + [B - 1, B, B + 1, 3 * B + 17]))


def _encode(x, k, dev, ws=None):
    """(scale, to_send, info) of the device encode of a host array."""
    from decentralizepy_amd import codec
    body, info = codec.quant_encode(torch.from_numpy(x).to(dev), k, workspace=ws)
    to_send = np.concatenate([np.array([info.padding, info.w], np.uint8), body.cpu().numpy()])
    return info.scale, to_send, info


def _decode(scale, to_send, dev):
    from decentralizepy_amd import codec
    body = np.zeros((to_send.size - 2 + 3) // 4 * 4, np.uint8)
    body[:to_send.size - 2] = to_send[2:]
    n = (8 * (to_send.size - 2) - int(to_send[0])) // int(to_send[1])
    return codec.quant_decode(torch.from_numpy(body).to(dev), n, int(to_send[1]),
                              scale).cpu().numpy()


def _check_stats(x, dev, ws):
    _, _, info = _encode(x, 32767, dev, ws)
    assert ops.bits_of(info.max_abs) == ops.bits_of(np.max(np.abs(x))), x.size
    assert ops.bits_of(info.abs_sum) == ops.bits_of(ops.abs_sum(x)), \
        (x.size, info.abs_sum, ops.abs_sum(x))


@pytest.mark.parametrize("n", _stat_sizes())
def test_statistics_equal_the_restatement(dev, n):
    from decentralizepy_amd import codec
    ws = codec.Workspace(dev)
    _check_stats(ops.recipe(n, n, 0.01), dev, ws)
    if n >= 3:
        _check_stats(ops.mixed(n, n), dev, ws)


def test_statistics_past_two_tiles_of_chunks(dev):
    """n = 2^22 + 8193 + 5: more chunk sums than one staged tile of the final chain, a full
    chunk after the tile edge and a short last chunk; normal and mixed-magnitude data."""
    from decentralizepy_amd import codec
    n = 2 ** 22 + 8193 + 5
    ws = codec.Workspace(dev)
    _check_stats(ops.recipe(11, n, 0.01), dev, ws)
    _check_stats(ops.mixed(12, n), dev, ws)


@pytest.mark.parametrize("name", ops.codec_ids())
def test_pack_and_unpack_equal_the_fixtures(dev, name):
    case, x, rec_to_send, rec_out = ops.load_case(name)
    scale, to_send, info = _encode(x, case["k"], dev)
    assert isinstance(scale, np.float32)
    out = _decode(scale, to_send, dev)
    ops.check_case(case, scale, to_send, out, rec_to_send, rec_out)
    if rec_to_send is not None:  # the device decode of the recorded stream itself
        rec_scale = np.array([case["scale_bits"]], np.uint32).view(np.float32)[0]
        got = _decode(rec_scale, rec_to_send, dev)
        np.testing.assert_array_equal(got.view(np.uint32), rec_out.view(np.uint32))


@pytest.mark.parametrize("k", ops.KS)
def test_pack_equals_the_restatement_at_word_edges(dev, k):
    from decentralizepy_amd import codec
    B = _block()
    ws = codec.Workspace(dev)
    for n in PACK_SIZES + [B - 1, B + 1]:
        x = ops.recipe(7 * n + k % 1000, n, 0.01)
        scale, to_send, _ = _encode(x, k, dev, ws)
        ref_scale, ref = ops.encode(x, k)
        assert ops.bits_of(scale) == ops.bits_of(ref_scale), (n, k)
        np.testing.assert_array_equal(to_send, ref, err_msg=str((n, k)))
        out = _decode(scale, to_send, dev)
        np.testing.assert_array_equal(out.view(np.uint32),
                                      ops.decode(ref_scale, ref).view(np.uint32))


def test_unaligned_and_two_d_inputs(dev):
    """A view that starts 4 bytes into its buffer takes the scalar loads; 2-D input flattens."""
    from decentralizepy_amd.compression.Quantization import Quantization
    x = ops.recipe(3, 10_001, 0.01)
    t = torch.from_numpy(x).to(dev)
    q = Quantization(255)
    scale, to_send = pickle.loads(q.compress_float_device(t[1:]))
    ref_scale, ref = ops.encode(x[1:], 255)
    assert ops.bits_of(scale) == ops.bits_of(ref_scale)
    np.testing.assert_array_equal(to_send, ref)
    scale, to_send = pickle.loads(q.compress_float(x[:10_000].reshape(100, 100).astype(np.float64)))
    ref_scale, ref = ops.encode(x[:10_000], 255)
    assert ops.bits_of(scale) == ops.bits_of(ref_scale)
    np.testing.assert_array_equal(to_send, ref)


@pytest.mark.parametrize("cls_name", ["Quantization", "EliasQuantization"])
def test_class_streams_interoperate(dev, cls_name):
    """compress_float_device -> a wire value the restatement (a reference node) decodes to the
    values decompress_float_device gives, on the synchronous and the asynchronous path."""
    import importlib
    cls = getattr(importlib.import_module("decentralizepy_amd.compression." + cls_name), cls_name)
    for k, n in ((32767, 20_001), (7, 1000), (2 ** 30, 33)):
        comp = cls(float_precision=k)
        x = ops.recipe(n + k % 100, n, 0.01)
        blob = comp.compress_float_device(torch.from_numpy(x).to(dev))
        assert isinstance(blob, bytes) and comp.value_count(blob) == n
        scale, to_send = pickle.loads(blob)
        assert isinstance(scale, np.float32)
        ref_scale, ref = ops.encode(x, k)
        assert ops.bits_of(scale) == ops.bits_of(ref_scale)
        np.testing.assert_array_equal(to_send, ref)
        want = ops.decode(scale, to_send)
        got = comp.decompress_float_device(blob, device=dev)
        assert got.is_cuda and got.dtype == torch.float32
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        got = comp.decompress_float_device(blob, device=dev, status=status)
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert int(status.item()) == 0
        host = comp.decompress_float(blob)
        assert isinstance(host, np.ndarray) and host.dtype == np.float32
        np.testing.assert_array_equal(host.view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(np.frombuffer(comp.compress_float(x), np.uint8),
                                      np.frombuffer(blob, np.uint8))


def test_float64_scale_decodes_in_double(dev):
    """A sender's Python-float scale multiplies in fp64 (int32 array * float), as numpy does."""
    from decentralizepy_amd.compression.Quantization import Quantization
    _, to_send = ops.encode(ops.recipe(9, 1000, 0.01), 2 ** 30 - 1)
    scale = 1.0 / 3.0
    got = Quantization().decompress_float(pickle.dumps((scale, to_send)))
    np.testing.assert_array_equal(got.view(np.uint32), ops.decode(scale, to_send).view(np.uint32))


def test_bad_inputs_raise(dev):
    from decentralizepy_amd.compression.Quantization import Quantization
    q = Quantization(255)
    n = _block() + 5
    for poison in (np.nan, np.inf, -np.inf):
        x = ops.recipe(1, n)
        x[n - 2] = poison
        with pytest.raises(ValueError):
            q.compress_float_device(torch.from_numpy(x).to(dev))
    with pytest.raises(ValueError):
        q.compress_float_device(torch.zeros(n, device=dev))
    with pytest.raises(ValueError):
        q.compress_float_device(torch.zeros(0, device=dev))
    with pytest.raises(TypeError):
        Quantization(None).compress_float_device(torch.ones(4, device=dev))
    # and the compressor still works afterwards
    x = ops.recipe(2, 100, 0.01)
    np.testing.assert_array_equal(pickle.loads(q.compress_float(x))[1], ops.encode(x, 255)[1])


def test_malformed_streams_raise_on_the_async_path_and_leave_the_status_word(dev):
    from decentralizepy_amd.compression.EliasQuantization import EliasQuantization
    comp = EliasQuantization()
    x = ops.recipe(4, 100, 0.01)
    scale, to_send = pickle.loads(comp.compress_float_device(torch.from_numpy(x).to(dev)))
    status = torch.full((1,), 5, dtype=torch.int32, device=dev)
    bad = [pickle.dumps((scale, to_send[:-1])), pickle.dumps((scale, to_send, 0)),
           pickle.dumps(("x", to_send)), b"junk",
           pickle.dumps((scale, np.concatenate([[np.uint8(0), np.uint8(40)], to_send[2:]])))]
    for blob in bad:
        with pytest.raises(ValueError):
            comp.decompress_float_device(blob, device=dev, status=status)
        with pytest.raises(ValueError):
            comp.decompress_float_device(blob, device=dev)
    good = comp.decompress_float_device(pickle.dumps((scale, to_send)), device=dev, status=status)
    np.testing.assert_array_equal(good.cpu().numpy().view(np.uint32),
                                  ops.decode(scale, to_send).view(np.uint32))
    assert int(status.item()) == 5  # never written: nothing is left for the device to find


@pytest.mark.parametrize("name", ops.plugin_ids())
def test_plugin_replays_reference_run(dev, tmp_path, name):
    plugin = ops.replay_plugin(name, tmp_path)
    if name.startswith("plain"):
        sc, _ = ops.load_plugin(name)
        assert plugin.received_this_round == len(sc["neighbours"])


def test_plain_average_constructor_and_wire(dev, tmp_path):
    from decentralizepy_amd.sharing.PlainAverageSharing import PlainAverageSharing
    from decentralizepy_amd.sharing.Sharing import Sharing
    from tests import scenario
    model = scenario.make_model([3, 4, 5])
    p = PlainAverageSharing(0, 0, None, scenario._Mapping(), scenario._Graph([1, 2]), model, None,
                            str(tmp_path))
    assert isinstance(p, Sharing) and p.received_this_round == 0
    for data in (p.get_data_to_send(), p.get_data_to_send(degree=4), p.get_data_to_send(1, x=2)):
        assert list(data) == ["params", "iteration"]
