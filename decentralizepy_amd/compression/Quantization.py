"""Fixed-ratio quantiser on the MI355X codec, byte-identical to the reference.

Drop-in for ``decentralizepy.compression.Quantization.Quantization`` (compression/
Quantization.py:10-132): ``__init__(float_precision=2**15-1)``, the attribute ``k``, and a wire
value a reference node decodes — ``pickle.dumps((np.float32(scale), uint8[padding, num_bits,
body...]))`` with ``num_bits`` bits per value instead of 32.  The statistics (max|x| and the fp32
sum of |x| in numpy's summation order), the quantisation and the bit packing run as HIP kernels
(``dpz_quant_encode``), the unpacking as ``dpz_quant_decode`` (csrc/dpz_quant.hip); the
reference loops over the values in Python.

Known reference behaviour, kept for wire parity: the values are normalised by ``max|x| / k`` but
rescaled by ``mean|x| / k``, so amplitudes do NOT round-trip (decoded values come out smaller by
mean|x| / max|x|).  The scale is chosen by the sender and travels in
the stream, so a sender that fixes it stays decodable here.

Differences at the edges: an all-zero, non-finite or empty input raises ValueError (the reference
raises ValueError for all-zero, NaN and empty inputs); ``float_precision`` must be an int in
[1, 2^30] (ValueError; the reference overflows at 2^31) and ``None`` raises TypeError on the first
compress, as in the reference; a 2-D input is flattened and cast to fp32.
"""
import pickle

import numpy as np
import torch

from .. import codec
from .._device import host_copy_into, pick_device
from .Compression import Compression
from .Elias import _grown, stage_up


def parse_stream(data):
    """``(scale, to_send, n, w)`` of a wire value; ValueError when it is not a quantised stream.
    Everything is checked from lengths on the host, so the decode needs no device-side error."""
    try:
        obj = pickle.loads(data)
    except Exception as e:  # a truncated or foreign pickle
        raise ValueError(f"quantised stream: not a pickle ({e})") from None
    if not isinstance(obj, tuple) or len(obj) != 2:
        raise ValueError("quantised stream: expected a (scale, bytes) pair")
    scale, x = obj
    if isinstance(scale, (bool, np.bool_)) or not isinstance(scale, (int, float, np.integer,
                                                                     np.floating)):
        raise ValueError("quantised stream: the scale is not a real scalar")
    if not isinstance(x, np.ndarray) or x.dtype != np.uint8 or x.ndim != 1 or x.size < 3:
        raise ValueError("quantised stream: expected a 1-D uint8 array of at least 3 bytes")
    padding, w = int(x[0]), int(x[1])
    if not 2 <= w <= 32:
        raise ValueError(f"quantised stream: {w} bits per value")
    if padding > 7:
        raise ValueError(f"quantised stream: padding {padding}")
    bits = 8 * (x.size - 2) - padding
    if bits % w:
        raise ValueError("quantised stream: the body is no whole number of values")
    return float(scale), x, bits // w, w


class Quantization(Compression):
    """Compress metadata and quantize parameters"""

    def __init__(self, float_precision: int = 2 ** 15 - 1, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.k = float_precision
        self._init_device()

    def _init_device(self):
        if not hasattr(self, "_ws"):
            self.device = None
            self._ws = None
            self._staging = None
            self._names = None

    def _dev(self, device=None):
        if device is not None:
            self.device = torch.device(device)
        if self.device is None:
            self.device = pick_device(0)
        if self._ws is None or self._ws.device != self.device:
            self._ws = codec.Workspace(self.device)
        return self.device

    def _checked_k(self):
        """``k`` as an int in [1, 2^30]: TypeError for None (the reference's ``mean / None``) or
        any other non-int, ValueError outside the range (the reference overflows at 2^31)."""
        k = self.k
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"float_precision must be an int, got {type(k).__name__}")
        if not 1 <= int(k) <= 2 ** 30:
            raise ValueError("float_precision must be in [1, 2^30]")
        return int(k)

    # ---- device surface ------------------------------------------------------------------------
    def compress_float_device(self, vals):
        """Device fp32 values -> the pickled wire value.  The body comes down through a pinned
        buffer kept with the compressor; the two header bytes are put in front during the copy
        from the pinned buffer into the array that is pickled."""
        k = self._checked_k()
        self._dev(vals.device)
        x = vals.reshape(-1)
        if x.dtype != torch.float32:
            x = x.float()
        if not x.is_contiguous():
            x = x.contiguous()
        body, info = codec.quant_encode(x, k, workspace=self._ws)
        nb = body.numel()
        pin = _grown(self._ws, "quant_out_pin", nb, dict(pin_memory=True))[:nb]
        pin.copy_(body, non_blocking=True)
        torch.cuda.current_stream(body.device).synchronize()
        to_send = np.empty(nb + 2, dtype=np.uint8)
        to_send[0], to_send[1] = info.padding, info.w
        host_copy_into(torch.from_numpy(to_send[2:]), pin)
        return pickle.dumps((np.float32(info.scale), to_send))

    def value_count(self, bytes):
        """The number of values a wire value holds (its header), without decoding it."""
        return parse_stream(bytes)[2]

    def decompress_float_device(self, bytes, device=None, status=None):
        """The pickled wire value -> device fp32 values.  The header is validated on the host
        (ValueError); with ``status`` (the round's device status word) the body goes up through
        the compressor's pinned ring and nothing synchronises — the word is never touched, as
        no error is left for the device to find."""
        scale, x, n, w = parse_stream(bytes)
        dev = self._dev(device)
        if n < 1:
            raise ValueError("quantised stream: no values")
        b = x[2:]
        need = ((b.size + 3) // 4) * 4
        if status is not None:
            return codec.quant_decode(stage_up(self, b, need, dev, "vals"), n, w, scale)
        ws = self._ws
        pin = _grown(ws, "quant_pin", need, dict(pin_memory=True))
        dbuf = _grown(ws, "quant_dev", need, dict(device=dev))
        host_copy_into(pin[:b.size], b)
        pin[b.size:need].zero_()
        dbuf[:need].copy_(pin[:need], non_blocking=True)
        out = codec.quant_decode(dbuf[:need], n, w, scale)
        torch.cuda.current_stream(dev).synchronize()  # pin and dbuf are free for the next call
        return out

    # ---- reference host surface ------------------------------------------------------------------
    def compress_float(self, x):
        """reference Quantization.py:28-91"""
        arr = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        self._checked_k()
        if arr.size == 0:
            raise ValueError("cannot quantise an empty array")
        return self.compress_float_device(torch.from_numpy(arr).to(self._dev()))

    def decompress_float(self, bytes):
        """reference Quantization.py:93-132"""
        return self.decompress_float_device(bytes).cpu().numpy()
