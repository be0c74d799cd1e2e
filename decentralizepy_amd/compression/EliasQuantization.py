"""Elias-gamma indices + quantised values, both byte-identical to the reference and both coded on
the device (reference compression/EliasQuantization.py:5-21, MRO ``Elias, Quantization``).

The index legs are :class:`Elias` (``compress_device`` / ``decompress_device``, asynchronous
decode), the value legs :class:`Quantization` (``compress_float_device`` /
``decompress_float_device``: ``float_precision`` levels per sign, ``num_bits`` bits per value).
"""
from .Elias import Elias
from .Quantization import Quantization


class EliasQuantization(Elias, Quantization):
    """Compress metadata and quantize parameters"""

    def __init__(self, float_precision: int = 2 ** 15 - 1, *args, **kwargs):
        Elias.__init__(self, *args, **kwargs)
        self.k = float_precision
