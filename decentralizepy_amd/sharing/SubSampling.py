"""SubSampling plugin (random subsampling of the model, seed on the wire) on the MI355X codec.

Drop-in for the reference ``decentralizepy.sharing.SubSampling.SubSampling``
(``src/decentralizepy/sharing/SubSampling.py``): same constructor keyword arguments (``alpha,
dict_ordered, save_shared, metadata_cap, pickle, layerwise, compress, compression_package,
compression_class, float_precision``), same attributes (``random_generator``, ``seed``,
``init_model``, ``model.shared_parameters_counter``), same wire dict (``{seed, alpha,
params: fp32[k]}``), so a node running this class talks to reference nodes and to its CPU twin.

The payload names no indices: the receiver rebuilds the sender's Bernoulli mask from the seed with
``torch.rand(n, generator=g) <= alpha``.  Here that mask comes from a jump-ahead MT19937 on the
device (``codec.mt_mask``), bit for bit the torch CPU stream; ``layerwise=True`` draws the same
bits (the generator's stream continues across the per-tensor ``rand`` calls), so both forms use
the one flat mask.

Device path (HIP kernels, fp32, bit-exact with the reference's operation order):
  serialized_model    mask from ``seed + communication_round``, then one gather of the selected
                      values in index order (+ ``shared_parameters_counter[mask] += 1`` unless
                      layerwise, the reference's TODO); one 8-byte read of the count sizes params
  _averaging(_server) one mask per payload from its own seed and alpha, then one fold launch
                      that reads bit masks instead of index lists (``codec.mask_decode_average``)
  deserialized_model  mask, then replace (the fold with one payload of weight 1)
"""
import logging

import numpy as np
import torch

from .. import codec
from .._device import DeviceCounter, flatten_state, to_host
from .Sharing import Sharing


class SubSampling(Sharing):
    """This class implements the subsampling version of model sharing."""

    def __init__(self, rank, machine_id, communication, mapping, graph, model, dataset, log_dir,
                 alpha=1.0, dict_ordered=True, save_shared=False, metadata_cap=1.0, pickle=True,
                 layerwise=False, compress=False, compression_package=None,
                 compression_class=None, float_precision=None):
        super().__init__(rank, machine_id, communication, mapping, graph, model, dataset, log_dir,
                         compress, compression_package, compression_class, float_precision)
        self.alpha = alpha
        self.dict_ordered = dict_ordered
        self.save_shared = save_shared
        self.metadata_cap = metadata_cap

        self.random_generator = torch.Generator()
        # Will use the random device if supported by CPU, else uses the system time
        self.random_generator.seed()
        self.seed = self.random_generator.initial_seed()

        self.pickle = pickle  # accepted, unused (as in the reference)
        self.layerwise = layerwise
        logging.debug("subsampling pickling=" + str(pickle))

        if self.save_shared:
            # reference SubSampling.py:107-110: the condition holds for every rank, so the
            # shared-parameter log is never written
            if rank != 0 or rank != 1:
                self.save_shared = False

        with torch.no_grad():
            self.init_model = flatten_state(self.model.state_dict())
        self.model.shared_parameters_counter = DeviceCounter(
            torch.zeros(self.number_of_params, dtype=torch.int32, device=self.device))
        self._vals = None  # the gather's output buffer, grown on demand

    def _full(self):
        return self.alpha > self.metadata_cap  # Share fully (strict, as the reference)

    # ---- send ------------------------------------------------------------------------------
    def apply_subsampling(self):
        """reference SubSampling.py:129-182: (selected values, seed, alpha); the values are a
        device tensor in index order."""
        curr_seed = self.seed + self.communication_round  # is increased in step
        flat = self._local_flat_device()
        mask, rank_tab, count = codec.mt_mask(curr_seed, self.alpha, self.number_of_params,
                                              self.device, workspace=self.workspace)
        k = int(count.item())
        if self._vals is None or self._vals.numel() < k:
            self._vals = torch.empty(max(k, 1), dtype=torch.float32, device=self.device)
        counter = None if self.layerwise else self.model.shared_parameters_counter.device_tensor
        codec.mask_gather(flat, mask, rank_tab, self._vals, counter=counter, count=k)
        return self._vals[:k], curr_seed, self.alpha

    def serialized_model(self):
        """reference SubSampling.py:184-233"""
        if self._full():
            return super().serialized_model()
        with torch.no_grad():
            subsample, seed, alpha = self.apply_subsampling()
            if not self.dict_ordered:
                raise NotImplementedError
            m = dict()
            m["seed"] = seed
            m["alpha"] = alpha
            m["params"] = to_host(subsample, self.staging, "vals")
            return self.compress_data(m)

    # ---- receive -----------------------------------------------------------------------------
    def _device_payload(self, data):
        """Received (decompressed) payload -> (mask, rank_tab, vals, count) on the device: the
        sender's mask from its seed and alpha."""
        if self._full():
            return super()._device_payload(data)
        vals = self._h2d(data["params"], np.float32, "params")
        mask, rank_tab, count = codec.mt_mask(data["seed"], data["alpha"], self.number_of_params,
                                              self.device, workspace=self.workspace)
        return mask, rank_tab, vals, count

    def _fold(self, local, payloads, weights, w_self):
        if self._full():
            return super()._fold(local, payloads, weights, w_self)
        # the fold indexes vals by mask rank: every payload must hold exactly its mask's count
        # (the reference's T[binary_mask] = params raises on the same mismatch)
        counts = torch.cat([p[3] for p in payloads]).cpu().tolist()
        return codec.mask_decode_average(local, [p[:3] for p in payloads], weights, w_self,
                                         counts=counts)

    def deserialized_model(self, m):
        """reference SubSampling.py:235-308: the local model with the sender's selection
        replaced, as a state_dict of CPU tensors."""
        if self._full():
            return super().deserialized_model(m)
        m = self.decompress_data(m)
        with torch.no_grad():
            if not self.dict_ordered:
                raise NotImplementedError
            out = self._fold(self._local_flat_device(), [self._device_payload(m)], [1.0], None)
            return self._unflatten(to_host(out, self.staging, "result"))
