"""PlainAverageSharing plugin (plain averaging, no Metropolis-Hastings) over the MI355X codec.

Drop-in for the reference ``decentralizepy.sharing.PlainAverageSharing.PlainAverageSharing``
(``src/decentralizepy/sharing/PlainAverageSharing.py``; the class Epidemic Learning's
``tutorial/EpidemicLearning/config_EL.ini`` names): same constructor, ``received_this_round``,
a wire dict with ``iteration`` but no ``degree``, and every received model and the local one
weighted ``1 / (len(peer_deques) + 1)``.

What runs on the GPU: the average is the one ``dpz_decode_average`` launch of ``Sharing`` — the
neighbours' terms in deque order, the local term last, the reference's fp32 order
(PlainAverageSharing.py:82-114).  A compressor's payloads are decoded on the device first.
"""
import logging

import torch

from .Sharing import Sharing


class PlainAverageSharing(Sharing):
    """Class to do plain averaging instead of Metropolis Hastings"""

    def __init__(self, rank, machine_id, communication, mapping, graph, model, dataset, log_dir,
                 compress=False, compression_package=None, compression_class=None,
                 float_precision=None):
        super().__init__(rank, machine_id, communication, mapping, graph, model, dataset, log_dir,
                         compress, compression_package, compression_class, float_precision)
        self.received_this_round = 0

    def _averaging(self, peer_deques):
        """Averages the received models with the local model (reference :82-114)."""
        self.received_this_round = 0
        with torch.no_grad():
            weight = 1 / (len(peer_deques) + 1)
            payloads = []
            for n in peer_deques:
                self.received_this_round += 1
                data = peer_deques[n].popleft()
                iteration = data["iteration"]
                del data["iteration"]
                del data["CHANNEL"]
                logging.debug("Averaging model from neighbor {} of iteration {}".format(
                    n, iteration))
                data = self.decompress_data(data, device=True)
                payloads.append(self._device_payload(data))
            local = self._local_flat_device()
            out = self._fold(local, payloads, [weight] * len(payloads), weight)
            self._load_flat(out)
        self._post_step()
        self.communication_round += 1

    def get_data_to_send(self, *args, **kwargs):
        """reference :116-120: no ``degree`` on the wire."""
        self._pre_step()
        data = self.serialized_model()
        data["iteration"] = self.communication_round
        return data
