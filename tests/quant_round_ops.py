"""numpy restatement of the reference's QUANTISED full-model rounds — TEST INFRASTRUCTURE ONLY —
and the recorded reference runs (tests/golden/quant_round.json + quant_round_*.npz,
make_golden_quant_round.py).

``NumpyQuantRound`` is tests/epidemic_ops.py's node-by-node engine with every sender's model
passed through the restated quantiser (tests/quantization_ops.py ``encode`` / ``decode``) before
the fold; a receiver's own term is its fp32 model.  It is the yardstick of the engines in
decentralizepy_amd/gossip_quant.py where no fixture exists (other graphs, other sizes).
"""
import json
import os

import numpy as np

from tests import epidemic_ops as eops
from tests import quantization_ops as qops

GOLDEN = eops.GOLDEN
f32 = np.float32
RUNS = ["fullshare6_q255", "el_d7_q32767", "el_d1_q32767"]


def fold(local, payloads, weights, w_self):
    """The fold of ``(scale, to_send)`` wire values with the receiver's own fp32 model."""
    return eops.fold(local, [qops.decode(s, t) for s, t in payloads], weights, w_self)


class NumpyQuantRound(eops.NumpyRound):
    """Every node of a topology, one synchronous quantised round per ``step()``, node by node."""

    def __init__(self, adj, x, float_precision, degree=None, random_seed=None, senders=None):
        super().__init__(adj, x, degree, random_seed, senders)
        self.k = float_precision
        self.wire = None  # of the last round: every node's (scale, to_send)

    def step(self):
        if self.full:
            lists = eops.mh_lists(self.adj)
        else:
            self.send_sets = [set(s) for s in self.senders(self.round)]
            lists = []
            for i, got in enumerate(eops.receive_lists(self.adj, self.send_sets)):
                w = 1 / (len(got) + 1)
                lists.append((got, [w] * len(got), w))
                if got:
                    self.received_this_round[i] = len(got)
        self.wire = [qops.encode(row, self.k) for row in self.x]
        dec = [qops.decode(s, t) for s, t in self.wire]
        self.x = np.stack([eops.fold(self.x[i], [dec[j] for j in s], w, ws)
                           for i, (s, w, ws) in enumerate(lists)])
        self.round += 1


# ---- the recorded reference runs ----------------------------------------------------------------
def runs():
    with open(os.path.join(GOLDEN, "quant_round.json")) as f:
        return json.load(f)["runs"]


_npz = {}


def load(name):
    """(meta, arrays): a run's record; ``arrays["last"]`` the models after its last round,
    ``arrays["to_send_<u>"]`` the stored round-0 wire values."""
    meta = next(r for r in runs() if r["name"] == name)
    if name not in _npz:
        _npz[name] = dict(np.load(os.path.join(GOLDEN, f"quant_round_{name}.npz")))
    return meta, _npz[name]


graph = eops.graph
initial_models = eops.initial_models


def check_round(meta, arrays, r, models, lo=0, received=None, send_sets=None):
    """Rows [lo, lo + len(models)) after round r against the record."""
    eops.check_round(meta, arrays["last"], r, models, lo=lo, received=received,
                     send_sets=send_sets)


def check_wire(meta, arrays, q, scale, to_send):
    """Node q's round-0 wire value against the record."""
    rec = meta["wire"][q]
    to_send = np.asarray(to_send)
    assert isinstance(scale, np.float32) and to_send.dtype == np.uint8
    assert qops.bits_of(scale) == rec["scale_bits"], (q, qops.bits_of(scale), rec["scale_bits"])
    assert (int(to_send[0]), int(to_send[1])) == (rec["padding"], rec["w"]), q
    assert to_send.size == 2 + (meta["n"] * rec["w"] + 7) // 8
    assert qops.sha(to_send[2:]) == rec["body_sha"], q
    if f"to_send_{q}" in arrays:
        np.testing.assert_array_equal(to_send, arrays[f"to_send_{q}"])
