"""CPU: how dpz_decode_average_batch folds a batch (csrc/dpz_fold_walk.hip fold_batch_plan,
exported as dpz_debug_fold_batch_plan): node after node (path 0), the <= 4 sparse payloads kernel
(path 1) or the any-degree kernel (path 2), and the launches of the call.  The library launches
by the same function.  No GPU: the plan makes no device call."""
import ctypes

import pytest

from decentralizepy_amd import _lib

N = 100_003
FIELDS = ("path", "launches", "first", "passes")


def plan(counts, k=None, dense=None, n=N, flags=_lib.DPZ_FOLD_SELF, aligned=1):
    """counts: payloads per node; k / dense: per payload, flattened (default: n // 10, sparse)."""
    tot = sum(counts)
    k = [n // 10] * tot if k is None else k
    dense = [0] * tot if dense is None else dense
    out = (ctypes.c_int * len(FIELDS))()
    rc = _lib.lib().dpz_debug_fold_batch_plan(
        len(counts), n, (ctypes.c_int * max(1, len(counts)))(*counts),
        (ctypes.c_int64 * max(1, tot))(*k), (ctypes.c_int * max(1, tot))(*dense), flags, aligned,
        out)
    assert rc == 0
    return dict(zip(FIELDS, out))


def test_todays_kernel_keeps_its_batches():
    p = plan([4] * 22)
    assert (p["path"], p["launches"], p["first"], p["passes"]) == (1, 1, 22, 1)
    p = plan([4] * 23)
    assert (p["path"], p["launches"], p["first"], p["passes"]) == (1, 2, 22, 1)
    p = plan([1, 2, 3, 4])
    assert (p["path"], p["launches"]) == (1, 1)


def test_any_degree_batches():
    p = plan([16] * 8)
    assert (p["path"], p["launches"], p["first"], p["passes"]) == (2, 1, 8, 1)
    p = plan([6] + [1] * 6)                      # the 7-node star
    assert (p["path"], p["launches"], p["first"], p["passes"]) == (2, 1, 7, 1)
    # fullyConnected_16: 16 + 240 slots, two tables
    p = plan([15] * 16)
    assert (p["path"], p["launches"], p["first"], p["passes"]) == (2, 2, 9, 1)
    p = plan([95] * 2)                           # 96_node_fullyConnected, two of its nodes
    assert (p["path"], p["launches"], p["first"], p["passes"]) == (2, 6, 2, 6)
    # one node of more than 16: the others are finished after the first pass
    p = plan([17, 2, 16, 33])
    assert (p["path"], p["launches"], p["first"], p["passes"]) == (2, 3, 4, 3)
    # a mixed batch with one node of five keeps 22 nodes of <= 4 in one launch
    p = plan([5] + [4] * 21)
    assert (p["path"], p["launches"], p["first"]) == (2, 1, 22)


def test_a_dense_payload_takes_the_any_degree_kernel():
    dense = [0] * 36
    dense[7] = 1
    k = [N if d else N // 10 for d in dense]
    p = plan([3] * 12, k=k, dense=dense)
    assert (p["path"], p["launches"], p["first"], p["passes"]) == (2, 1, 12, 1)
    # every payload of every node dense
    p = plan([2, 2], k=[N] * 4, dense=[1] * 4)
    assert (p["path"], p["launches"]) == (2, 1)
    # a dense payload is a full row
    assert plan([2, 2], k=[N - 1] + [N // 10] * 3, dense=[1, 0, 0, 0])["path"] == 0


def test_node_after_node_batches():
    assert plan([4])["path"] == 0                                   # m = 1
    assert plan([4, 4], n=1023, k=[10] * 8)["path"] == 0
    assert plan([4, 4], n=1024, k=[10] * 8)["path"] == 1
    assert plan([3, 0, 3])["path"] == 0                             # a node without payloads
    assert plan([2, 2], k=[N // 10, 0, N // 10, N // 10])["path"] == 0   # an empty payload
    assert plan([5, 5], k=[N // 10] * 9 + [0])["path"] == 0
    assert plan([4, 4], aligned=0)["path"] == 0
    assert plan([5, 5], aligned=0)["path"] == 0
    assert plan([4, 4], flags=_lib.DPZ_FOLD_SELF | _lib.DPZ_FOLD_ZERO_BASE)["path"] == 0
    assert plan([5, 5], flags=_lib.DPZ_FOLD_SELF | _lib.DPZ_FOLD_ACCUMULATE)["path"] == 0
    both = _lib.DPZ_FOLD_SELF | _lib.DPZ_FOLD_ALSO_LOCAL
    assert plan([5, 5], flags=both)["path"] == 2
    assert plan([2, 2], k=[N] + [N // 10] * 3, dense=[1, 0, 0, 0], flags=both)["path"] == 0
    assert plan([2, 2], k=[N] + [N // 10] * 3, dense=[1, 0, 0, 0])["path"] == 2
    # node after node: at least one launch per node, and one per 16 payloads
    p = plan([4, 4], aligned=0)
    assert p["launches"] >= 2 and p["first"] == 1
    p = plan([33, 1], aligned=0)
    assert p["launches"] >= 4 and p["passes"] == 3


def test_plan_validates_arguments():
    L = _lib.lib()
    out = (ctypes.c_int * len(FIELDS))()
    c = (ctypes.c_int * 2)(4, 4)
    k = (ctypes.c_int64 * 8)(*([10] * 8))
    f = _lib.DPZ_FOLD_SELF
    assert L.dpz_debug_fold_batch_plan(2, N, c, k, None, f, 1, out) == 0
    assert out[0] == 1                                             # dense NULL: all sparse
    assert L.dpz_debug_fold_batch_plan(-1, N, c, k, None, f, 1, out) == _lib.DPZ_ERR_ARG
    assert L.dpz_debug_fold_batch_plan(2, 0, c, k, None, f, 1, out) == _lib.DPZ_ERR_ARG
    assert L.dpz_debug_fold_batch_plan(2, N, None, k, None, f, 1, out) == _lib.DPZ_ERR_ARG
    assert L.dpz_debug_fold_batch_plan(2, N, c, None, None, f, 1, out) == _lib.DPZ_ERR_ARG
    assert L.dpz_debug_fold_batch_plan(2, N, c, k, None, f, 1, None) == _lib.DPZ_ERR_ARG
    neg = (ctypes.c_int * 2)(4, -1)
    assert L.dpz_debug_fold_batch_plan(2, N, neg, k, None, f, 1, out) == _lib.DPZ_ERR_ARG


@pytest.mark.parametrize("counts", [[4] * 29, [4] * 30, [16] * 8, [16] * 9, [1] * 74])
def test_a_launch_holds_what_its_table_holds(counts):
    """A node takes one slot and one per payload of the launch's 146."""
    counts = [5] + counts[1:]  # (one node of five: the any-degree kernel)
    p = plan(counts)
    slots = 0
    first = 0
    for c in counts:
        if slots + 1 + c > 146:
            break
        slots += 1 + c
        first += 1
    assert p["path"] == 2 and p["first"] == first
    assert p["launches"] == (1 if first == len(counts) else 2)
