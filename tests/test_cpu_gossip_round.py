"""CPU: what the round engines share (decentralizepy_amd/gossip_round.py) — the sharding prologue
and the packed rows with their status words, on CPU tensors with a stub engine."""
import numpy as np
import pytest
import torch

from decentralizepy_amd.gossip_round import PackedRowRound, ShardedRound, shard, up4

ADJ = [set() for _ in range(16)]


def _sharded(n_nodes, rank=0, world=1, group=None, rows=None):
    lo, hi, _ = shard(n_nodes, world, rank)
    x = torch.zeros(hi - lo if rows is None else rows, 7)
    return ShardedRound(ADJ[:n_nodes], x, rank, world, group, None)


class _Stub(PackedRowRound):
    def __init__(self, n_nodes, rank=0, world=1, group=None):
        lo, hi, _ = shard(n_nodes, world, rank)
        super().__init__(ADJ[:n_nodes], torch.zeros(hi - lo, 3), rank, world, group, None)
        self._alloc_rows(self.HEADER + 4)


def test_up4():
    assert [up4(v) for v in (0, 1, 4, 5, 8.0)] == [0, 4, 4, 8, 8]


def test_one_rank_without_a_group_exchanges_in_place():
    eng = _sharded(5)
    assert not eng.coll and (eng.lo, eng.hi, eng.per, eng.m) == (0, 5, 5, 5)
    assert eng.per == eng.n_nodes and eng.N == 7 and eng.round == 0
    assert eng.device == torch.device("cpu")


def test_a_group_makes_one_rank_collective():
    assert _sharded(5, group="g").coll and _sharded(5, group="g").per == 5


def test_rank_outside_the_world_is_rejected():
    with pytest.raises(ValueError, match="rank"):
        ShardedRound(ADJ[:6], torch.zeros(0, 7), 2, 2, None, None)
    with pytest.raises(ValueError, match="rank"):
        ShardedRound(ADJ[:6], torch.zeros(3, 7), -1, 2, None, None)


def test_wrong_row_count_is_rejected():
    with pytest.raises(ValueError, match="rows"):
        _sharded(5, rows=4)
    with pytest.raises(ValueError, match="rows"):
        _sharded(16, rank=2, world=3, rows=6)  # the last rank owns 4 of its block's 6 rows


def test_sixteen_nodes_over_three_ranks():
    engs = [_sharded(16, rank=r, world=3) for r in range(3)]
    assert [(e.lo, e.hi) for e in engs] == [(0, 6), (6, 12), (12, 16)]
    assert [e.m for e in engs] == [6, 6, 4] and all(e.per == 6 and e.coll for e in engs)


def test_packed_rows_without_a_group():
    eng = _Stub(5)
    assert eng.rows is eng.send and eng.recv is None and eng.row_words == 8
    assert eng.send.shape == (5, 8) and eng.guard.shape == (5,) and eng.send.dtype == torch.int32
    eng.send[:, 2] = torch.tensor([0, 3, 0, 0, 1], dtype=torch.int32)
    eng.send[:, 4] = torch.arange(5, dtype=torch.int32)
    eng.exchange()
    assert torch.equal(eng.guard[:eng.per], eng.send[:, 2])
    assert eng._row(3)[4] == 3
    assert eng._bad_nodes() == []  # the host copy is the engine's to order
    eng._guard_to_host()
    assert eng._bad_nodes() == [1, 4]


def test_count_round_trips_past_31_bits():
    eng = _Stub(5)
    for count in (0, 2 ** 31 + 5, 2 ** 40 + 1):
        eng.send[2, :2] = torch.tensor([count], dtype=torch.int64).view(torch.int32)
        assert eng._count_of(eng._row(2)) == count
    assert eng.send[2, 2] == 0  # the status word is not part of the count


def test_bad_nodes_skip_the_padded_rows_of_the_last_block(monkeypatch):
    import torch.distributed as dist
    eng = _Stub(16, rank=1, world=3)
    assert eng.rows is eng.recv and eng.recv.shape == (18, 8) and eng.send.shape == (6, 8)
    status = np.zeros(18, dtype=np.int32)
    status[[2, 6, 15, 16, 17]] = [1, 5, 1, 9, 9]  # rows 16 and 17 pad the last rank's block
    calls = []

    def all_gather(recv, send, group=None):  # the three ranks' rows, filled by hand
        calls.append((recv is eng.recv, send is eng.send, group))
        recv[:, 2] = torch.from_numpy(status)

    monkeypatch.setattr(dist, "all_gather_into_tensor", all_gather)
    eng.exchange()
    assert calls == [(True, True, None)]
    assert torch.equal(eng.guard, torch.from_numpy(status))
    eng._guard_to_host()
    assert eng._bad_nodes() == [2, 6, 15]
