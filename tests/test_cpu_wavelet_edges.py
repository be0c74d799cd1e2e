"""CPU: the length chooser of the wavelet edge sweep (tests/wavelet_edges.py) picks lengths that
make the sweep worth running, for the built kernels' tile widths and for other widths the
kernels could be built with (DPZ_DWT_TL / DPZ_IDWT_TILE)."""
import pytest

from tests import wavelet_edges as we

GEOMETRIES = [(128, 4096), (64, 2048), (256, 8192), (32, 4096)]


def _check_forward(dwt_tile):
    interior = set()
    for level, k in we.forward_cases():
        ns = we.forward_lengths(level, k, dwt_tile)
        t = dwt_tile << level
        assert ns[0] == k * t - (4 << level) and ns[-1] == k * t + (1 << level)
        assert len(ns) == 5 * (1 << level) + 1 and ns == sorted(set(ns))
        lens = [we.level_lengths(n, level) for n in ns]
        assert all(min(v[:-1]) >= 4 for v in lens), "every level input holds the 4 taps"
        residues = {v[level] % dwt_tile for v in lens}
        assert {0, 1, 2, dwt_tile - 2, dwt_tile - 1} <= residues, (level, k, sorted(residues))
        parities = {tuple(x & 1 for x in v[:level]) for v in lens}
        assert len(parities) == 1 << level, (level, k)
        # the window holds every length of the one-output odd tail
        bad = set(we.predicted_unstaged(level, dwt_tile))
        assert len(bad) == 1 << (level - 1)
        assert bad <= {n % t for n in ns}, (level, k)
        if level == 4:
            interior |= {we.interior_tiles(n, dwt_tile) for n in ns}
            if k < 3:
                assert all(we.interior_tiles(n, dwt_tile) == 0 for n in ns)
    assert {0, 1, 2} <= interior


def _check_inverse(idwt_tile):
    for k in we.INVERSE_K:
        ns = we.inverse_lengths(k, idwt_tile)
        assert ns == list(range(k * idwt_tile - 4, k * idwt_tile + 5))
        tiles = {-(-n // idwt_tile) for n in ns}
        assert tiles == {k, k + 1}, "the window straddles a tile boundary"
        assert {n % idwt_tile for n in ns} >= {idwt_tile - 1, 0, 1}
        assert {n & 1 for n in ns} == {0, 1}


@pytest.mark.parametrize("dwt_tile,idwt_tile", GEOMETRIES)
def test_chooser_covers_the_tile_edges(dwt_tile, idwt_tile):
    _check_forward(dwt_tile)
    _check_inverse(idwt_tile)


def test_chooser_covers_the_built_kernels():
    from decentralizepy_amd import shard
    dwt_tile, idwt_tile = shard.tile_widths()
    _check_forward(dwt_tile)
    _check_inverse(idwt_tile)
    # what the sweep costs: 11, 21, 41 and 81 lengths per case, none past 4 tiles + one output
    for level, k in we.forward_cases():
        assert max(we.forward_lengths(level, k, dwt_tile)) <= 4 * (dwt_tile << level) + (1 << level)


def test_predicted_lengths_at_the_default_width():
    """the residues found by walking the span arithmetic on the CPU, TL = 128"""
    assert we.predicted_unstaged(1, 128) == [255]
    assert we.predicted_unstaged(2, 128) == [507, 508]
    assert we.predicted_unstaged(3, 128) == [1011, 1012, 1013, 1014]
    assert we.predicted_unstaged(4, 128) == list(range(2019, 2027))
