"""Lengths at which the fused wavelet kernels' tiling can go wrong, derived from the built kernels'
geometry (``shard.tile_widths()``: the forward tile of DWT_TL level-L outputs, the inverse tile
of IDWT_TILE outputs) instead of from literals.  No GPU, no device code: plain index arithmetic
shared by tests/test_cpu_wavelet_edges.py and tests/test_gpu_wavelet_edges.py.

Forward: a tile owns DWT_TL level-L outputs, i.e. T = DWT_TL * 2^L inputs, so the windows
[k T - 4 * 2^L, k T + 2^L] walk the last tile through "nearly full", "full", "one output",
"two outputs" with every parity pattern of the level lengths below it (the odd-length levels
take pywt's right-overhang order).  Inverse: the windows [k V - 4, k V + 4] around the
multiples of V = IDWT_TILE.
"""

FILTER_LEN = {"sym2": 4, "haar": 2}
FORWARD_LEVELS = (1, 2, 3, 4)
INVERSE_K = (1, 2, 3)


def level_lengths(n, level, wavelet="sym2"):
    """[len_0 = n, ..., len_L]: len_l = (len_{l-1} + F - 1) // 2 (sym2: + 3, haar: + 1)."""
    f = FILTER_LEN[wavelet]
    lens = [int(n)]
    for _ in range(level):
        lens.append((lens[-1] + f - 1) // 2)
    return lens


def forward_ks(level):
    """k = 3 at level 4 only: the first lengths with an interior tile."""
    return (1, 2, 3, 4) if level == 4 else (1, 2, 4)


def forward_cases(levels=FORWARD_LEVELS):
    return [(lv, k) for lv in levels for k in forward_ks(lv)]


def forward_lengths(level, k, dwt_tile):
    t = dwt_tile << level
    return list(range(k * t - (4 << level), k * t + (1 << level) + 1))


def inverse_lengths(k, idwt_tile):
    return list(range(k * idwt_tile - 4, k * idwt_tile + 5))


def forward_tiles(n, level, dwt_tile, wavelet="sym2"):
    return -(-level_lengths(n, level, wavelet)[level] // dwt_tile)


def interior_tiles(n, dwt_tile):
    """Level-4 sym2 tiles on the interior (register) path of an unsharded launch: tiles
    1 <= t with (t + 2) * 16 * DWT_TL <= n; every other tile runs the edge (span) path."""
    nt = forward_tiles(n, 4, dwt_tile)
    hi = min(n // (16 * dwt_tile) - 1, nt)
    return max(0, hi - 1)


def predicted_unstaged(level, dwt_tile):
    """Residues n mod DWT_TL * 2^L at which, before the one-output tail tile was widened
    (DESIGN.md §3.4), the last tile owned one level-L output of an odd-length level-(L-1) input
    and its odd-tail convolution read extension slots that were never written."""
    t = dwt_tile << level
    out = []
    for n in range(2 * t, 3 * t):
        lens = level_lengths(n, level)
        if lens[level] % dwt_tile == 1 and lens[level - 1] % 2 == 1:
            out.append(n % t)
    return sorted(out)
