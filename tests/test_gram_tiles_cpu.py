"""The one-product Gram pass's tile table (csrc/kernels/gram_tile_order.hpp, bound as _C.gram_tile_order): 256 x 256
tiles, entry (tx << 16) | u = the pair of 256 x 128 tiles (tx, 2 u) and (tx, 2 u + 1), for a Gram of tm 256-row
tiles by tn 128-column tiles.  Walked on the host: the halves of the symmetric table are exactly the 256 x 128
tiles with ty >= 2 tx (the tiles the hot-tile pass and gram_adapt_last count), the non-symmetric table covers every
tile once, and every coordinate fits the entry's 16 bits.
Reference: the kernel rows the Gram replaces, svmTrain.cu:212-249 (cuBLAS Sgemv + exp).
"""
import pytest

from dpsvm_amd._native import load

# (tm, tn): tn odd (a last tile with a left half only), tm = 1, one tile, the headline's 235 x 469, tables longer
# and shorter than a round of XCD chunks
SHAPES = [(1, 1), (1, 2), (1, 3), (2, 3), (2, 4), (3, 5), (3, 6), (5, 9), (9, 17), (28, 55), (40, 80), (235, 469)]


def _halves(table, tn):
    out = []
    for e in table:
        tx, u = e >> 16, e & 0xFFFF
        assert 0 <= e < 1 << 32
        for h in (0, 1):
            if 2 * u + h < tn:
                out.append((tx, 2 * u + h))
        assert 2 * u < tn  # no tile without a left half
    return out


@pytest.mark.parametrize("tm,tn", SHAPES)
def test_symmetric_halves_are_the_upper_tiles(tm, tn):
    C = load()
    table = C.gram_tile_order(tm, tn, True)
    halves = _halves(table, tn)
    want = {(tx, ty) for tx in range(tm) for ty in range(tn) if ty >= 2 * tx}
    assert len(halves) == len(set(halves))  # each once
    assert set(halves) == want  # and nothing else
    assert len(table) == len(set(table))
    assert all((e >> 16) < tm and (e >> 16) < 1 << 16 and (e & 0xFFFF) < (tn + 1) // 2 for e in table)


@pytest.mark.parametrize("tm,tn", SHAPES + [(3, 1), (6, 2), (11, 5)])
def test_rectangular_covers_every_tile_once(tm, tn):
    C = load()
    table = C.gram_tile_order(tm, tn, False)
    halves = _halves(table, tn)
    assert len(halves) == len(set(halves)) == tm * tn
    assert set(halves) == {(tx, ty) for tx in range(tm) for ty in range(tn)}
    assert len(table) == tm * ((tn + 1) // 2)


def test_headline_counts():
    C = load()
    table = C.gram_tile_order(235, 469, True)
    assert len(table) == 235 * 236 // 2
    assert len(_halves(table, 469)) == 55225  # gram_tiles of the 60000-row headline
