"""Tile plan of the whole-region translator (stain2stain_amd.region.plan_tiles): pure Python, no library, no GPU."""
import math

import pytest
import torch


def _check_axis(origins, L, tile, overlap):
    S = tile - overlap
    if L <= tile:
        assert origins == [0]
        return
    assert len(origins) == math.ceil((L - tile) / S) + 1
    assert origins[0] == 0 and origins[-1] == L - tile                  # last tile flush with the edge
    assert all(0 <= o <= L - tile for o in origins)
    assert all(0 < b - a <= S for a, b in zip(origins, origins[1:]))    # strictly increasing, at most S apart
    # every pixel covered: the tiles start at 0, end at L, and no gap between consecutive tiles (b - a <= S < tile)
    assert origins[-1] + tile == L and all(b - a <= tile for a, b in zip(origins, origins[1:]))


@pytest.mark.parametrize("tile", [16, 64, 256])
def test_axis_sweep(tile):
    from stain2stain_amd.region import plan_tiles
    for overlap in range(tile):
        for L in range(1, 701):
            p = plan_tiles(L, 1, tile, overlap)
            assert p.dtype == torch.int32 and p.dim() == 2 and p.shape[1] == 2
            assert p[:, 1].eq(0).all()
            _check_axis(p[:, 0].tolist(), L, tile, overlap)


@pytest.mark.parametrize("H,W,tile,overlap", [(700, 333, 64, 16), (1, 700, 16, 3), (256, 257, 256, 32),
                                               (511, 96, 64, 0), (5, 5, 16, 15)])
def test_two_axes_row_major(H, W, tile, overlap):
    from stain2stain_amd.region import plan_tiles
    p = plan_tiles(H, W, tile, overlap)
    ys = plan_tiles(H, 1, tile, overlap)[:, 0].tolist()
    xs = plan_tiles(W, 1, tile, overlap)[:, 0].tolist()
    assert p.tolist() == [[y, x] for y in ys for x in xs]                 # all tiles of one tile row, then the next
    cov = torch.zeros(H, W, dtype=torch.bool)
    for y, x in p.tolist():
        cov[y:y + tile, x:x + tile] = True
    assert cov.all()


@pytest.mark.parametrize("args", [(10, 10, 0, 0), (10, 10, -4, 0), (10, 10, 16, -1), (10, 10, 16, 16),
                                  (10, 10, 16, 20), (0, 10, 16, 4), (10, 0, 16, 4), (-3, 10, 16, 4)])
def test_invalid_arguments(args):
    from stain2stain_amd.region import plan_tiles
    with pytest.raises(ValueError):
        plan_tiles(*args)


def test_band_rows_do_not_depend_on_height():
    from stain2stain_amd.region import band_rows_for
    for W, tile, overlap, batch in ((150, 64, 16, 5), (4096, 256, 32, 32), (300, 16, 4, 1)):
        rows = {band_rows_for(H, W, tile, overlap, batch) for H in (2000, 5000, 20000)}
        assert len(rows) == 1 and rows.pop() < 2000
