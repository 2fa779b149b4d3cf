"""plan_region_batches (stain2stain_amd.region): the host-only rule that cuts a tile plan into ranges of at most
``batch`` kept tiles that fit the accumulator ring.  No GPU."""
import pytest
import torch

from stain2stain_amd.region import band_rows_for, plan_region_batches, plan_tiles

PLANS = [(150, 130, 32, 8, 4), (400, 70, 32, 0, 5), (20, 130, 32, 8, 4), (300, 300, 64, 16, 7)]


def _setup(H, W, T, ov, batch):
    return plan_tiles(H, W, T, ov), band_rows_for(H, W, T, ov, batch)


def _fits(tops, kept, p0, p1, batch, band_rows, T):
    """The two bounds of a range [p0, p1); tiles of the first tile's own row span the same rows and always fit."""
    return sum(kept[p0:p1]) <= batch and (tops[p1 - 1] == tops[p0] or tops[p1 - 1] + T - tops[p0] <= band_rows)


@pytest.mark.parametrize("H,W,T,ov,batch", PLANS)
@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_ranges_partition_respect_the_bounds_and_are_maximal(H, W, T, ov, batch, density):
    plan, band_rows = _setup(H, W, T, ov, batch)
    N = plan.shape[0]
    tops = plan[:, 0].tolist()
    g = torch.Generator().manual_seed(int(density * 10) + H)
    for _ in range(5):
        keep = torch.rand(N, generator=g) < density
        kept = keep.tolist()
        ranges = plan_region_batches(plan, keep, batch, band_rows, T)
        assert ranges[0][0] == 0 and ranges[-1][1] == N
        assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        for p0, p1 in ranges:
            assert p1 > p0
            assert _fits(tops, kept, p0, p1, batch, band_rows, T)
            assert min(H, tops[p1 - 1] + T) - tops[p0] <= band_rows          # the rows it touches fit the ring
            assert p1 == N or not _fits(tops, kept, p0, p1 + 1, batch, band_rows, T)


@pytest.mark.parametrize("H,W,T,ov,batch", PLANS)
def test_all_true_gives_the_fixed_slices(H, W, T, ov, batch):
    plan, band_rows = _setup(H, W, T, ov, batch)
    N = plan.shape[0]
    ranges = plan_region_batches(plan, torch.ones(N, dtype=torch.bool), batch, band_rows, T)
    assert ranges == [(p0, min(N, p0 + batch)) for p0 in range(0, N, batch)]


@pytest.mark.parametrize("H,W,T,ov,batch", PLANS)
def test_all_false_gives_ranges_without_kept_tiles(H, W, T, ov, batch):
    plan, band_rows = _setup(H, W, T, ov, batch)
    N = plan.shape[0]
    tops = plan[:, 0].tolist()
    ranges = plan_region_batches(plan, torch.zeros(N, dtype=torch.bool), batch, band_rows, T)
    assert ranges[0][0] == 0 and ranges[-1][1] == N and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    for p0, p1 in ranges:                                    # only the row bound cuts: whole tile rows
        assert min(H, tops[p1 - 1] + T) - tops[p0] <= band_rows
        assert p1 == N or tops[p1] + T - tops[p0] > band_rows


def test_one_kept_tile_per_range_when_batch_is_one():
    plan, band_rows = _setup(150, 130, 32, 8, 1)
    N = plan.shape[0]
    keep = torch.zeros(N, dtype=torch.bool)
    keep[[3, 4, 20]] = True
    ranges = plan_region_batches(plan, keep, 1, band_rows, 32)
    assert all(int(keep[p0:p1].sum()) <= 1 for p0, p1 in ranges)
    assert sum(int(keep[p0:p1].sum()) for p0, p1 in ranges) == 3


def test_rejections():
    plan, band_rows = _setup(150, 130, 32, 8, 4)
    N = plan.shape[0]
    ok = torch.ones(N, dtype=torch.bool)
    with pytest.raises(ValueError):
        plan_region_batches(plan, torch.ones(N + 1, dtype=torch.bool), 4, band_rows, 32)
    with pytest.raises(ValueError):
        plan_region_batches(plan, torch.ones((N, 1), dtype=torch.bool), 4, band_rows, 32)
    with pytest.raises(ValueError):
        plan_region_batches(plan, torch.ones(N, dtype=torch.uint8), 4, band_rows, 32)
    with pytest.raises(ValueError):
        plan_region_batches(plan, torch.ones(N), 4, band_rows, 32)
    with pytest.raises(TypeError):
        plan_region_batches(plan, [True] * N, 4, band_rows, 32)
    with pytest.raises(ValueError):
        plan_region_batches(plan, ok, 0, band_rows, 32)
    with pytest.raises(ValueError):
        plan_region_batches(plan, ok, 4, 0, 32)


def test_exported_from_the_package():
    import stain2stain_amd
    assert stain2stain_amd.plan_region_batches is plan_region_batches
    assert "tissue_counts" in stain2stain_amd.__all__ and "plan_region_batches" in stain2stain_amd.__all__
