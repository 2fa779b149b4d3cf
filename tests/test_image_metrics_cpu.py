"""Image-quality metrics without a GPU: the fp64 restatement (tests/image_quality_ref.py) against closed forms, the
region band planner, and the argument checks the wrappers make before they touch the device."""
import math

import pytest
import torch

import image_quality_ref as R


def _rand(shape, seed, lo=0.0, hi=255.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo


# ---- the reference against closed forms ------------------------------------------------------------------------------
def test_identical_images():
    a = _rand((2, 3, 40, 33), 0).round()
    q = R.image_quality_ref(a, a.clone(), 255.0)
    assert torch.equal(q["ssim"], torch.ones(2, dtype=torch.float64))
    assert torch.equal(q["mse"], torch.zeros(2, dtype=torch.float64)) and torch.equal(q["mae"], q["mse"])
    assert torch.isinf(q["psnr"]).all() and (q["psnr"] > 0).all()


@pytest.mark.parametrize("va,vb,L", [(200.0, 190.0, 255.0), (10.0, 250.0, 255.0), (0.75, 0.25, 1.0), (0.0, 1.0, 1.0)])
def test_constant_images(va, vb, L):
    a, b = torch.full((1, 2, 30, 25), va, dtype=torch.float64), torch.full((1, 2, 30, 25), vb, dtype=torch.float64)
    q = R.image_quality_ref(a, b, L)
    c1 = (0.01 * L) ** 2
    assert abs(float(q["ssim"]) - (2 * va * vb + c1) / (va * va + vb * vb + c1)) < 1e-12
    assert abs(float(q["psnr"]) - 20.0 * math.log10(L / abs(va - vb))) < 1e-10
    assert abs(float(q["mse"]) - (va - vb) ** 2) < 1e-12 * max(1.0, (va - vb) ** 2)
    assert abs(float(q["mae"]) - abs(va - vb)) < 1e-12 * max(1.0, abs(va - vb))


def test_ssim_is_scale_invariant():
    a, b = _rand((2, 3, 50, 41), 1).round(), _rand((2, 3, 50, 41), 2).round()
    b = (0.7 * a + 0.3 * b).round()
    q255, q1 = R.image_quality_ref(a, b, 255.0), R.image_quality_ref(a / 255.0, b / 255.0, 1.0)
    assert (q255["ssim"] - q1["ssim"]).abs().max() < 1e-12
    assert (q255["psnr"] - q1["psnr"]).abs().max() < 1e-10


@pytest.mark.parametrize("C,H,W", [(1, 11, 11), (3, 37, 53), (4, 96, 80)])
def test_valid_position_count(C, H, W):
    a = _rand((1, C, H, W), 3)
    m = R.ssim_map(a, a, 255.0)
    assert m.numel() == (H - 10) * (W - 10) * C == R.valid_positions(C, H, W)


def test_window_is_normalised_and_symmetric():
    g = R.gaussian_window()
    assert abs(float(g.sum()) - 1.0) < 1e-15 and torch.equal(g, g.flip(0)) and g.argmax() == 5
    from stain2stain_amd.image_metrics import gaussian_taps
    assert (torch.tensor(gaussian_taps(11, 1.5), dtype=torch.float64) - g).abs().max() < 1e-15
    assert (torch.tensor(gaussian_taps(7, 1.0), dtype=torch.float64) - R.gaussian_window(7, 1.0)).abs().max() < 1e-15


def test_quantised_conversion_is_the_save_conversion():
    x = torch.tensor([-1.5, -1.0, -0.999, 0.0, 0.003, 0.5, 0.999, 1.0, 2.0])
    img, L = R.network_to_image(x, True)
    want = ((x * 0.5 + 0.5) * 255).clamp(0, 255).to(torch.uint8).double()
    assert L == 255.0 and torch.equal(img, want)
    img, L = R.network_to_image(x, False)
    assert L == 1.0 and float(img.min()) == 0.0 and float(img.max()) == 1.0


# ---- the band planner ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [11, 12, 42, 43, 74, 75, 300, 330, 1034, 2049])
@pytest.mark.parametrize("band_rows", [None, 42, 43, 74, 138, 1000])
@pytest.mark.parametrize("window", [11, 7])
def test_plan_bands_covers_every_valid_row_once(H, band_rows, window):
    from stain2stain_amd.image_metrics import BLOCK_ROWS, plan_bands
    if band_rows is not None and band_rows < BLOCK_ROWS + window - 1:
        with pytest.raises(ValueError):
            plan_bands(H, window, band_rows)
        return
    bands = plan_bands(H, window, band_rows)
    valid = H - window + 1
    seen = [0] * valid
    next_block = 0
    for by0, nby, r0, r1 in bands:
        assert by0 == next_block and nby >= 1                      # whole, consecutive blocks
        next_block = by0 + nby
        v0, v1 = by0 * BLOCK_ROWS, min(valid, (by0 + nby) * BLOCK_ROWS)
        assert r0 == v0 and r1 == v1 + window - 1 and 0 <= r0 < r1 <= H   # the rows the band's windows touch
        if band_rows is not None:
            assert r1 - r0 <= band_rows
        for v in range(v0, v1):
            seen[v] += 1
    assert seen == [1] * valid
    assert next_block == -(-valid // BLOCK_ROWS)
    if band_rows is None:
        assert len(bands) == 1


def test_plan_bands_rejects():
    from stain2stain_amd.image_metrics import plan_bands
    with pytest.raises(ValueError):
        plan_bands(10)
    with pytest.raises(ValueError):
        plan_bands(100, 11, 41)
    with pytest.raises(ValueError):
        plan_bands(100, 10)
    with pytest.raises(ValueError):
        plan_bands(100, 13)


# ---- argument checks that need no GPU --------------------------------------------------------------------------------
def test_image_quality_rejects():
    from stain2stain_amd import image_quality
    a = torch.zeros((2, 3, 32, 32))
    with pytest.raises(RuntimeError, match="GPU"):
        image_quality(a, a.clone())                                  # CPU tensors: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        image_quality(torch.zeros((2, 32, 32, 3), dtype=torch.uint8), torch.zeros((2, 32, 32, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        image_quality(a, torch.zeros((2, 3, 32, 31)))
    with pytest.raises(ValueError):
        image_quality(a, a.to(torch.uint8))
    with pytest.raises(ValueError):
        image_quality(torch.zeros((2, 3, 10, 32)), torch.zeros((2, 3, 10, 32)))      # H below the window
    with pytest.raises(ValueError):
        image_quality(torch.zeros((2, 3, 32, 8)), torch.zeros((2, 3, 32, 8)), window=9)
    with pytest.raises(ValueError):
        image_quality(torch.zeros((2, 5, 32, 32)), torch.zeros((2, 5, 32, 32)))      # C > 4
    with pytest.raises(ValueError):
        image_quality(a, a.clone(), window=10)
    with pytest.raises(ValueError):
        image_quality(a, a.clone(), window=13)
    with pytest.raises(ValueError):
        image_quality(a, a.clone(), sigma=0.0)
    with pytest.raises(ValueError):
        image_quality(a.double(), a.double())
    with pytest.raises(ValueError):
        image_quality(torch.zeros((2, 32, 32, 4), dtype=torch.uint8), torch.zeros((2, 32, 32, 4), dtype=torch.uint8))
    with pytest.raises(TypeError):
        image_quality(a.numpy(), a)


def test_region_quality_rejects():
    from stain2stain_amd import region_quality
    u = torch.zeros((40, 40, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        region_quality(u.float(), u.float())
    with pytest.raises(ValueError):
        region_quality(u, u[:39])
    with pytest.raises(ValueError):
        region_quality(u[..., :2], u[..., :2])
    with pytest.raises(ValueError):
        region_quality(u[:10], u[:10])
    with pytest.raises(ValueError):
        region_quality(u, u.clone(), band_rows=20)
    with pytest.raises(ValueError):
        region_quality(u[:, ::2], u[:, ::2])                         # pixels not contiguous within a row
    with pytest.raises(TypeError):
        region_quality(u, None)


def test_generation_quality_rejects_a_non_tensor_sampler():
    from stain2stain_amd import generation_quality
    a = torch.zeros((1, 3, 16, 16))
    with pytest.raises(TypeError):
        generation_quality(lambda x: [x], a, a)
