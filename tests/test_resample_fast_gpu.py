"""The 2 x 2 up-sampling backward (resample.hip, upsample2x_bwd_quad_kernel) against the per-pixel window kernel it
replaced (``ops.upsample2x_bwd(..., _reference=True)``): bit for bit, on NaN-poisoned buffers, and both within the
step-wise suite's tolerances of the fp64 reference (tests/stepwise_ref.py; 4e-3 max / 2.2e-3 L2 for bf16 storage, 1e-4
for fp32, as tests/test_stepwise_bf16_gpu.py uses them).

Shapes: maps of 4x4, 5x7, 8x4, 16x16 and 33x17 source pixels (the smallest the kernel takes, odd sizes whose last pixel
pair is moved back by one, more pixel pairs than thread slots), C/8 below, at and above the 32-piece lane group (C = 8,
24, 128, 1024: at 1024 a row pair is split over four workgroups), an output of exactly twice the input and one padded
unevenly (2H+1 x 2W+3), dy dense and as the upper channel slice of a concat buffer whose lower channels are NaN.  The
forward kernel is unchanged, so there is no forward case here; tests/test_resample_window_cpu.py holds the window
placement the kernel rests on and the host's choice of kernel."""
import functools

import pytest
import torch

import stepwise_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_BF, L2_BF, TOL_F32 = 4e-3, 2.2e-3, 1e-4

SIZES = [(4, 4), (5, 7), (8, 4), (16, 16), (33, 17)]
CHANNELS = [8, 24, 128, 1024]
B = 2


@pytest.fixture(autouse=True)
def poison():
    import torch.utils.deterministic as tud
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
            tud.fill_uninitialized_memory)
    torch.use_deterministic_algorithms(True, warn_only=True)
    tud.fill_uninitialized_memory = True
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
        tud.fill_uninitialized_memory = prev[2]


def out_size(hin, win, padded):
    return (2 * hin + 1, 2 * win + 3) if padded else (2 * hin, 2 * win)


@functools.lru_cache(maxsize=None)
def case(hin, win, C, padded):
    """(dy [B, Ho, Wo, C] fp32 holding bf16-exact values, fp64 dx): one reference per shape, shared by both dtypes."""
    Ho, Wo = out_size(hin, win, padded)
    g = torch.Generator().manual_seed(1000 * hin + 10 * win + C + int(padded))
    dy = R.bf(torch.rand(B, Ho, Wo, C, generator=g) - 0.5)
    pt, pl = (Ho - 2 * hin) // 2, (Wo - 2 * win) // 2
    ref = R.upsample2x_bwd(dy[:, pt:pt + 2 * hin, pl:pl + 2 * win], hin, win)     # the pad's gradient goes nowhere
    return dy, ref


def run_both(dy_dev, hin, win):
    from stain2stain_amd import ops
    assert torch.empty(64, device=DEV, dtype=dy_dev.dtype).isnan().all()          # outputs start out as NaN
    # the two calls really run different kernels (s2s_upsample2x_bwd_family: 0 gather, 1 window, 2 the 2 x 2 kernel)
    small = hin <= 3 or win <= 3
    assert ops.upsample2x_bwd_family(dy_dev, hin, win) == (0 if small else 2)
    assert ops.upsample2x_bwd_family(dy_dev, hin, win, _reference=True) == (0 if small else 1)
    new = ops.upsample2x_bwd(dy_dev, hin, win)
    old = ops.upsample2x_bwd(dy_dev, hin, win, _reference=True)
    torch.cuda.synchronize()
    return new, old


def check(new, old, ref, dtype, what):
    assert bool(torch.isfinite(new.float()).all()), what
    assert torch.equal(new, old), f"{what}: differs from the window kernel in {int((new != old).sum())} elements"
    rm, rl = R.rel_max(new, ref), R.rel_l2(new, ref)
    print(f"{what}: rel max {rm:.3e} rel L2 {rl:.3e}")
    if dtype == torch.bfloat16:
        assert rm <= TOL_BF and rl <= L2_BF, what
    else:
        assert rm <= TOL_F32 and rl <= TOL_F32, what


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_backward_matches_window_kernel(size, C, dtype):
    hin, win = size
    for padded in (False, True):
        dy, ref = case(hin, win, C, padded)
        Ho, Wo = out_size(hin, win, padded)
        # dense
        new, old = run_both(dy.to(DEV, dtype), hin, win)
        check(new, old, ref, dtype, f"{hin}x{win} C{C} pad{int(padded)} dense")
        # upper channel slice of a concat buffer; the skip's channels below it are NaN and stay NaN
        cs = 16
        cat = torch.full((B, Ho, Wo, cs + C), float("nan"), device=DEV, dtype=dtype)
        cat[..., cs:] = dy.to(DEV, dtype)
        new, old = run_both(cat[..., cs:], hin, win)
        check(new, old, ref, dtype, f"{hin}x{win} C{C} pad{int(padded)} slice")
        assert bool(cat[..., :cs].isnan().all())
        assert torch.equal(cat[..., cs:], dy.to(DEV, dtype))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_three_pixel_maps_keep_the_branching_gather(dtype):
    """Hin = 3 or Win = 3: both entry points run the branching gather, as before."""
    for hin, win in ((3, 5), (6, 3)):
        dy, ref = case(hin, win, 24, True)
        new, old = run_both(dy.to(DEV, dtype), hin, win)
        check(new, old, ref, dtype, f"{hin}x{win}")

