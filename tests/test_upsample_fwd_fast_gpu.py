"""The register-window up-sampling forward (resample.hip, upsample2x_fwd_win_kernel) against the row-sweep kernel it
replaced (``ops.upsample2x_fwd(..., _reference=True)``): bit for bit, on NaN-poisoned outputs.

Shapes: maps of 1x1 (both entry points keep the row sweep), 2x3 (the smallest the new kernel takes: every row pair is a
first or last one), 4x4, 5x7, 16x16 and 33x18 source pixels (odd sizes, more source columns than a workgroup's slots at
C = 264, several bands); outputs of exactly twice the input and padded by 1 and 3 rows / columns (and unevenly, 1 x 3);
C = 8, 24, 64 and 264 (below, inside and above the 32-piece lane group, so C = 264 takes two channel groups); with and
without the per-(sample, channel) bias; B = 1 and 3; input and output dense, and input as a channel slice of a wider
tensor with the output as a channel slice of a concat buffer whose other channels hold a sentinel that must survive.
tests/test_upsample_fwd_window_cpu.py holds the window the kernel rests on and the host's choice of kernel; the
row-sweep kernel's own accuracy is held by the step-wise suite."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIZES = [(1, 1), (2, 3), (4, 4), (5, 7), (16, 16), (33, 18)]
CHANNELS = [8, 24, 64, 264]
PADS = [(0, 0), (1, 1), (3, 3), (1, 3)]
SENTINEL = 7.0


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


@functools.lru_cache(maxsize=None)
def inputs(hin, win, C):
    """(x [3, hin, win, C], bias [3, C]) in fp32 holding bf16-exact values; B = 1 takes the first sample."""
    g = torch.Generator().manual_seed(100000 * hin + 1000 * win + C)
    x = (torch.rand(3, hin, win, C, generator=g) - 0.5).bfloat16().float()
    x[0, 0, 0, :4] = 0.0                                   # exact zeros of both signs among the taps
    x[0, -1, -1, :4] = -0.0
    bias = (torch.rand(3, C, generator=g) - 0.5).bfloat16().float()
    return x, bias


def run_both(x, out_shape, bias, sliced, dtype):
    """The two kernels' outputs for one case; ``sliced``: strided input, output inside a concat buffer."""
    from stain2stain_amd import ops
    B, hin, win, C = x.shape
    small = hin < 2 or win < 2
    outs = []
    for reference in (False, True):
        if sliced:
            wide = torch.full((B, hin, win, C + 16), float("nan"), device=DEV, dtype=dtype)
            wide[..., 8:8 + C] = x
            xin = wide[..., 8:8 + C]
            cat = torch.full((*out_shape[:3], C + 24), SENTINEL, device=DEV, dtype=dtype)
            cat[..., 16:16 + C] = float("nan")
            out = cat[..., 16:16 + C]
        else:
            xin = x
            out = torch.empty(out_shape, device=DEV, dtype=dtype)
            assert out.isnan().all()                       # outputs start out as NaN
        # the two calls really run different kernels (s2s_upsample2x_fwd_family: 0 row sweep, 1 register window)
        assert ops.upsample2x_fwd_family(xin, out, _reference=reference) == (0 if small or reference else 1)
        ops.upsample2x_fwd(xin, out, bias, _reference=reference)
        torch.cuda.synchronize()
        if sliced:
            assert bool((cat[..., :16] == SENTINEL).all()) and bool((cat[..., 16 + C:] == SENTINEL).all())
            assert bool(wide[..., :8].isnan().all()) and bool(wide[..., 8 + C:].isnan().all())
            assert torch.equal(wide[..., 8:8 + C], x)
        outs.append(out.clone())
    return outs


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_forward_matches_row_sweep_kernel(size, C, dtype):
    hin, win = size
    x_all, bias_all = inputs(hin, win, C)
    for B in (1, 3):
        x = x_all[:B].to(DEV, dtype).contiguous()
        for with_bias in (False, True):
            bias = bias_all[:B].to(DEV).contiguous() if with_bias else None
            for ph, pw in PADS:
                shape = (B, 2 * hin + ph, 2 * win + pw, C)
                for sliced in (False, True):
                    what = f"{hin}x{win} C{C} B{B} bias{int(with_bias)} pad{ph}x{pw} sliced{int(sliced)}"
                    new, old = run_both(x, shape, bias, sliced, dtype)
                    assert bool(torch.isfinite(new.float()).all()), what
                    assert torch.equal(new, old), f"{what}: differs in {int((new != old).sum())} elements"
                    # -0.0 == 0.0 under torch.equal: the signs of zeros must agree too
                    assert torch.equal(torch.signbit(new), torch.signbit(old)), what
                    # the pad is zero, the image is not all zero
                    t, l = ph // 2, pw // 2
                    assert bool(new[:, t:t + 2 * hin, l:l + 2 * win].any()), what
                    new[:, t:t + 2 * hin, l:l + 2 * win] = 0
                    assert not bool(new.any()), what
