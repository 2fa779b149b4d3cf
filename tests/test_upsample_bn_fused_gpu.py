"""BatchNorm + ReLU applied in the up-sampling's loads (resample.hip, the affine form of upsample2x_fwd_win_kernel;
``ops.upsample2x_fwd(raw, out, bias, bn_relu=(scale, shift))``) against the chain it replaces, ``ops.bn_relu_apply``
followed by ``ops.upsample2x_fwd``: bit for bit, signs of zeros included.

Outputs start NaN-filled and are a channel slice of a wider buffer (``ldy > C``) whose other channels hold a sentinel that
must survive.  Source maps: 2x2 (every row pair is a first or last one), 3x5 into an odd output padded by 1 x 3, 4x4, 9x7,
17x33 (five bands of four source rows, the last one ragged) and 1x4, which the row-sweep kernel takes: there the wrapper
runs the chain into a scratch tensor.  C = 8, 24, 64 and 264 (264 channels are 33 channel pieces, one more than a channel
group holds, so the launch has two channel groups); with and without the time bias; bf16 and fp32; the raw input is
centred on zero, so the ReLU cuts about half of it, and ``scale`` has entries of both signs; 9x7 also runs with the input
as a channel slice (``ldx > C``).  The trainers' switch is held by tests/test_lazy_up_trainers_gpu.py."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (hin, win, pad rows, pad columns)
MAPS = [(2, 2, 0, 0), (3, 5, 1, 3), (4, 4, 0, 0), (9, 7, 2, 2), (17, 33, 0, 1), (1, 4, 0, 0)]
CHANNELS = [8, 24, 64, 264]
SENTINEL = 7.0
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


@functools.lru_cache(maxsize=None)
def inputs(hin, win, C):
    """(raw [B, hin, win, C], scale [C], shift [C], bias [B, C]) in fp32; raw and bias hold bf16-exact values."""
    g = torch.Generator().manual_seed(100000 * hin + 1000 * win + C)
    raw = (torch.rand(B, hin, win, C, generator=g) - 0.5).bfloat16().float()
    raw[0, 0, 0, :4] = 0.0                                 # exact zeros of both signs among the taps
    raw[0, -1, -1, :4] = -0.0
    scale = (torch.rand(C, generator=g) - 0.5) * 4.0       # both signs
    shift = (torch.rand(C, generator=g) - 0.5) * 0.2
    bias = (torch.rand(B, C, generator=g) - 0.5).bfloat16().float()
    return raw, scale, shift, bias


def out_slice(shape, C, dtype):
    cat = torch.full((*shape, C + 24), SENTINEL, device=DEV, dtype=dtype)
    cat[..., 16:16 + C] = float("nan")
    return cat, cat[..., 16:16 + C]


def check_case(hin, win, ph, pw, C, dtype, with_bias, sliced_in):
    from stain2stain_amd import ops
    raw_c, scale_c, shift_c, bias_c = inputs(hin, win, C)
    scale, shift = scale_c.to(DEV), shift_c.to(DEV)
    bias = bias_c.to(DEV) if with_bias else None
    if sliced_in:
        wide = torch.full((B, hin, win, C + 16), float("nan"), device=DEV, dtype=dtype)
        wide[..., 8:8 + C] = raw_c.to(DEV, dtype)
        raw = wide[..., 8:8 + C]
    else:
        raw = raw_c.to(DEV, dtype).contiguous()
    shape = (B, 2 * hin + ph, 2 * win + pw)
    what = f"{hin}x{win} pad{ph}x{pw} C{C} {dtype} bias{int(with_bias)} sliced{int(sliced_in)}"

    act, _ = ops.bn_relu_apply(raw, scale, shift)
    frac = float((act == 0).float().mean())
    assert 0.25 < frac < 0.75, (what, frac)                # the ReLU cuts about half
    cat_ref, ref = out_slice(shape, C, dtype)
    ops.upsample2x_fwd(act, ref, bias)

    cat_new, new = out_slice(shape, C, dtype)
    assert bool(new.isnan().all())
    # the fused call runs the window kernel wherever the plain one does; a one-pixel axis keeps the row sweep
    assert ops.upsample2x_fwd_family(raw, new) == (0 if hin < 2 or win < 2 else 1), what
    ops.upsample2x_fwd(raw, new, bias, bn_relu=(scale, shift))
    torch.cuda.synchronize()

    assert bool(torch.isfinite(new.float()).all()), what
    assert torch.equal(new, ref), f"{what}: differs in {int((new != ref).sum())} elements"
    assert torch.equal(torch.signbit(new), torch.signbit(ref)), what
    assert bool((cat_new[..., :16] == SENTINEL).all()) and bool((cat_new[..., 16 + C:] == SENTINEL).all()), what
    if sliced_in:                                          # the input and what surrounds it are untouched
        assert bool(wide[..., :8].isnan().all()) and bool(wide[..., 8 + C:].isnan().all()), what
        assert torch.equal(wide[..., 8:8 + C], raw_c.to(DEV, dtype)), what
    # the pad is zero (the affine of a zero would not be), the image is not
    t, l = ph // 2, pw // 2
    img = new.clone()
    assert bool(img[:, t:t + 2 * hin, l:l + 2 * win].any()), what
    img[:, t:t + 2 * hin, l:l + 2 * win] = 0
    assert not bool(img.any()), what


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("m", MAPS, ids=[f"{m[0]}x{m[1]}" for m in MAPS])
def test_fused_bn_relu_upsampling_equals_the_chain(m, C, dtype):
    hin, win, ph, pw = m
    for with_bias in (False, True):
        check_case(hin, win, ph, pw, C, dtype, with_bias, sliced_in=False)
    if (hin, win) == (9, 7):
        check_case(hin, win, ph, pw, C, dtype, True, sliced_in=True)
        check_case(hin, win, ph, pw, C, dtype, False, sliced_in=True)


def test_mismatched_scale_is_refused():
    from stain2stain_amd import ops
    raw = torch.zeros(1, 4, 4, 16, device=DEV, dtype=torch.bfloat16)
    out = torch.empty(1, 8, 8, 16, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="scale / shift"):
        ops.upsample2x_fwd(raw, out, None, bn_relu=(torch.ones(8, device=DEV), torch.zeros(8, device=DEV)))
