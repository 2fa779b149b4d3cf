"""The bf16-only convolution kernels of the pix2pix step at kernel level, every launch plan, against fp64 references on
the bf16-rounded operands (tests/p2p_forms_ref.py):

  * s2s_conv4x4s2_nhwc / s2s_convt4x4s2_nhwc: one shape per value 0..6 of s2s_conv4x4s2_plan / s2s_convt4x4s2_plan (the six
    tile plans and the flat form) plus non-flat split-K, with bias, activation and second output (forward) or into a
    channel slice (transposed); bf16 outputs to 4e-3 (one bf16 rounding is 2^-9);
  * ops.convkxk_wgrad in bf16: the DMA kernel from the plain tensor and from the space-to-depth image with splits that own
    an uneven number of pixel tiles (double buffering across tiles), the flat, small and rows kernels, both fold kernels,
    the tap-major layout, accumulate once per kernel; the outputs are fp32, so the bound is the 1e-4 that
    test_conv4x4_gpu.py holds the older entry points to;
  * ops.convsm_fwd (conv_small.hip), both modes: the kernel rounds the bias-added accumulators to bf16 BEFORE it takes the
    statistics (conv_small.hip: "the statistics are those of the values as stored"), so y / y2 / stats are compared with
    the fp64 InstanceNorm of the kernel's own stored ``raw`` (teacher forcing, as test_stepwise_bf16_gpu.py does), and
    ``raw`` with the fp64 convolution, all to 4e-3; mean and 1/std to the 1e-5 of test_instnorm_forms_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

import p2p_forms_ref as R
from conftest import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
TOL_BF16 = 4e-3
TOL_F32 = 1e-4


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(BF).to(DEV)


def _nchw(t):
    return t.double().cpu().permute(0, 3, 1, 2)


def _ids(table):
    return ["-".join(str(v) for v in row) for row in table]


def _hold(what, err, tol):
    print(f"{what}: {err:.2e} (bound {tol:.0e})")
    assert err < tol, f"{what}: {err:.3e} >= {tol:.0e}"


# ----------------------------------------------------------------------------------------------------------------------
# stride-2 convolutions, every plan
# ----------------------------------------------------------------------------------------------------------------------
_FWD = [(p, 1, B, H, W, C, Cin) for p, B, H, W, C, Cin in R.CONV_FWD_PLANS] + R.CONV_FWD_SPLIT
_TR = [(p, 1, B, H, W, C, Cin) for p, B, H, W, C, Cin in R.CONV_T_PLANS] + R.CONV_T_SPLIT


@pytest.mark.parametrize("row", _FWD, ids=_ids(_FWD))
def test_conv4x4s2_every_plan(row):
    from stain2stain_amd import _native, ops
    L = _native.lib()
    plan, min_split, B, H, W, C, Cin = row
    assert L.s2s_conv4x4s2_plan(B, H, W, C, Cin) == plan
    ks = L.s2s_conv4x4s2_ksplit(B, H, W, C, Cin)
    assert ks >= min_split and (plan == 6 or min_split > 1 or ks == 1)
    x, w, b = R.conv_operands(B, Cin, 2 * H, 2 * W, C, 31 * plan + B)
    wf, _ = ops.pack_conv4x4_t(w.float().to(DEV), 2, BF)
    wide = torch.full((B, H, W, 2 * C + 8), 7.0, dtype=BF, device=DEV)
    y = ops.conv4x4s2(_nhwc(x), wf, b.float().to(DEV), C, act=True, slope=0.2, out2=wide[..., 8:8 + C])
    ref = R.conv_s2_reference(x, w, b)
    _hold("y = lrelu(conv + bias)", relerr(_nchw(y), F.leaky_relu(ref, 0.2)), TOL_BF16)
    _hold("out2 = relu(conv + bias)", relerr(_nchw(wide[..., 8:8 + C]), F.relu(ref)), TOL_BF16)
    assert bool((wide[..., :8] == 7.0).all()) and bool((wide[..., 8 + C:] == 7.0).all())
    # and the plain form (no bias, no activation): the same kernel's other epilogue
    y0 = ops.conv4x4s2(_nhwc(x), wf, None, C)
    _hold("y = conv", relerr(_nchw(y0), R.conv_s2_reference(x, w, None)), TOL_BF16)


@pytest.mark.parametrize("row", _TR, ids=_ids(_TR))
def test_convT4x4s2_every_plan(row):
    from stain2stain_amd import _native, ops
    L = _native.lib()
    plan, min_split, B, h, w_, C, Cin = row
    assert L.s2s_convt4x4s2_plan(B, h, w_, C, Cin) == plan
    ks = L.s2s_convt4x4s2_ksplit(B, h, w_, C, Cin)
    assert ks >= min_split and (plan == 6 or min_split > 1 or ks == 1)
    x, w, b = R.conv_operands(B, Cin, h, w_, C, 37 * plan + B, transposed=True)
    _, wd = ops.pack_conv4x4_t(w.float().to(DEV), 2, BF)
    wide = torch.full((B, 2 * h, 2 * w_, 2 * C + 8), -3.0, dtype=BF, device=DEV)
    ops.convT4x4s2(_nhwc(x), wd, b.float().to(DEV), C, out=wide[..., C:2 * C])
    _hold("y = convT + bias", relerr(_nchw(wide[..., C:2 * C]), R.convT_s2_reference(x, w, b)), TOL_BF16)
    assert bool((wide[..., :C] == -3.0).all()) and bool((wide[..., 2 * C:] == -3.0).all())


# ----------------------------------------------------------------------------------------------------------------------
# 4x4 weight gradients
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", R.WGRAD, ids=[r[0] for r in R.WGRAD])
def test_wgrad_bf16_every_kernel(row):
    from stain2stain_amd import _native, ops
    L = _native.lib()
    name, ks, plain, B, H, W, C, Cout = row
    cin = 4 * C if ks == 2 else C
    S, tiles = L.s2s_convkxk_wgrad_splits(0, B, H, W, cin, Cout, ks), R.wgrad_tiles(B, H, W)
    if name in R.WGRAD_UNEVEN:
        assert (S, tiles) == R.WGRAD_UNEVEN[name]
        assert tiles % S != 0 and -(-tiles // S) >= 3 and H % 8 != 0 and W % 16 != 0      # uneven, >= 3 for some split, ragged
    if name in R.WGRAD_FOLD4:
        assert S == R.WGRAD_FOLD4[name] and S >= 16 and -(-C // 64) * Cout <= 1024       # wgrad_fold4x4_kernel<4>
    elif not name.startswith(("flat", "small")):
        assert S < 16                                                                      # wgrad_fold4x4_kernel<1>
    if name.startswith("flat"):
        assert H <= 8 and W <= 8 and (B * H * W > 1024 or C % 16 != 0)
    if name.startswith("small"):
        assert B * H * W <= 1024 and C % 16 == 0 and ((B * H * W + 127) // 128 == 1) == (name == "small_1tile")
    x, dy, ref = R.wgrad_case(ks, B, H, W, C, Cout, 1000 + 7 * B + H)
    xg = _nhwc(x)
    if ks == 2 and not plain:
        xg = ops.space_to_depth_pad1_t(xg)
    dyg = _nhwc(dy)
    grad = torch.full((Cout, C, 4, 4), 3.0, dtype=torch.float32, device=DEV)
    ops.convkxk_wgrad(dyg, xg, grad, ks, x_plain=plain)
    _hold(f"{name}: dW", relerr(grad, ref), TOL_F32)
    ops.convkxk_wgrad(dyg, xg, grad, ks, accumulate=True, x_plain=plain)
    _hold(f"{name}: dW accumulated", relerr(grad, 2 * ref), TOL_F32)


@pytest.mark.parametrize("row", R.WGRAD_LAYOUT0, ids=_ids(R.WGRAD_LAYOUT0))
def test_wgrad_bf16_tap_major_layout(row):
    """layout 0 through the raw entry point: grad[ks*ks][Cout][cin], reduced by split_sum_kernel.  For ks = 2 the operand
    is any [B, H+1, W+1, cin] tensor and the reference the weight gradient of a plain 2x2 convolution over it."""
    from stain2stain_amd import _native, ops
    L = _native.lib()
    ks, B, H, W, cin, Cout = row
    g = torch.Generator().manual_seed(5 + ks)
    x = torch.randn(B, cin, H + 1, W + 1, generator=g, dtype=torch.float64).to(BF).double()
    dy = torch.randn(B, Cout, H, W, generator=g, dtype=torch.float64).to(BF).double()
    ref = torch.nn.grad.conv2d_weight(x, (Cout, cin, ks, ks), dy, stride=1, padding=1 if ks == 4 else 0)
    ref = ref.permute(2, 3, 0, 1).reshape(ks * ks, Cout, cin)
    S = L.s2s_convkxk_wgrad_splits(0, B, H, W, cin, Cout, ks)
    assert S > 1
    part = torch.empty(S * ks * ks * Cout * cin, dtype=torch.float32, device=DEV)
    grad = torch.full((ks * ks, Cout, cin), 3.0, dtype=torch.float32, device=DEV)
    xg, dyg = _nhwc(x), _nhwc(dy)
    for acc in (0, 1):
        rc = L.s2s_convkxk_wgrad_nhwc(0, dyg.data_ptr(), Cout, Cout, xg.data_ptr(), cin, cin, part.data_ptr(), grad.data_ptr(),
                                      0, acc, B, H, W, ks, 0, ops._stream())
        assert rc == 0
        _hold(f"layout 0, ks {ks}, accumulate {acc}", relerr(grad, (1 + acc) * ref), TOL_F32)


# ----------------------------------------------------------------------------------------------------------------------
# conv_small.hip forward
# ----------------------------------------------------------------------------------------------------------------------
def _check_norm_of_stored_raw(raw, y, y2, st, slope):
    rawn = _nchw(raw)
    ref = R.instnorm_reference(rawn, None, None, slope)
    _hold("y against the norm of the stored raw", relerr(_nchw(y), ref["y"]), TOL_BF16)
    if y2 is not None:
        _hold("y2 against the norm of the stored raw", relerr(_nchw(y2), ref["y2"]), TOL_BF16)
    st = st.double().cpu()
    _hold("mean", float((st[0] - ref["stats"][0]).abs().max()) / max(1.0, float(rawn.abs().max())), R.TOL_STAT)
    _hold("1/std", float(((st[1] - ref["stats"][1]).abs() / ref["stats"][1]).max()), R.TOL_STAT)


@pytest.mark.parametrize("row", R.CONVSM_FWD, ids=_ids(R.CONVSM_FWD))
def test_convsm_forward_conv_norm(row):
    from stain2stain_amd import ops
    B, ho, cin, cout, slope = row
    x, w, b = R.conv_operands(B, cin, 2 * ho, 2 * ho, cout, 100 * B + ho)
    wf, _ = ops.pack_conv4x4_t(w.float().to(DEV), 2, BF)
    wide = torch.full((B, ho, ho, 2 * cout), 7.0, dtype=BF, device=DEV)
    y, raw, st = ops.convsm_fwd(1, _nhwc(x), wf, b.float().to(DEV), cout, norm=True, slope=slope, out2=wide[..., :cout])
    _hold("raw", relerr(_nchw(raw), R.conv_s2_reference(x, w, b)), TOL_BF16)
    _check_norm_of_stored_raw(raw, y, wide[..., :cout], st, slope)
    assert bool((wide[..., cout:] == 7.0).all())


@pytest.mark.parametrize("row", R.CONVSM_T, ids=_ids(R.CONVSM_T))
def test_convsm_forward_transposed_conv_norm(row):
    from stain2stain_amd import ops
    B, hi, cin, cout = row
    x, w, b = R.conv_operands(B, cin, hi, hi, cout, 10 * B + hi, transposed=True)
    _, wd = ops.pack_conv4x4_t(w.float().to(DEV), 2, BF)
    y, raw, st = ops.convsm_fwd(2, _nhwc(x), wd, b.float().to(DEV), cout, norm=True, slope=0.0)
    _hold("raw", relerr(_nchw(raw), R.convT_s2_reference(x, w, b)), TOL_BF16)
    _check_norm_of_stored_raw(raw, y, None, st, 0.0)
