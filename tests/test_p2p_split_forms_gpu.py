"""The deferred split-K path of the pix2pix step (bf16): a stride-2 convolution called with ``defer=True`` leaves its
partial slabs to the single-launch InstanceNorm (s2s_instnorm_lrelu_fwd_split / _bwd_split), which ops.py and instnorm.hip
both promise gives "the same bits" as reduce launch + two-launch form.  That promise is asserted here with torch.equal, on
the flat form at C <= 64 and C > 64, on non-flat split-K with tile plans 5, 1 and 3, at split counts of 2 and of 3 or
more, with a channel tail in the norm's 64-channel workgroup where the convolution takes one (the transposed form wants
C % 64 == 0).  The arithmetic of the two-launch form itself is pinned by test_instnorm_forms_gpu.py; the convolution
output is held to 4e-3 (one bf16 rounding is 2^-9) against the fp64 convolution of the bf16-rounded operands."""
import pytest
import torch

import p2p_forms_ref as R
from conftest import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ERR_NULL = -5


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(BF).to(DEV)


def _nchw(t):
    return t.double().cpu().permute(0, 3, 1, 2)


def _ids(table):
    return ["-".join(str(v) for v in row) for row in table]


def _conv(kind, x, wp, bias, C, defer):
    from stain2stain_amd import ops
    return (ops.conv4x4s2 if kind == "conv" else ops.convT4x4s2)(x, wp, bias, C, defer=defer)


@pytest.mark.parametrize("with_bias,slope", [(True, 0.2), (False, 0.0)])
@pytest.mark.parametrize("row", R.SPLIT_FWD + R.SPLIT_T, ids=_ids(R.SPLIT_FWD + R.SPLIT_T))
def test_deferred_split_gives_the_same_bits(row, with_bias, slope):
    from stain2stain_amd import _native, ops
    L = _native.lib()
    kind, plan, min_split, B, H, W, C, Cin = row
    T = kind == "convT"
    Ho, Wo = (2 * H, 2 * W) if T else (H, W)
    ksplit = (L.s2s_convt4x4s2_ksplit if T else L.s2s_conv4x4s2_ksplit)(B, H, W, C, Cin)
    assert (L.s2s_convt4x4s2_plan if T else L.s2s_conv4x4s2_plan)(B, H, W, C, Cin) == plan
    assert ksplit > 1 and ksplit >= min_split and ops.instnorm_split_ok(BF, Ho, Wo, C)
    x, w, b = R.conv_operands(B, Cin, H if T else 2 * H, W if T else 2 * W, C, 7 * B + H + C, transposed=T)
    wf, wd = ops.pack_conv4x4_t(w.float().to(DEV), 2, BF)
    wp = wd if T else wf
    bias = b.float().to(DEV) if with_bias else None
    xg = _nhwc(x)

    # ---- forward: reduce launch + two-launch form against slabs folded by the norm ----
    raw_a = _conv(kind, xg, wp, bias, C, False)
    wide_a = torch.full((B, Ho, Wo, 2 * C + 8), 5.0, dtype=BF, device=DEV)
    wide_b = wide_a.clone()
    y_a, y_b = torch.empty_like(raw_a), torch.empty_like(raw_a)
    st_a = ops.instnorm_lrelu_fwd2(raw_a, slope, y_a, wide_a[..., C:2 * C])
    sp = _conv(kind, xg, wp, bias, C, True)
    assert isinstance(sp, ops.SplitSum) and sp.slabs.shape[0] == ksplit and sp.shape == (B, Ho, Wo, C)
    st_b, raw_b = ops.instnorm_lrelu_fwd2_split(sp, slope, y_b, wide_b[..., C:2 * C])
    assert torch.equal(raw_a, raw_b) and torch.equal(y_a, y_b) and torch.equal(st_a, st_b)
    assert torch.equal(wide_a, wide_b)                              # y2 and the sentinel channels around it
    assert bool((wide_b[..., :C] == 5.0).all()) and bool((wide_b[..., 2 * C:] == 5.0).all())
    assert bool((wide_b[..., C:2 * C] >= 0).all()) and bool((wide_b[..., C:2 * C] != 5.0).any())
    ref = (R.convT_s2_reference if T else R.conv_s2_reference)(x, w, b if with_bias else None)
    err = relerr(_nchw(raw_b), ref)
    print(f"raw against fp64: {err:.2e}")
    assert err < 4e-3

    # ---- backward: g as the SplitSum of a deferred data-gradient convolution against g as the reduced tensor ----
    gen = torch.Generator().manual_seed(11 + C)
    gy = _nhwc(torch.randn(B, Cin, H if T else 2 * H, W if T else 2 * W, generator=gen))
    g2w = torch.full((B, Ho, Wo, C + 16), 2.0, dtype=BF, device=DEV)
    g2w[..., 8:8 + C] = torch.randn(B, Ho, Wo, C, generator=gen).to(BF).to(DEV)
    g_t = _conv(kind, gy, wp, None, C, False)
    for g2 in (None, g2w[..., 8:8 + C]):
        g_s = _conv(kind, gy, wp, None, C, True)
        assert isinstance(g_s, ops.SplitSum)
        dx_a = ops.instnorm_lrelu_bwd2(g_t, g2, raw_a, st_a, slope)
        dx_b = ops.instnorm_lrelu_bwd2(g_s, g2, raw_a, st_a, slope)
        assert torch.equal(dx_a, dx_b)
        assert bool(torch.isfinite(dx_b.float()).all()) and float(dx_b.float().abs().max()) > 0


def test_defer_is_refused_where_it_does_not_apply():
    """Host-side only: the entry points return the error status before any launch."""
    from stain2stain_amd import _native, ops
    L = _native.lib()
    _, _, _, B, H, W, C, Cin = R.SPLIT_FWD[0]
    assert L.s2s_conv4x4s2_ksplit(B, H, W, C, Cin) > 1
    x = torch.zeros((B, 2 * H, 2 * W, Cin), dtype=BF, device=DEV)
    wf = torch.zeros(((4 * Cin + 31) // 32, 4, C, 32), dtype=BF, device=DEV)
    y2 = torch.zeros((B, H, W, C), dtype=BF, device=DEV)
    kwork = torch.zeros((64, B * H * W, C), dtype=torch.float32, device=DEV)

    def conv(y2p, act, b, h, w):
        return L.s2s_conv4x4s2_nhwc(0, x.data_ptr(), Cin, Cin, wf.data_ptr(), 0, 0, C, y2p, C if y2p else 8, act, 0.2,
                                    kwork.data_ptr(), b, h, w, C, ops._stream())
    assert conv(0, 1, B, H, W) == ERR_NULL                        # with the activation in the epilogue
    assert conv(y2.data_ptr(), 0, B, H, W) == ERR_NULL            # with a second output
    plan, B1, H1, W1, C1, Cin1 = R.CONV_FWD_PLANS[1]
    assert L.s2s_conv4x4s2_ksplit(B1, H1, W1, C1, Cin1) == 1
    x1 = torch.zeros((B1, 2 * H1, 2 * W1, Cin1), dtype=BF, device=DEV)
    w1 = torch.zeros(((4 * Cin1 + 31) // 32, 4, C1, 32), dtype=BF, device=DEV)
    k1 = torch.zeros((2, B1 * H1 * W1, C1), dtype=torch.float32, device=DEV)
    assert L.s2s_conv4x4s2_nhwc(0, x1.data_ptr(), Cin1, Cin1, w1.data_ptr(), 0, 0, C1, 0, 8, 0, 0.0, k1.data_ptr(), B1, H1,
                                W1, C1, ops._stream()) == ERR_NULL                                       # an unsplit shape
    assert L.s2s_conv4x4s2_nhwc(0, x.data_ptr(), Cin, Cin, wf.data_ptr(), 0, 0, C, 0, 8, 0, 0.0, 0, B, H, W, C,
                                ops._stream()) == ERR_NULL                                               # no slab buffer
    plan, Bt, ht, wt, Ct, Cint = R.CONV_T_PLANS[1]
    assert L.s2s_convt4x4s2_ksplit(Bt, ht, wt, Ct, Cint) == 1
    xt = torch.zeros((Bt, ht, wt, Cint), dtype=BF, device=DEV)
    wdt = torch.zeros(((Cint + 31) // 32, 16, Ct, 32), dtype=BF, device=DEV)
    kt = torch.zeros((2, Bt * 4 * ht * wt, Ct), dtype=torch.float32, device=DEV)
    assert L.s2s_convt4x4s2_nhwc(0, xt.data_ptr(), Cint, Cint, wdt.data_ptr(), 0, 0, Ct, kt.data_ptr(), Bt, ht, wt, Ct,
                                 ops._stream()) == ERR_NULL                                              # an unsplit shape
    # and ops.py never asks for it there: the call runs undeferred and returns the tensor
    assert torch.is_tensor(ops.conv4x4s2(x, wf.view(-1), None, C, act=True, slope=0.2, defer=True))
    assert torch.is_tensor(ops.conv4x4s2(x, wf.view(-1), None, C, out2=y2, defer=True))
    assert torch.is_tensor(ops.conv4x4s2(x1, w1.view(-1), None, C1, defer=True))
