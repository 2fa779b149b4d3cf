"""The teacher-forced references of tests/stepwise_ref.py against torch autograd of the layers they stand for
(nn.Conv2d, nn.BatchNorm2d, F.max_pool2d, F.interpolate) in fp64, so that the GPU tests of the bf16 step
(tests/test_stepwise_bf16_gpu.py) rest on references that are themselves tested.  No GPU needed."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import stepwise_ref as R
from conftest import relerr

BF = torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("c1", [0, 16])
def test_conv_references_match_conv2d_autograd(c1):
    g = _gen(1 + c1)
    B, H, W, c0, cout = 2, 9, 12, 24, 40
    x0 = R.bf(torch.rand(B, H, W, c0, generator=g) * 2 - 1)
    x1 = R.bf(torch.rand(B, H, W, c1, generator=g) * 2 - 1) if c1 else None
    w = R.bf((torch.rand(cout, c0 + c1, 3, 3, generator=g) * 2 - 1) * 0.2)
    b = torch.rand(cout, generator=g) - 0.5
    dy = R.bf(torch.rand(B, cout, H, W, generator=g) - 0.5)
    conv = torch.nn.Conv2d(c0 + c1, cout, 3, padding=1).double()
    with torch.no_grad():
        conv.weight.copy_(w.double()); conv.bias.copy_(b.double())
    xin = torch.cat([x0, x1], -1) if c1 else x0
    x = xin.permute(0, 3, 1, 2).double().requires_grad_(True)
    y = conv(x)
    y.backward(dy.double())
    xc = R.cat_input(x0, x1)
    assert torch.equal(xc, xin.permute(0, 3, 1, 2))
    assert relerr(R.conv3x3(xc, w, b), y) < 1e-5
    assert relerr(R.conv3x3(xc, w), y - b.double()[None, :, None, None]) < 1e-5
    assert relerr(R.conv3x3_dgrad(dy, w), x.grad) < 1e-5
    assert relerr(R.conv3x3_wgrad(xc, dy), conv.weight.grad) < 1e-5


def test_stem_image_rounds_to_bf16():
    x = torch.rand(2, 3, 5, 7, generator=_gen(2)) * 2 - 1
    s = R.stem_image(x)
    assert torch.equal(s, x.to(BF).float()) and not torch.equal(s, x)


def test_batchnorm_references_match_batchnorm2d():
    """Statistics of the bias-free conv output, scale / shift, and the running update of a BatchNorm2d that sits behind
    a biased conv (its input is conv + bias), against nn.BatchNorm2d in train mode, fp64."""
    g = _gen(3)
    B, H, W, C = 3, 6, 10, 16
    raw = torch.randn(B, H, W, C, generator=g, dtype=torch.float64) * 1.7 + 0.4
    bias = torch.rand(C, generator=g, dtype=torch.float64) - 0.5
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.rand(C, generator=g, dtype=torch.float64) - 0.5
    rm0 = torch.rand(C, generator=g, dtype=torch.float64)
    rv0 = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    bn = torch.nn.BatchNorm2d(C, momentum=0.1, eps=1e-5).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm0); bn.running_var.copy_(rv0)
    ref = bn(raw.permute(0, 3, 1, 2) + bias[None, :, None, None])            # what the reference network computes
    st = R.bn_stats(raw)
    scale, shift = R.bn_affine(st, gamma, beta)
    assert relerr(_nhwc(ref), raw * scale + shift) < 1e-12
    rm, rv = R.bn_running(rm0, rv0, st, 0.1, bias)
    assert relerr(rm, bn.running_mean) < 1e-12 and relerr(rv, bn.running_var) < 1e-12
    rm_nb, _ = R.bn_running(rm0, rv0, st, 0.1, None)
    assert relerr(rm_nb, bn.running_mean) > 1e-3              # the late bias is visible in the running mean
    y32, ys = R.bn_relu_apply(raw.float(), scale.float(), shift.float())
    assert relerr(y32, _nhwc(ref).clamp_min(0)) < 1e-6
    assert torch.equal(ys, y32.to(BF).float())
    assert float(R.bf16_ulps(ys, _nhwc(ref).clamp_min(0)).max()) <= 0.5 + 1e-3


def test_fma_emulation_is_single_rounding():
    """fmaf(x, s, h) rounds once: the emulation must not round the product to fp32 first."""
    x = torch.tensor([1.0 + 2.0 ** -12], dtype=torch.float32)
    s = torch.tensor([1.0 + 2.0 ** -12], dtype=torch.float32)
    h = torch.tensor([-1.0], dtype=torch.float32)
    fused = R.fma_f32(x, s, h)
    assert float(fused) == 2.0 ** -11 + 2.0 ** -24
    assert float(x * s + h) == 2.0 ** -11                   # the unfused fp32 expression loses the 2^-24 term


def _brute_force_winner(y):
    B, H, W, C = y.shape
    out = torch.empty(B, H // 2, W // 2, C, dtype=torch.long)
    for b, i, j, c in itertools.product(range(B), range(H // 2), range(W // 2), range(C)):
        vals = [float(y[b, 2 * i + di, 2 * j + dj, c]) for di, dj in ((0, 0), (0, 1), (1, 0), (1, 1))]
        out[b, i, j, c] = vals.index(max(vals))                   # the first maximum
    return out


def test_pool_tie_rule_matches_brute_force():
    g = _gen(4)
    y = torch.randint(0, 3, (2, 6, 8, 5), generator=g).float() * 0.5          # mostly ties
    win = R.pool_winner(y)
    assert torch.equal(win, _brute_force_winner(y))
    assert torch.equal(R.maxpool2(y), _nhwc(F.max_pool2d(y.permute(0, 3, 1, 2), 2)))
    gp = torch.rand(2, 3, 4, 5, generator=g)
    sc = R.pool_scatter(gp, win)
    assert torch.equal(sc.reshape(2, 3, 2, 4, 2, 5).sum((2, 4)), gp)
    for b, i, j, c in [(0, 0, 0, 0), (1, 2, 3, 4), (0, 1, 2, 3)]:
        k = int(win[b, i, j, c])
        assert float(sc[b, 2 * i + k // 2, 2 * j + k % 2, c]) == float(gp[b, i, j, c])


def _separated_raw(g, B, H, W, C):
    """Conv outputs whose 2x2 windows hold clearly different values (no pool ties even after bf16 rounding)."""
    base = torch.randn(B, H // 2, W // 2, 1, C, generator=g, dtype=torch.float64)
    perm = torch.stack([torch.randperm(4, generator=g) for _ in range(B * (H // 2) * (W // 2) * C)])
    off = perm.reshape(B, H // 2, W // 2, C, 4).permute(0, 1, 2, 4, 3).double() * 0.3
    q = base + off                                            # [B, H/2, W/2, 4, C]
    return q.reshape(B, H // 2, W // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)


@pytest.mark.parametrize("pooled", [True, False])
def test_bn_relu_backward_matches_autograd(pooled):
    """BN(train) -> ReLU -> {dense gradient, 2x2 max-pool gradient} backward against fp64 autograd of
    nn.BatchNorm2d / relu / F.max_pool2d (inputs without pool ties, so both pick the same winner)."""
    g = _gen(5 + pooled)
    B, H, W, C = 2, 8, 6, 16
    raw = R.bf(_separated_raw(g, B, H, W, C).float())
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.rand(C, generator=g) - 0.5
    g1 = R.bf(torch.rand(B, H, W, C, generator=g) - 0.5)
    gp = R.bf(torch.rand(B, H // 2, W // 2, C, generator=g) - 0.5) if pooled else None
    st = R.bn_stats(raw)
    scale, shift = R.bn_affine(st, gamma, beta)
    stats = torch.stack([st["mean"], st["invstd"], scale, shift]).float()
    bn = torch.nn.BatchNorm2d(C).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma.double()); bn.bias.copy_(beta.double())
    x = raw.permute(0, 3, 1, 2).double().requires_grad_(True)
    y = torch.relu(bn(x))
    loss = (y * g1.permute(0, 3, 1, 2).double()).sum()
    if pooled:
        loss = loss + (F.max_pool2d(y, 2) * gp.permute(0, 3, 1, 2).double()).sum()
    loss.backward()
    draw, dgamma, dbeta = R.bn_relu_bwd(g1, gp, raw, stats, gamma)
    assert relerr(draw, _nhwc(x.grad)) < 1e-5
    assert relerr(dgamma, bn.weight.grad) < 1e-5 and relerr(dbeta, bn.bias.grad) < 1e-5


def test_bn_relu_backward_gradient_only_through_the_pool():
    """g1 = None (an encoder level whose activation feeds nothing but the next level's pool)."""
    g = _gen(7)
    B, H, W, C = 1, 4, 4, 8
    raw = R.bf(_separated_raw(g, B, H, W, C).float())
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.zeros(C)
    gp = R.bf(torch.rand(B, H // 2, W // 2, C, generator=g) - 0.5)
    st = R.bn_stats(raw)
    scale, shift = R.bn_affine(st, gamma, beta)
    stats = torch.stack([st["mean"], st["invstd"], scale, shift]).float()
    a, _, _ = R.bn_relu_bwd(None, gp, raw, stats, gamma)
    b, _, _ = R.bn_relu_bwd(torch.zeros_like(raw), gp, raw, stats, gamma)
    assert torch.equal(a, b)


@pytest.mark.parametrize("hin", [1, 4, 7])
def test_upsample_matches_interpolate(hin):
    g = _gen(8 + hin)
    B, C = 2, 8
    x = torch.rand(B, hin, hin + 2, C, generator=g, dtype=torch.float64) * 2 - 1
    bias = torch.rand(B, C, generator=g, dtype=torch.float64) - 0.5
    dy = torch.rand(B, 2 * hin, 2 * hin + 4, C, generator=g, dtype=torch.float64) - 0.5
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    up = F.interpolate(xn + bias[:, :, None, None], scale_factor=2, mode="bilinear", align_corners=True)
    up.backward(dy.permute(0, 3, 1, 2))
    assert relerr(R.upsample2x(x, bias), _nhwc(up)) < 1e-12
    assert relerr(R.upsample2x(x) + bias[:, None, None, :], _nhwc(up)) < 1e-12     # align_corners weights sum to 1
    assert relerr(R.upsample2x_bwd(dy, hin, hin + 2), _nhwc(xn.grad)) < 1e-12
    assert relerr(R.pixel_sum(dy), dy.sum((1, 2))) < 1e-12


def test_head_loss_matches_autograd():
    g = _gen(9)
    B, H, W, C, cout = 2, 5, 6, 16, 3
    x = R.bf(torch.rand(B, H, W, C, generator=g) - 0.5)
    w = torch.rand(cout, C, 1, 1, generator=g) - 0.5
    b = torch.rand(cout, generator=g) - 0.5
    u = torch.rand(B, cout, H, W, generator=g) * 2 - 1
    xn = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    v = F.conv2d(xn, wd, bd)
    loss = F.mse_loss(v, u.double())
    loss.backward()
    l, vr, dx, dw, db = R.head_loss(x, w, b, u)
    assert abs(float(l) - float(loss.detach())) < 1e-12
    assert relerr(vr, v) < 1e-12 and relerr(R.head_fwd(x, w, b), v) < 1e-12
    assert relerr(dx, _nhwc(xn.grad)) < 1e-12 and relerr(dw, wd.grad) < 1e-12 and relerr(db, bd.grad) < 1e-12


def test_time_path_and_glue():
    from oracle import unet_oracle as O
    g = _gen(10)
    t = torch.rand(5, generator=g)
    assert relerr(R.time_embedding(t, 32), O.time_embedding(t, 32)) < 1e-6
    dec = torch.nn.Module()
    dec.time_mlp = torch.nn.Sequential(torch.nn.Linear(32, 32), torch.nn.SiLU(), torch.nn.Linear(32, 32))
    dec.time_proj = torch.nn.Linear(32, 24)
    temb = R.time_embedding(t, 32)
    dtb = torch.rand(5, 24, generator=g, dtype=torch.float64)
    tb, grads = R.time_path(temb, dec, dtb)
    dd = dec.double()
    x = temb.clone()
    ref = dd.time_proj(dd.time_mlp(x))
    ref.backward(dtb)
    assert relerr(tb, ref) < 1e-12
    for n, p in dd.named_parameters():
        assert relerr(grads[n], p.grad) < 1e-12, n
    x0 = torch.rand(3, 3, 4, 4, generator=g)
    x1 = torch.rand(3, 3, 4, 4, generator=g)
    tt = torch.rand(3, generator=g)
    xt, ut = R.cfm_sample(x0, x1, tt)
    assert relerr(xt, tt.double()[:, None, None, None] * x1 + (1 - tt.double()[:, None, None, None]) * x0) < 1e-12
    assert relerr(ut, x1.double() - x0.double()) < 1e-12


def test_eval_affine_matches_batchnorm_eval():
    bn = torch.nn.BatchNorm2d(8).double()
    g = _gen(11)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5, generator=g); bn.bias.uniform_(-0.5, 0.5, generator=g)
        bn.running_mean.uniform_(-1, 1, generator=g); bn.running_var.uniform_(0.5, 2, generator=g)
    bn.eval()
    x = torch.rand(2, 8, 3, 3, generator=g, dtype=torch.float64)
    sc, sh = R.eval_affine(bn)
    assert relerr(x * sc[None, :, None, None] + sh[None, :, None, None], bn(x)) < 1e-12


def test_bf16_ulps():
    r = torch.tensor([1.0, 1.0, 3.0, -0.75, 0.0])
    a = torch.tensor([1.0 + 2 ** -7, 1.0 + 2 ** -8, 3.0 + 2 ** -6, -0.75 - 2 ** -8, 0.0])
    assert torch.allclose(R.bf16_ulps(a, r), torch.tensor([1.0, 0.5, 1.0, 1.0, 0.0], dtype=torch.float64))


def test_recorder_restores_every_attribute():
    from stain2stain_amd import engine, ops
    names = [(engine, "_conv_bn_relu"), (engine, "_conv_bn_relu_bwd"), (ops, "conv3x3")] + \
        [(ops, n) for n in R.Recorder.OPS]
    before = [getattr(m, n) for m, n in names]
    with R.Recorder():
        assert all(getattr(m, n) is not f for (m, n), f in zip(names, before))
    assert all(getattr(m, n) is f for (m, n), f in zip(names, before))
    with pytest.raises(ZeroDivisionError):
        with R.Recorder():
            1 / 0
    assert all(getattr(m, n) is f for (m, n), f in zip(names, before))


def test_recorder_clones_at_call_time():
    """A wrapped op records its arguments as they were when it was called, even if the caller overwrites them later,
    and in-place outputs as they were when it returned."""
    from stain2stain_amd import ops
    calls = []
    orig = ops.axpy_

    def fake_axpy(x, y, a):
        calls.append(1)
        x.add_(y, alpha=a)
    ops.axpy_ = fake_axpy
    try:
        x, y = torch.ones(4), torch.full((4,), 2.0)
        with R.Recorder() as rec:
            ops.axpy_(x, y, 0.5)
        x.zero_()
    finally:
        ops.axpy_ = orig
    r = rec.calls["axpy_"][0]
    assert calls == [1]
    assert torch.equal(r["args"][0], torch.ones(4)) and torch.equal(r["after"][0], torch.full((4,), 2.0))
