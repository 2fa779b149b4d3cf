"""Kernel parity on poisoned memory: every buffer a HIP entry point is handed from ``torch.empty`` (outputs, BatchNorm
partial rows, split-K slabs, loss / reduction partials) and every cached ``ops._workspace`` slab starts out as NaN, so a
kernel that leaves an element unwritten which is later read shows up as a non-finite or wrong result instead of reading
the allocator's kindly zeros.

  * ``torch.use_deterministic_algorithms(True)`` with ``torch.utils.deterministic.fill_uninitialized_memory`` fills
    every ``torch.empty`` with NaN (floats, bf16) or the integer maximum (checked on the device by the first test);
  * ``ops._workspace`` is wrapped so that each slab it hands out is filled with 0xFF bytes first -- NaN read as float32
    and as float64 (seg_eval / head_mse_eval view their slabs as doubles);
  * wrappers taking ``out=`` run once into NaN and once into a finite sentinel (1e4): a kernel that reads the old
    contents (``fmaxf``, ``+=``) can hide a NaN but not the sentinel.

The 3x3 convolution cases pin the kernel family they were written for (``s2s_conv3x3_family``).  Tolerances are those of
the parity tests the cases come from (tests/test_ops_gpu.py); the parity tests imported at the end run unchanged under
the poison fixture."""
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Conv3x3Family (conv3x3_mfma.hip) as s2s_conv3x3_family returns it
STAGE_RESIDENT, STAGE_STREAM, PERS_CARRY, PERS, TAP, SPLIT_F32 = range(6)


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    from stain2stain_amd import ops
    import torch.utils.deterministic as tud
    prev_det, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    prev_fill = tud.fill_uninitialized_memory
    orig = ops._workspace

    def poisoned(device, numel, tag):
        buf = orig(device, numel, tag)
        buf.view(torch.uint8).fill_(255)
        return buf

    torch.use_deterministic_algorithms(True, warn_only=True)
    tud.fill_uninitialized_memory = True
    try:
        for buf in ops._WORKSPACE.values():
            buf.view(torch.uint8).fill_(255)
        monkeypatch.setattr(ops, "_workspace", poisoned)
        yield
    finally:
        torch.use_deterministic_algorithms(prev_det, warn_only=prev_warn)
        tud.fill_uninitialized_memory = prev_fill


def finite(t):
    return bool(torch.isfinite(t.float()).all())


def nhwc(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV, dtype)


def nchw(y):
    return y.float().cpu().permute(0, 3, 1, 2).contiguous()


def rnd(x, dtype):
    return x.to(dtype).float() if dtype == torch.bfloat16 else x


def test_poison_is_on():
    from stain2stain_amd import ops
    assert torch.empty(1000, device=DEV).isnan().all()
    assert torch.empty(1000, device=DEV, dtype=torch.bfloat16).isnan().all()
    assert (torch.empty(100, device=DEV, dtype=torch.int64) == torch.iinfo(torch.int64).max).all()
    assert ops._workspace(torch.device(DEV), 64, "probe").isnan().all()
    assert ops._workspace(torch.device(DEV), 64, "probe").view(torch.float64).isnan().all()


# ---------------------------------------------------------------------------------------------------------------------
# 3x3 convolution: one case per launch family
# ---------------------------------------------------------------------------------------------------------------------
FAMILY_CASES = [
    # id, (B, H, W, c0, c1, cout), bias, affine, stats, stat_rows (-1 = the launch's preferred layout, 0 = per tile),
    # split-K workspace, fp32, {S2S_CONV_STAGE: family}  (tests/test_env_variants_gpu.py runs these under
    # S2S_CONV_STAGE=0 too: that is where the persistent kernel carries statistics)
    ("resident_stats_plain", (1, 240, 270, 64, 0, 256), 0, 0, 1, -1, 0, 0, {1: STAGE_RESIDENT, 0: TAP}),
    ("resident_stats_xcd", (1, 256, 256, 8, 0, 256), 0, 0, 1, -1, 0, 0, {1: STAGE_RESIDENT, 0: TAP}),
    ("resident_stats_gy3", (2, 200, 256, 32, 32, 192), 0, 0, 1, -1, 0, 0, {1: STAGE_RESIDENT, 0: PERS}),
    ("resident_stats_per_tile_rows", (1, 240, 270, 16, 0, 256), 0, 0, 1, 0, 0, 0, {1: TAP, 0: TAP}),
    ("resident_plain", (2, 200, 256, 64, 0, 136), 0, 0, 0, -1, 0, 0, {1: STAGE_RESIDENT, 0: PERS}),
    ("resident_eval_affine", (1, 240, 270, 64, 0, 200), 1, 1, 0, -1, 0, 0, {1: STAGE_RESIDENT, 0: TAP}),
    ("stream_stats", (4, 250, 270, 64, 8, 40), 0, 0, 1, -1, 0, 0, {1: STAGE_STREAM, 0: PERS_CARRY}),
    ("stream_plain", (4, 250, 270, 64, 8, 40), 0, 0, 0, -1, 0, 0, {1: STAGE_STREAM, 0: PERS}),
    ("stream_stats_carried", (4, 256, 256, 96, 0, 24), 0, 0, 1, -1, 0, 0, {1: STAGE_STREAM, 0: PERS_CARRY}),
    ("pers_stats_per_tile", (6, 64, 256, 96, 0, 192), 0, 0, 1, -1, 0, 0, {1: PERS, 0: PERS}),
    ("pers_plain", (6, 64, 256, 96, 0, 192), 0, 0, 0, -1, 0, 0, {1: PERS, 0: PERS}),
    ("tap_bias_stats", (2, 20, 37, 16, 0, 24), 1, 0, 1, -1, 0, 0, {1: TAP, 0: TAP}),
    ("tap_eval_affine", (3, 12, 10, 40, 0, 200), 1, 1, 0, -1, 0, 0, {1: TAP, 0: TAP}),
    ("tap_ksplit", (1, 16, 16, 256, 64, 192), 1, 0, 0, -1, 1, 0, {1: TAP, 0: TAP}),
    ("tap_ksplit_affine", (2, 8, 8, 256, 0, 72), 0, 1, 0, -1, 1, 0, {1: TAP, 0: TAP}),
    ("split_f32_stats", (2, 20, 37, 16, 8, 72), 1, 0, 1, -1, 0, 1, {1: SPLIT_F32, 0: SPLIT_F32}),
]


@pytest.mark.parametrize("case", FAMILY_CASES, ids=[c[0] for c in FAMILY_CASES])
def test_conv3x3_family_poisoned(case):
    from stain2stain_amd import ops
    _, (B, H, W, c0, c1, cout), has_bias, affine, stats, rows_req, kwork, f32, want = case
    dtype = torch.float32 if f32 else torch.bfloat16
    dt = 1 if f32 else 0
    L = ops._L()
    mode = int(os.environ.get("S2S_CONV_STAGE", "1"))
    pers_off = os.environ.get("S2S_CONV_PERS") == "0"
    g = torch.Generator().manual_seed(31)
    x = torch.rand(B, c0 + c1, H, W, generator=g) * 2 - 1
    w = (torch.rand(cout, c0 + c1, 3, 3, generator=g) * 2 - 1) * 0.1
    b = torch.rand(cout, generator=g) - 0.5 if has_bias else None
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.rand(cout, generator=g) - 0.5
    xs = nhwc(x, dtype)
    ld = c0 + c1
    x0, x1 = xs[..., :c0], (xs[..., c0:] if c1 else None)
    wf, _ = ops.pack_conv3x3(w.to(DEV), dtype)
    rows = L.s2s_conv3x3_stat_blocks(dt, B, H, W, cout) if rows_req == 0 else \
        L.s2s_conv3x3_stat_rows(dt, B, H, W, cout, c0, c1, ld, ld, has_bias)
    fam = L.s2s_conv3x3_family(dt, B, H, W, cout, c0, c1, ld, ld, cout, has_bias, affine, stats,
                               rows_req if stats else -1, kwork)
    if mode in want and not pers_off and os.environ.get("S2S_CONV_XCD", "1") == "1":
        assert fam == want[mode], (fam, want[mode])
    if fam == STAGE_RESIDENT and stats:
        assert rows == 256 * 8
    nsplit = L.s2s_conv3x3_ksplit(dt, B, H, W, cout, c0 + c1) if kwork else 1
    if kwork:
        assert nsplit > 1
    ref = F.conv2d(rnd(x, dtype), rnd(w, dtype), b, padding=1)          # (fp32 on the CPU: these are GFLOPs)
    if affine:
        ref = ref * sc[None, :, None, None] + sh[None, :, None, None]
    tol = 4e-3 if dtype == torch.bfloat16 else 1e-4
    for fill in (float("nan"), 1e4):
        y = torch.full((B, H, W, cout), fill, device=DEV, dtype=dtype)
        stat = torch.full((2, cout, rows), fill, device=DEV) if stats else None
        kw = torch.full((nsplit, B * H * W, cout), fill, device=DEV) if kwork else None
        rc = L.s2s_conv3x3_nhwc_s(dt, x0.data_ptr(), ld, c0, x1.data_ptr() if c1 else None, ld, c1, wf.data_ptr(),
                                  None if b is None else bd(b).data_ptr(),
                                  y.data_ptr(), cout, None if stat is None else stat.data_ptr(), rows if stats else 0,
                                  bd(sc).data_ptr() if affine else None, bd(sh).data_ptr() if affine else None, 0,
                                  None if kw is None else kw.data_ptr(), B, H, W, cout, ops._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert finite(y), fill
        yb = nchw(y)
        assert relerr(yb, ref) < tol, fill
        if stats:
            assert finite(stat), fill
            s = stat.double().sum(-1).cpu()
            assert relerr(s[0], yb.double().sum((0, 2, 3))) < 2e-4, fill
            assert relerr(s[1], (yb.double() ** 2).sum((0, 2, 3))) < 2e-4, fill
    if not stats and not kwork:                        # the wrapper's own buffers (out= as NaN and as a sentinel)
        for fill in (None, float("nan"), 1e4):
            out = None if fill is None else torch.full((B, H, W, cout), fill, device=DEV, dtype=dtype)
            y, _ = ops.conv3x3(x0, x1, wf, None if b is None else b.to(DEV), cout, out=out,
                               scale=sc.to(DEV) if affine else None, shift=sh.to(DEV) if affine else None)
            assert finite(y) and relerr(nchw(y), ref) < tol


_KEEP = []


def bd(t):
    """A device copy that stays alive until the launch that reads its pointer has run."""
    d = t.to(DEV).float().contiguous()
    _KEEP.append(d)
    del _KEEP[:-8]
    return d


@pytest.mark.parametrize("order", ["small_after_large", "large_after_small"])
def test_conv3x3_wgrad_shares_its_workspace(order):
    """Two weight-gradient launches of different sizes on the one cached slab buffer: the second must not read slabs
    the first left behind (the buffer is poisoned before each)."""
    from stain2stain_amd import ops
    shapes = [(2, 96, 128, 64, 0, 64), (1, 9, 70, 8, 8, 72)]
    if order == "large_after_small":
        shapes = shapes[::-1]
    g = torch.Generator().manual_seed(41)
    for B, H, W, c0, c1, cout in shapes:
        for dtype in (torch.bfloat16, torch.float32):
            cin = c0 + c1
            x = torch.rand(B, cin, H, W, generator=g) * 2 - 1
            dy = torch.rand(B, cout, H, W, generator=g) * 2 - 1
            wv = torch.zeros(cout, cin, 3, 3, requires_grad=True)
            (F.conv2d(rnd(x, dtype), wv, None, padding=1) * rnd(dy, dtype)).sum().backward()
            xs = nhwc(x, dtype)
            for fill in (float("nan"), 1e4):
                grad = torch.full((cout, cin, 3, 3), fill, device=DEV)
                ops.conv3x3_wgrad(nhwc(dy, dtype), xs[..., :c0], xs[..., c0:] if c1 else None, grad, accumulate=False)
                assert finite(grad) and relerr(grad.cpu(), wv.grad) < 1e-4, (B, H, W, dtype, fill)


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm / resampling wrappers where the existing tests pre-zero or pass fresh buffers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_upsample_pad_is_written(dtype):
    """engine.decoder_forward hands upsample2x_fwd an empty concat buffer: the kernel writes the zero pad itself."""
    from oracle import unet_oracle as O
    from stain2stain_amd import ops
    g = torch.Generator().manual_seed(43)
    B, C, h, w, Ho, Wo = 2, 24, 5, 6, 11, 14
    x = rnd(torch.rand(B, C, h, w, generator=g) * 2 - 1, dtype)
    bias = torch.rand(B, C, generator=g) - 0.5
    up = O.upsample2x_bilinear_ac(x.double() + bias.double()[:, :, None, None])
    up = F.pad(up, [(Wo - 2 * w) // 2, Wo - 2 * w - (Wo - 2 * w) // 2, (Ho - 2 * h) // 2, Ho - 2 * h - (Ho - 2 * h) // 2])
    for fill in (None, 1e4):
        buf = torch.empty(B, Ho, Wo, C + 8, device=DEV, dtype=dtype) if fill is None else \
            torch.full((B, Ho, Wo, C + 8), fill, device=DEV, dtype=dtype)
        ops.upsample2x_fwd(nhwc(x, dtype), buf[..., 8:], bias.to(DEV))
        out = buf[..., 8:]
        assert finite(out) and relerr(nchw(out), up) < (4e-3 if dtype == torch.bfloat16 else 1e-4)
    gy = rnd(torch.rand(B, C, Ho, Wo, generator=g) - 0.5, dtype)
    xr = x.double().requires_grad_(True)
    upr = O.upsample2x_bilinear_ac(xr)
    upr = F.pad(upr, [(Wo - 2 * w) // 2, Wo - 2 * w - (Wo - 2 * w) // 2, (Ho - 2 * h) // 2, Ho - 2 * h - (Ho - 2 * h) // 2])
    (upr * gy.double()).sum().backward()
    dx = ops.upsample2x_bwd(nhwc(gy, dtype), h, w)
    assert finite(dx) and relerr(nchw(dx), xr.grad) < (4e-3 if dtype == torch.bfloat16 else 1e-4)
    ps = ops.pixel_sum(dx)
    assert finite(ps) and relerr(ps.cpu(), nchw(dx).double().sum((2, 3))) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bn_apply_pool_and_backward_into_sentinels(dtype):
    from stain2stain_amd import ops
    g = torch.Generator().manual_seed(44)
    B, C, H, W = 3, 24, 13, 11
    z = rnd(torch.rand(B, C, H, W, generator=g) * 4 - 2, dtype)
    zs = nhwc(z, dtype)
    n = B * H * W
    # partial sums in several rows, some of them zero (a producer that had no pixels of a channel)
    stat = torch.zeros(2, C, 5, device=DEV)
    stat[0, :, 1] = zs.float().sum((0, 1, 2))
    stat[1, :, 3] = (zs.float() ** 2).sum((0, 1, 2))
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    st = ops.bn_finalize(stat, n, gamma.to(DEV), beta.to(DEV), rm, rv, None)
    zd = z.double()
    mean, var = zd.mean((0, 2, 3)), zd.var((0, 2, 3), unbiased=False)
    assert finite(st) and relerr(st[0].cpu(), mean) < 1e-5 and relerr(st[1].cpu(), (var + 1e-5).rsqrt()) < 1e-5
    y_ref = ((zd - mean[None, :, None, None]) * (var + 1e-5).rsqrt()[None, :, None, None] * gamma.double()[None, :, None, None]
             + beta.double()[None, :, None, None]).clamp_min(0)
    y_ref = rnd(y_ref.float(), dtype).double()
    p_ref = F.max_pool2d(y_ref, 2)
    tol = 4e-3 if dtype == torch.bfloat16 else 1e-4
    for fill in (None, float("nan"), 1e4):
        out = None if fill is None else torch.full((B, H, W, C), fill, device=DEV, dtype=dtype)
        pool = None if fill is None else torch.full((B, H // 2, W // 2, C), fill, device=DEV, dtype=dtype)
        y, p = ops.bn_relu_apply(zs, st[2], st[3], out=out, pool=pool, want_pool=True)
        assert finite(y) and finite(p)
        assert relerr(nchw(y), y_ref) < tol and relerr(nchw(p), p_ref) < tol, fill
    mp = ops.maxpool2(y)
    assert finite(mp) and relerr(nchw(mp), F.max_pool2d(nchw(y).double(), 2)) == 0.0
    g1 = rnd(torch.rand(B, C, H, W, generator=g) - 0.5, dtype)
    gp = rnd(torch.rand(B, C, H // 2, W // 2, generator=g) - 0.5, dtype)
    zr = zd.clone().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    m_, v_ = zr.mean((0, 2, 3)), zr.var((0, 2, 3), unbiased=False)
    yr = ((zr - m_[None, :, None, None]) * (v_ + 1e-5).rsqrt()[None, :, None, None] * gr[None, :, None, None]
          + br[None, :, None, None]).clamp_min(0)
    if dtype == torch.bfloat16:   # the kernel pools the stored (bf16) value: pool winners are taken after the rounding
        yr = yr + (yr.detach().to(dtype).double() - yr.detach())
    ((yr * g1.double()).sum() + (F.max_pool2d(yr, 2) * gp.double()).sum()).backward()
    dgam, dbet, dbias = (torch.full((C,), 1e4, device=DEV) for _ in range(3))
    dz = ops.bn_relu_bwd(nhwc(g1, dtype), nhwc(gp, dtype), zs, st, gamma.to(DEV), dgam, dbet, dbias)
    assert finite(dz) and finite(dgam) and finite(dbet) and finite(dbias)
    assert relerr(nchw(dz), zr.grad) < tol * 2
    assert relerr(dgam.cpu(), gr.grad) < (5e-3 if dtype == torch.bfloat16 else 1e-4)
    assert relerr(dbet.cpu(), br.grad) < (5e-3 if dtype == torch.bfloat16 else 1e-4)


# ---------------------------------------------------------------------------------------------------------------------
# trainers: one eager step with and without poison, from the same state dict
# ---------------------------------------------------------------------------------------------------------------------
def _run_cfm(precision, features, size, batch):
    from stain2stain_amd import CFMTrainer, FlowUNet
    torch.manual_seed(5)
    net = FlowUNet(3, features, 3, 32, precision=precision)
    g = torch.Generator().manual_seed(6)
    x0 = torch.rand(batch, 3, size, size, generator=g) * 2 - 1
    x1 = torch.rand(batch, 3, size, size, generator=g) * 2 - 1
    t = torch.rand(batch, generator=g)
    net = net.to(DEV).train()
    tr = CFMTrainer(net, lr=1e-4, weight_decay=1e-5)
    loss, v = tr.forward_backward(x0.to(DEV), x1.to(DEV), t.to(DEV))
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    tr.optimizer_step()
    torch.cuda.synchronize()
    params = {k: p.detach().clone() for k, p in net.state_dict().items()}
    tr.close()
    return loss.detach().clone(), v.detach().clone(), grads, params


def _unpoisoned(fn):
    import torch.utils.deterministic as tud
    from stain2stain_amd import ops
    prev = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(False)
    wrapped = ops._workspace
    ops._workspace = _ORIG_WORKSPACE[0]
    try:
        return fn()
    finally:
        ops._workspace = wrapped
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


_ORIG_WORKSPACE = []


@pytest.fixture(autouse=True, scope="module")
def _orig_workspace():
    from stain2stain_amd import ops
    _ORIG_WORKSPACE[:] = [ops._workspace]
    yield


def _bit_equal(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _bit_equal(a[k], b[k], f"{what}/{k}")
        return
    assert finite(a), what
    assert torch.equal(a, b), what


@pytest.mark.parametrize("precision,features,size,batch", [("bf16", [64, 128], 256, 4), ("fp32", [16, 32], 64, 2)])
def test_cfm_trainer_step_is_bit_equal_under_poison(precision, features, size, batch):
    from stain2stain_amd import ops
    if precision == "bf16":          # the first level's statistics launch runs on the staged kernel, filter resident
        c = features[0]
        fam = ops._L().s2s_conv3x3_family(0, batch, size, size, c, c, 0, c, c, c, 0, 0, 1, -1, 0)
        if os.environ.get("S2S_CONV_STAGE", "1") == "1":
            assert fam == STAGE_RESIDENT
    clean = _unpoisoned(lambda: _run_cfm(precision, features, size, batch))
    dirty = _run_cfm(precision, features, size, batch)
    for a, b, what in zip(dirty, clean, ("loss", "v", "grad", "param")):
        _bit_equal(a, b, what)


def _run_multitask():
    from stain2stain_amd import FlowMatchingDecoder, MultiTaskTrainer, SegmentationDecoder, SharedEncoder
    torch.manual_seed(7)
    enc = SharedEncoder(3, [16, 32], precision="fp32").to(DEV).train()
    fdec = FlowMatchingDecoder(32, [16], 3, 32, precision="fp32").to(DEV).train()
    sdec = SegmentationDecoder(32, [16], 1, precision="fp32").to(DEV).train()
    g = torch.Generator().manual_seed(8)
    x0 = torch.rand(2, 3, 40, 48, generator=g) * 2 - 1
    x1 = torch.rand(2, 3, 40, 48, generator=g) * 2 - 1
    mask = (torch.rand(2, 1, 40, 48, generator=g) > 0.5).float()
    t = torch.rand(2, generator=g)
    tr = MultiTaskTrainer(enc, fdec, sdec, time_emb_dim=32, lr=1e-4, weight_decay=1e-5)
    losses, outs = tr.forward_backward(x0.to(DEV), x1.to(DEV), mask.to(DEV), t.to(DEV), want_outputs=True)
    mods = (("e.", enc), ("f.", fdec), ("s.", sdec))
    grads = {pre + k: p.grad.detach().clone() for pre, m in mods for k, p in m.named_parameters()}
    tr.optimizer_step()
    torch.cuda.synchronize()
    params = {pre + k: v.detach().clone() for pre, m in mods for k, v in m.state_dict().items()}
    out = ({k: v.detach().clone() for k, v in losses.items()}, {k: v.detach().clone() for k, v in outs.items()},
           grads, params)
    if hasattr(tr, "close"):
        tr.close()
    return out


def test_multitask_trainer_step_is_bit_equal_under_poison():
    clean = _unpoisoned(_run_multitask)
    dirty = _run_multitask()
    for a, b, what in zip(dirty, clean, ("losses", "outputs", "grad", "param")):
        _bit_equal(a, b, what)


def _run_pix2pix():
    from stain2stain_amd import PatchGANDiscriminator, Pix2PixGenerator, Pix2PixTrainer
    torch.manual_seed(9)
    G, D = Pix2PixGenerator(ngf=16, num_downs=5), PatchGANDiscriminator(ndf=16)
    g = torch.Generator().manual_seed(10)
    src = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    tgt = torch.rand(2, 3, 64, 64, generator=g) * 2 - 1
    G, D = G.to(DEV), D.to(DEV)
    tr = Pix2PixTrainer(G, D, precision="bf16")
    losses = tr.step(src.to(DEV), tgt.to(DEV))
    torch.cuda.synchronize()
    params = {**{"G." + k: v.detach().clone() for k, v in G.state_dict().items()},
              **{"D." + k: v.detach().clone() for k, v in D.state_dict().items()}}
    out = (losses.detach().clone(), params)
    tr.close()
    return out


def test_pix2pix_trainer_step_is_bit_equal_under_poison():
    clean = _unpoisoned(_run_pix2pix)
    dirty = _run_pix2pix()
    for a, b, what in zip(dirty, clean, ("losses", "param")):
        _bit_equal(a, b, what)


# ---------------------------------------------------------------------------------------------------------------------
# the existing parity tests of the other entry points, run under the poison fixture
# ---------------------------------------------------------------------------------------------------------------------
from test_ops_gpu import test_stem_and_head as test_poisoned_stem_and_head  # noqa: E402
from test_ops_gpu import test_bn_relu_pool_forward_backward as test_poisoned_bn_relu_pool  # noqa: E402
from test_ops_gpu import test_time_path_and_loss as test_poisoned_time_path_and_loss  # noqa: E402
from test_ops_gpu import test_head_loss_fused_matches_separate_ops as test_poisoned_head_loss_fused  # noqa: E402
from test_instnorm_gpu import test_ops_against_torch as test_poisoned_instnorm  # noqa: E402
from test_pix2pix_engine_gpu import test_conv_s2_transposed_and_s1_against_torch as test_poisoned_p2p_convs  # noqa: E402
from test_pix2pix_engine_gpu import test_loss_and_activation_kernels_against_torch as test_poisoned_p2p_losses  # noqa: E402
from test_pix2pix_engine_gpu import test_instnorm_second_output_and_second_gradient as test_poisoned_instnorm2  # noqa: E402
from test_conv4x4_gpu import test_conv4x4_stride2_forward_and_input_gradient as test_poisoned_conv4x4s2  # noqa: E402
from test_conv4x4_gpu import test_conv_transpose4x4_stride2 as test_poisoned_convT4x4s2  # noqa: E402
from test_conv4x4_gpu import test_conv4x4_stride1_forward_and_input_gradient as test_poisoned_conv4x4s1  # noqa: E402
from test_conv4x4_gpu import test_channel_sum as test_poisoned_channel_sum  # noqa: E402
from test_conv_small_gpu import test_conv_norm_forward as test_poisoned_convsm_fwd  # noqa: E402
from test_conv_small_gpu import test_transposed_conv_norm_forward as test_poisoned_convsm_tfwd  # noqa: E402
from test_conv_small_gpu import test_conv_data_gradient_ends_in_the_norm_backward as test_poisoned_convsm_bwd  # noqa: E402
from test_conv_small_gpu import test_weight_gradient_without_slabs as test_poisoned_convsm_wgrad  # noqa: E402
from test_multitask_gpu import test_seg_loss_kernel_matches_oracle as test_poisoned_seg_loss  # noqa: E402
from test_multitask_gpu import test_multiclass_loss_kernel_matches_oracle as test_poisoned_seg_loss_mc  # noqa: E402
from test_eval_metrics_gpu import test_binary_counts_metrics_losses as test_poisoned_seg_eval  # noqa: E402
from test_eval_metrics_gpu import test_multiclass_all_widths as test_poisoned_seg_eval_mc  # noqa: E402
from test_eval_metrics_gpu import test_head_mse_eval_matches_head_and_mse as test_poisoned_head_mse_eval  # noqa: E402
from test_variants_gpu import test_weighted_mse_and_charbonnier_kernels_match_oracle as test_poisoned_roi_losses  # noqa: E402
from test_region_gpu import test_gather_bit_exact as test_poisoned_region_gather  # noqa: E402
from test_region_gpu import test_blend_with_per_tile_constants as test_poisoned_region_blend  # noqa: E402
