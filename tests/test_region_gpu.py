"""Tiled whole-region translation (stain2stain_amd.region, csrc/region.hip) on the GPU: the gather is bit-exact against
numpy, the feathered blend against a float64 restatement in plan order, exact tilings against euler_generate on the same
crops, the streaming ring and the host staging against the in-memory result."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- numpy / float64 restatements -----------------------------------------------------------------------------------
def _norm(u8):
    return (u8.astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)


def _gather_ref(img, origins, T):
    """img uint8 [H, W, 3] -> fp32 [B, 3, T, T]: numpy.pad(mode="reflect") + crop + to_tensor + Normalize."""
    H, W, _ = img.shape
    pad = np.pad(img, ((0, max(0, T - H)), (0, max(0, T - W)), (0, 0)), mode="reflect")
    return np.stack([_norm(pad[y:y + T, x:x + T]).transpose(2, 0, 1) for y, x in origins])


def _axis_w(T, overlap):
    i = np.arange(T, dtype=np.float64)
    if overlap == 0:
        return np.ones(T)
    return np.minimum(1.0, np.minimum((i + 0.5) / overlap, (T - i - 0.5) / overlap))


def _blend_ref(outs, origins, H, W, T, overlap):
    """float64 feathered blend of per-tile outputs [N, C, T, T] (plan order) -> [H, W, C]."""
    w2 = np.outer(_axis_w(T, overlap), _axis_w(T, overlap))
    C = outs.shape[1]
    acc = np.zeros((H, W, C))
    ws = np.zeros((H, W, 1))
    for v, (y, x) in zip(outs.astype(np.float64), origins):
        h, w = min(T, H - y), min(T, W - x)
        acc[y:y + h, x:x + w] += w2[:h, :w, None] * v.transpose(1, 2, 0)[:h, :w]
        ws[y:y + h, x:x + w] += w2[:h, :w, None]
    return acc / ws


def _u8_of(x):
    """The reference's save conversion in fp32: np.clip(denormalize(x) * 255, 0, 255).astype(np.uint8)."""
    x = np.asarray(x, dtype=np.float32)
    return np.clip((x * np.float32(0.5) + np.float32(0.5)) * np.float32(255.0), 0, 255).astype(np.uint8)


def _check_u8(got, ref64):
    pre = np.clip((ref64 * 0.5 + 0.5) * 255.0, 0, 255)
    want = np.trunc(pre).astype(np.int64)
    diff = np.abs(got.astype(np.int64) - want)
    near = np.abs(pre - np.round(pre)) <= 1e-3
    assert diff.max() <= 1 and not np.any((diff > 0) & ~near)


def _img(H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)


class _ConstSampler:
    """Input plus a per-tile constant (tile p of the plan gets 0.0005 * (p % 97)), so seams would show; records
    every output."""

    def __init__(self, batch):
        self.batch, self.calls = batch, []

    def __call__(self, x):
        k = len(self.calls) * self.batch + torch.arange(x.shape[0], device=x.device)
        out = x + (0.0005 * (k % 97)).float().view(-1, 1, 1, 1)
        self.calls.append(out.clone())
        return out

    def outputs(self, n):
        return torch.cat(self.calls)[:n].cpu().numpy()


def _net(precision):
    from stain2stain_amd import FlowUNet
    torch.manual_seed(1984)
    return FlowUNet(3, [16, 32, 64], 3, 32, precision=precision).to(DEV)


def _euler_by_batches(net, tiles, batch, steps):
    """euler_generate on plan-ordered tiles in batches of `batch`, the last padded by repeating its last tile."""
    from stain2stain_amd import euler_generate
    outs = []
    for p0 in range(0, tiles.shape[0], batch):
        b = tiles[p0:p0 + batch]
        if b.shape[0] < batch:
            b = torch.cat([b, b[-1:].expand(batch - b.shape[0], -1, -1, -1)])
        outs.append(euler_generate(net, b, steps, graph=True)[:min(batch, tiles.shape[0] - p0)])
    return torch.cat(outs)


# ---- 1. gather ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,T,overlap", [(37, 45, 64, 0), (1, 100, 16, 4), (133, 71, 32, 5), (64, 64, 64, 0),
                                           (2, 1, 16, 0), (250, 300, 64, 16)])
def test_gather_bit_exact(H, W, T, overlap):
    from stain2stain_amd import ops
    from stain2stain_amd.region import plan_tiles
    img = _img(H, W, 1)
    plan = plan_tiles(H, W, T, overlap)
    out = torch.empty((plan.shape[0], 3, T, T), device=DEV)
    ops.region_gather(img.to(DEV), 0, H, W, plan.to(DEV), T, out)
    assert np.array_equal(out.cpu().numpy(), _gather_ref(img.numpy(), plan.tolist(), T))


@pytest.mark.parametrize("y0,x0", [(13, 7), (4, 8)])          # misaligned and 4-byte aligned row starts
def test_gather_crop_view_and_band(y0, x0):
    from stain2stain_amd import ops
    from stain2stain_amd.region import plan_tiles
    big = _img(260, 320, 2).to(DEV)
    view = big[y0:y0 + 181, x0:x0 + 229]                        # row pitch 960 bytes > 3 W
    H, W, T = 181, 229, 32
    ref_img = view.cpu().numpy()
    plan = plan_tiles(H, W, T, 6)
    out = torch.empty((plan.shape[0], 3, T, T), device=DEV)
    ops.region_gather(view, 0, H, W, plan.to(DEV), T, out)
    assert np.array_equal(out.cpu().numpy(), _gather_ref(ref_img, plan.tolist(), T))
    # a band holding image rows [r0, r1): the tiles whose rows lie inside it
    r0, r1 = 52, 140
    sel = plan[(plan[:, 0] >= r0) & (plan[:, 0] + T <= r1)]
    out = torch.empty((sel.shape[0], 3, T, T), device=DEV)
    ops.region_gather(view[r0:r1], r0, H, W, sel.to(DEV), T, out)
    assert np.array_equal(out.cpu().numpy(), _gather_ref(ref_img, sel.tolist(), T))


# ---- 2, 3, 6. blend and finalise ------------------------------------------------------------------------------------
def _check_blend(H, W, T, overlap, batch, on_gpu=True):
    from stain2stain_amd import translate_region
    from stain2stain_amd.region import plan_tiles
    img = _img(H, W, 3)
    s = _ConstSampler(batch)
    u8, f = translate_region(img.to(DEV) if on_gpu else img, s, tile=T, overlap=overlap, batch=batch,
                             return_float=True)
    plan = plan_tiles(H, W, T, overlap)
    ref = _blend_ref(s.outputs(plan.shape[0]), plan.tolist(), H, W, T, overlap)
    assert u8.shape == (H, W, 3) and u8.dtype == torch.uint8 and f.shape == (H, W, 3)
    assert np.abs(f.cpu().numpy() - ref).max() <= 1e-6
    _check_u8(u8.cpu().numpy(), ref)
    return translate_region.last_stats


@pytest.mark.parametrize("H,W,T,overlap,batch", [(150, 130, 32, 8, 4), (64, 64, 64, 16, 2), (37, 45, 64, 16, 3),
                                                 (57, 40, 16, 6, 7), (80, 80, 32, 0, 5)])
def test_blend_with_per_tile_constants(H, W, T, overlap, batch):
    st = _check_blend(H, W, T, overlap, batch)
    from stain2stain_amd.region import plan_tiles
    n = plan_tiles(H, W, T, overlap).shape[0]
    assert st["tiles"] == n and st["batches"] == -(-n // batch) and st["channels"] == 3


def test_identity_sampler_returns_the_normalised_input():
    from stain2stain_amd import translate_region
    img = _img(211, 173, 4)
    u8, f = translate_region(img.to(DEV), lambda x: x.clone(), tile=64, overlap=24, batch=3, return_float=True)
    assert np.abs(f.cpu().numpy() - _norm(img.numpy())).max() <= 1e-6
    _check_u8(u8.cpu().numpy(), _norm(img.numpy()).astype(np.float64))


def test_streaming_ring_is_independent_of_height():
    stats = [_check_blend(H, 150, 64, 16, 5) for H in (1100, 700)]
    for st in stats:
        assert st["band_rows"] < 700
        assert st["accumulator_bytes"] <= st["band_rows"] * 150 * (3 + 1) * 4
    assert stats[0]["band_rows"] == stats[1]["band_rows"]
    assert stats[0]["accumulator_bytes"] == stats[1]["accumulator_bytes"]


# ---- 4, 5. the real network -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_exact_tiling_matches_euler_generate(precision):
    from stain2stain_amd import euler_generate, translate_region
    from stain2stain_amd.region import plan_tiles
    net = _net(precision)
    H, W, T, batch, steps = 96, 64, 32, 4, 4
    img = _img(H, W, 5)
    u8, f = translate_region(img.to(DEV), lambda x: euler_generate(net, x, steps, graph=True), tile=T, overlap=0,
                             batch=batch, return_float=True)
    plan = plan_tiles(H, W, T, 0)
    tiles = torch.from_numpy(_gather_ref(img.numpy(), plan.tolist(), T)).to(DEV)
    ref = _euler_by_batches(net, tiles, batch, steps).cpu().numpy()
    side = np.zeros((H, W, 3), np.float32)
    for v, (y, x) in zip(ref, plan.tolist()):
        side[y:y + T, x:x + T] = v.transpose(1, 2, 0)
    assert np.array_equal(f.cpu().numpy(), side)
    assert np.array_equal(u8.cpu().numpy(), _u8_of(side))


def test_single_cover_pixels_match_their_tile():
    from stain2stain_amd import euler_generate, translate_region
    from stain2stain_amd.region import plan_tiles
    net = _net("fp32")
    H, W, T, ov, batch, steps = 80, 80, 32, 8, 4, 3
    img = _img(H, W, 6)
    u8, f = translate_region(img.to(DEV), lambda x: euler_generate(net, x, steps, graph=True), tile=T, overlap=ov,
                             batch=batch, return_float=True)
    plan = plan_tiles(H, W, T, ov).tolist()
    tiles = torch.from_numpy(_gather_ref(img.numpy(), plan, T)).to(DEV)
    ref = _euler_by_batches(net, tiles, batch, steps).cpu().numpy()
    cover = np.zeros((H, W), np.int64)
    owner = np.full((H, W, 3), np.nan, np.float32)
    for v, (y, x) in zip(ref, plan):
        cover[y:y + T, x:x + T] += 1
        owner[y:y + T, x:x + T] = v.transpose(1, 2, 0)
    one = cover == 1
    assert one.sum() > 0.3 * H * W
    assert np.abs(f.cpu().numpy()[one] - owner[one]).max() <= 1e-6


# ---- 7, 8. host input and determinism -------------------------------------------------------------------------------
def test_host_input_matches_device_input():
    from stain2stain_amd import euler_generate, translate_region
    net = _net("bf16")
    big = _img(400, 120, 7)
    img = big[3:330, 5:105]                                    # a crop view: row pitch 360 bytes
    run = lambda im: translate_region(im, lambda x: euler_generate(net, x, 2, graph=True), tile=32, overlap=8,
                                      batch=3, return_float=True)
    hu8, hf = run(img)
    assert not hu8.is_cuda and not hf.is_cuda
    du8, df = run(img.to(DEV))
    assert du8.is_cuda
    assert torch.equal(hu8, du8.cpu()) and torch.equal(hf, df.cpu())
    # the synthetic sampler through the host path, against the float64 restatement
    _check_blend(300, 90, 32, 8, 3, on_gpu=False)


def test_two_calls_are_bit_equal():
    from stain2stain_amd import euler_generate, translate_region
    net = _net("bf16")
    img = _img(150, 110, 8).to(DEV)
    run = lambda: translate_region(img, lambda x: euler_generate(net, x, 3, graph=True), tile=32, overlap=12,
                                   batch=5, return_float=True)
    a, b = run(), run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 9. multitask ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_classes", [None, 3])
def test_multitask_sampler(num_classes):
    from stain2stain_amd import (FlowMatchingDecoder, MultiTaskFlowMatchingModule, SegmentationDecoder, SharedEncoder,
                                 SolverConfig, multitask_sampler, translate_region)
    torch.manual_seed(1984)
    enc = SharedEncoder(3, [16, 32], precision="fp32")
    fdec = FlowMatchingDecoder(32, [16], 3, 32, precision="fp32")
    sdec = SegmentationDecoder(32, [16], 1 if num_classes is None else num_classes, precision="fp32")
    mod = MultiTaskFlowMatchingModule(enc, fdec, sdec, time_emb_dim=32, num_classes=num_classes,
                                      solver=SolverConfig("euler")).to(DEV)
    Cm = 1 if num_classes is None else num_classes
    img = _img(70, 90, 9)
    u8, probs = translate_region(img.to(DEV), multitask_sampler(mod, 3), tile=32, overlap=8, batch=4)
    assert u8.shape == (70, 90, 3) and probs.shape == (70, 90, Cm) and probs.dtype == torch.float32
    assert float(probs.min()) >= 0.0 and float(probs.max()) <= 1.0
    if num_classes is not None:
        assert float((probs.sum(-1) - 1).abs().max()) <= 1e-5
    # one tile: the module's own outputs for that tile
    one = _img(32, 32, 10)
    u8, probs, f = translate_region(one.to(DEV), multitask_sampler(mod, 3), tile=32, overlap=8, batch=2,
                                    return_float=True)
    x = torch.from_numpy(_gather_ref(one.numpy(), [(0, 0)], 32)).to(DEV).expand(2, -1, -1, -1).contiguous()
    gen, _ = mod.generate(x, num_steps=3, method="euler")           # the same batch shape as the sampler's calls
    with torch.no_grad():
        logits = mod.forward_segmentation(x)
    p = torch.sigmoid(logits) if num_classes is None else torch.softmax(logits, dim=1)
    assert float((f - gen[0].permute(1, 2, 0)).abs().max()) <= 1e-6
    assert float((probs - p[0].permute(1, 2, 0)).abs().max()) <= 1e-6


# ---- 10. rejections -------------------------------------------------------------------------------------------------
def test_rejections():
    from stain2stain_amd import translate_region
    img = _img(40, 40, 11).to(DEV)
    ident = lambda x: x.clone()
    with pytest.raises(ValueError):
        translate_region(img.float(), ident, tile=32, overlap=8, batch=2)
    with pytest.raises(ValueError):
        translate_region(torch.zeros((40, 40, 4), dtype=torch.uint8, device=DEV), ident, tile=32, overlap=8, batch=2)
    with pytest.raises(ValueError):
        translate_region(img[..., :2], ident, tile=32, overlap=8, batch=2)
    with pytest.raises(ValueError):
        translate_region(img, lambda x: x[:, :, :16].clone(), tile=32, overlap=8, batch=2)
    with pytest.raises(ValueError):
        translate_region(img, lambda x: x[:1].clone(), tile=32, overlap=8, batch=2)
    with pytest.raises(ValueError):
        translate_region(img, lambda x: x.double(), tile=32, overlap=8, batch=2)
    with pytest.raises(ValueError):
        translate_region(img, lambda x: (x.clone(), torch.zeros((2, 6, 32, 32), device=DEV)), tile=32, overlap=8,
                         batch=2)
    with pytest.raises(ValueError):
        translate_region(img, ident, tile=32, overlap=32, batch=2)
