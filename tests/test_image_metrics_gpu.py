"""The fused image-quality kernels (csrc/image_metrics.hip) against the fp64 restatement of tests/image_quality_ref.py,
on poisoned memory (every ``torch.empty`` and every ``ops._workspace`` slab starts as NaN / 0xFF, as in
tests/test_unwritten_memory_gpu.py), plus the bit equalities the design promises and the project's first direct seam
test.

Tolerances: mse and mae 1e-6 relative (fp64 accumulation; integer operands in the uint8 and quantised
paths); ssim 1e-4 absolute (about 3x the worst deviation of a plain fp32 evaluation of the formula from fp64, 3.6e-5 on a
flat bright image at L = 255); psnr against 10 log10(L^2 / mse) of the kernel's own mse, 1e-4 dB; identical images give
ssim 1, mse 0 and psnr +inf exactly."""
import math

import pytest
import torch

import image_quality_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("psnr", "ssim", "mae", "mse")
KINDS = ("smooth_noise8", "pm1", "flat_bright_pm1", "independent", "identical")


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


def test_poison_is_on():
    from stain2stain_amd import ops
    assert torch.empty(1000, device=DEV).isnan().all()
    assert ops._workspace(torch.device(DEV), 64, "probe").view(torch.float64).isnan().all()


def _levels(kind, B, C, H, W, seed):
    """(pred, target) as fp64 grey levels in [0, 255], integers (the uint8 loader takes them as they are)."""
    g = torch.Generator().manual_seed(seed)
    yy = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    ph = torch.rand((B, C, 1, 1), generator=g, dtype=torch.float64) * 6.28
    smooth = 128 + 60 * torch.sin(yy / 9.0 + ph) * torch.cos(xx / 13.0 - ph) + 30 * torch.sin((xx + yy) / 31.0)
    sign = (torch.randint(0, 2, (B, C, H, W), generator=g) * 2 - 1).double()
    if kind == "smooth_noise8":
        tgt, pred = smooth, smooth + 8.0 * torch.randn((B, C, H, W), generator=g, dtype=torch.float64)
    elif kind == "pm1":
        tgt, pred = smooth, smooth.round() + sign
    elif kind == "flat_bright_pm1":
        tgt = torch.full((B, C, H, W), 240.0, dtype=torch.float64)
        pred = tgt + sign
    elif kind == "independent":
        tgt = torch.rand((B, C, H, W), generator=g, dtype=torch.float64) * 255
        pred = torch.rand((B, C, H, W), generator=g, dtype=torch.float64) * 255
    elif kind == "identical":
        tgt = pred = smooth
    else:
        raise KeyError(kind)
    return pred.clamp(0, 255).round(), tgt.clamp(0, 255).round()


def _network(levels, jitter_seed=None):
    """Grey levels -> fp32 in the network's range; with a seed, a sub-level jitter so that the quantiser has work."""
    if jitter_seed is not None:
        g = torch.Generator().manual_seed(jitter_seed)
        levels = levels + torch.rand(levels.shape, generator=g, dtype=torch.float64) * 0.98
    return (levels / 127.5 - 1.0).float()


def _u8(levels):
    return levels.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _check(got, ref, L, what):
    got = {k: v.detach().cpu().double() for k, v in got.items()}
    for k in KEYS:
        assert got[k].shape == ref[k].shape, (what, k)
    zero = ref["mse"] == 0
    rel = lambda a, b: float(((a - b).abs() / b.abs().clamp_min(1e-300))[~zero].max()) if (~zero).any() else 0.0
    e_mse, e_mae = rel(got["mse"], ref["mse"]), rel(got["mae"], ref["mae"])
    e_ssim = float((got["ssim"] - ref["ssim"]).abs().max())
    own = torch.where(got["mse"] == 0, torch.full_like(got["mse"], math.inf),
                      10.0 * torch.log10(L * L / got["mse"].clamp_min(1e-300)))
    fin = torch.isfinite(own)
    e_psnr = float((got["psnr"] - own)[fin].abs().max()) if fin.any() else 0.0
    print(f"{what}: mse rel {e_mse:.2e} mae rel {e_mae:.2e} ssim abs {e_ssim:.2e} psnr dB {e_psnr:.2e}")
    assert e_mse <= 1e-6 and e_mae <= 1e-6, what
    assert e_ssim <= 1e-4, what
    assert e_psnr <= 1e-4 and torch.equal(torch.isfinite(got["psnr"]), fin), what
    if zero.any():
        assert (got["mse"][zero] == 0).all() and (got["mae"][zero] == 0).all() and (got["ssim"][zero] == 1).all()
        assert (got["psnr"][zero] == math.inf).all()


# every shape of the list with every B and C of the list somewhere; B = 32 at 256 x 256 is the benchmark size
SHAPES = [(32, 3, 256, 256), (1, 1, 256, 256), (3, 3, 96, 80), (1, 4, 96, 80), (3, 1, 11, 11), (1, 3, 11, 11),
          (32, 4, 11, 11), (3, 4, 37, 53), (1, 1, 37, 53), (3, 3, 37, 53)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,C,H,W", SHAPES)
@pytest.mark.parametrize("quantize", [True, False])
def test_parity_fp32(kind, B, C, H, W, quantize):
    from stain2stain_amd import image_quality
    pl, tl = _levels(kind, B, C, H, W, seed=B * 1000 + C * 100 + H)
    same = kind == "identical"
    x, y = _network(pl, 11), _network(tl, 11 if same else 12)
    got = image_quality(x.to(DEV), y.to(DEV), quantize=quantize)
    (a, L), (b, _) = R.network_to_image(x, quantize), R.network_to_image(y, quantize)
    for v in got.values():
        assert v.dtype == torch.float32 and tuple(v.shape) == (B,) and v.is_cuda
    _check(got, R.image_quality_ref(a, b, L), L, f"fp32 q={quantize} {kind} {B}x{C}x{H}x{W}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,H,W", [(32, 256, 256), (3, 96, 80), (1, 11, 11), (3, 37, 53), (1, 37, 53)])
def test_parity_uint8(kind, B, H, W):
    from stain2stain_amd import image_quality
    pl, tl = _levels(kind, B, 3, H, W, seed=B * 77 + H)
    got = image_quality(_u8(pl).to(DEV), _u8(tl).to(DEV))
    _check(got, R.image_quality_ref(pl, tl, 255.0), 255.0, f"uint8 {kind} {B}x{H}x{W}")


@pytest.mark.parametrize("window,sigma", [(7, 1.0), (3, 0.8), (1, 1.5), (9, 1.5)])
def test_parity_other_windows(window, sigma):
    from stain2stain_amd import image_quality
    pl, tl = _levels("smooth_noise8", 2, 3, 45, 70, seed=window)
    got = image_quality(_u8(pl).to(DEV), _u8(tl).to(DEV), window=window, sigma=sigma, k1=0.02, k2=0.05)
    _check(got, R.image_quality_ref(pl, tl, 255.0, window, sigma, 0.02, 0.05), 255.0, f"window {window}")


def _equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in KEYS)


def test_repeat_and_batch_independence():
    from stain2stain_amd import image_quality
    pl, tl = _levels("smooth_noise8", 5, 3, 70, 90, seed=5)
    x, y = _network(pl, 1).to(DEV), _network(tl, 2).to(DEV)
    for q in (True, False):
        full = image_quality(x, y, quantize=q)
        assert _equal(full, image_quality(x, y, quantize=q))
        for i in (0, 3, 4):
            one = image_quality(x[i:i + 1], y[i:i + 1], quantize=q)
            assert all(torch.equal(one[k][0], full[k][i]) for k in KEYS)
    pu, tu = _u8(pl).to(DEV), _u8(tl).to(DEV)
    full = image_quality(pu, tu)
    assert _equal(full, image_quality(pu, tu))
    one = image_quality(pu[2:3], tu[2:3])
    assert all(torch.equal(one[k][0], full[k][2]) for k in KEYS)


def test_quantised_fp32_equals_uint8_loader():
    from stain2stain_amd import image_quality
    pl, tl = _levels("smooth_noise8", 3, 3, 96, 80, seed=9)
    x, y = _network(pl, 3).to(DEV), _network(tl, 4).to(DEV)
    conv = lambda v: ((v * 0.5 + 0.5) * 255).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert _equal(image_quality(x, y, quantize=True), image_quality(conv(x), conv(y)))


def _region_pair(H, W, seed):
    pl, tl = _levels("smooth_noise8", 1, 3, H, W, seed=seed)
    return _u8(pl)[0], _u8(tl)[0]


def test_region_bands_and_host_input():
    from stain2stain_amd import image_quality, region_quality
    H, W = 301, 203
    p, t = _region_pair(H, W, 21)
    base = region_quality(p.to(DEV), t.to(DEV))
    for v in base.values():
        assert v.dim() == 0 and v.is_cuda and v.dtype == torch.float32
    _check({k: v.reshape(1) for k, v in base.items()},
           R.image_quality_ref(*[R.u8_to_image(v)[0] for v in (p, t)], 255.0), 255.0, "region")
    tile = image_quality(p[None].to(DEV), t[None].to(DEV))
    assert all(torch.equal(tile[k][0], base[k]) for k in KEYS)
    for band_rows in (42, 75, 138):
        assert _equal(base, region_quality(p.to(DEV), t.to(DEV), band_rows=band_rows)), band_rows
        assert region_quality.last_stats["bands"] > 1
        assert _equal(base, region_quality(p, t, band_rows=band_rows)), band_rows            # host input
        assert region_quality.last_stats["band_rows"] <= band_rows
        assert region_quality.last_stats["band_bytes"] == 2 * region_quality.last_stats["band_rows"] * W * 3
    assert _equal(base, region_quality(p, t))
    assert _equal(base, region_quality(p.to(DEV), t, band_rows=75))                          # one of each


def test_pitched_crop_equals_contiguous_copy():
    from stain2stain_amd import image_quality, region_quality
    p, t = _region_pair(260, 300, 22)
    for src in (lambda v: v.to(DEV), lambda v: v):
        cp, ct = src(p)[13:230, 7:250], src(t)[13:230, 7:250]
        assert not cp.is_contiguous()
        assert _equal(region_quality(cp, ct, band_rows=74), region_quality(cp.contiguous(), ct.contiguous()))
    pl, tl = _levels("independent", 4, 3, 64, 72, seed=23)
    pu, tu = _u8(pl).to(DEV), _u8(tl).to(DEV)
    vp, vt = pu[1:4, 5:50, 3:61], tu[1:4, 5:50, 3:61]
    assert not vp.is_contiguous()
    assert _equal(image_quality(vp, vt), image_quality(vp.contiguous(), vt.contiguous()))


def test_translate_region_leaves_no_seams():
    """The identity sampler through the tiled translation, scored against the input itself, on a region whose size is no
    multiple of the tile (the last tile row and column are flush with the edge and overlap their neighbours more).

    A black / white image: its normalised values are -1 and +1, so every feathered product w * v and every sum of them
    is exact in fp32, the blend returns exactly -1 / +1 and the save conversion exactly 0 / 255 -- any seam, any
    misplaced or mis-weighted tile would show: ssim 1 and mse 0 exactly.  On general grey levels an exact identity puts
    every pixel on the knife edge of the reference's truncating save conversion (``(u / 255) * 255`` one ulp low
    truncates to u - 1), so there the round trip may lose one level per pixel and nothing more: mae <= 1.

    Grey levels without the knife edge: a sampler that adds half a grey level (1/255 in the network's range) is the
    identity on uint8 images under the truncating conversion -- level u becomes u + 0.5, far from both neighbours, 255
    is clamped -- and an ulp of blending error cannot move it.  The tiled output then equals the input pixel for
    pixel, and a blend that is off by half a level anywhere is caught: ssim 1 and mse 0 exactly, no tolerance."""
    from stain2stain_amd import region_quality, translate_region
    g = torch.Generator().manual_seed(31)
    H, W = 203, 150
    bw = (torch.randint(0, 2, (H, W, 3), generator=g) * 255).to(torch.uint8)
    # low-frequency blobs as well, so that tile-sized structure exists
    bw[40:120, 30:100] = 255
    bw[90:160, 80:140, 1] = 0
    for img in (bw.to(DEV), bw):
        out = translate_region(img, lambda x: x.clone(), tile=64, overlap=16, batch=4)
        q = region_quality(out, img)
        assert float(q["ssim"]) == 1.0 and float(q["mse"]) == 0.0 and float(q["mae"]) == 0.0
        assert float(q["psnr"]) == math.inf
    grey = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
    out = translate_region(grey, lambda x: x.clone(), tile=64, overlap=16, batch=4)
    q = region_quality(out, grey)
    print(f"grey identity round trip: mae {float(q['mae']):.4f} ssim {float(q['ssim']):.6f}")
    assert float(q["mae"]) <= 1.0 and float(q["mse"]) <= 1.0
    for img in (grey, grey.cpu()):
        out = translate_region(img, lambda x: x + 1.0 / 255.0, tile=64, overlap=16, batch=4)
        assert torch.equal(out, img)
        q = region_quality(out, img)
        assert float(q["ssim"]) == 1.0 and float(q["mse"]) == 0.0 and float(q["mae"]) == 0.0
        assert float(q["psnr"]) == math.inf


def test_capture_and_replay():
    from stain2stain_amd import image_quality, ops
    pl, tl = _levels("smooth_noise8", 4, 3, 64, 48, seed=41)
    x, y = _network(pl, 5).to(DEV), _network(tl, 6).to(DEV)
    sx, sy = torch.zeros_like(x), torch.zeros_like(y)
    image_quality(sx, sy)                                           # warm-up: the workspace exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.capture_graph(graph):
        out = image_quality(sx, sy)
    try:
        for a, b in ((x, y), (y.flip(0), x)):
            sx.copy_(a)
            sy.copy_(b)
            graph.replay()
            assert _equal(out, image_quality(a, b))
    finally:
        del graph
