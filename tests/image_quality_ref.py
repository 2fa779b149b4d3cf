"""The image-quality metrics of stain2stain_amd.image_metrics restated in fp64 torch on the CPU: the ground truth of
tests/test_image_metrics_*.py.  (skimage's ``structural_similarity(gaussian_weights=True,
use_sample_covariance=False)`` and torchmetrics define SSIM the same way; neither is imported.)

  mse = mean (a - b)^2, mae = mean |a - b|, psnr = 10 log10(L^2 / mse) (+inf at mse == 0), per sample over all channels
  ssim: 11 x 11 separable Gaussian window (sigma 1.5, normalised), C1 = (k1 L)^2, C2 = (k2 L)^2, biased local moments,
        only positions whose window lies inside the image, mean over channels and positions

``network_to_image`` is the loaders' conversion from the network's range.  It is part of the definition of the input,
not of the metric, and it is an fp32 expression in the product (x * 0.5 exact, + 0.5 rounded once, * 255 rounded once --
the reference's save conversion on fp32 tensors), so it is evaluated in fp32 here as well; everything after it is fp64."""
import math

import torch
import torch.nn.functional as F


def gaussian_window(window=11, sigma=1.5):
    r = window // 2
    x = torch.arange(window, dtype=torch.float64) - r
    w = torch.exp(-(x * x) / (2.0 * sigma * sigma))
    return w / w.sum()


def network_to_image(x, quantize):
    """fp32 [.] in the network's range -> (fp64 image, L)."""
    u = x.detach().cpu().float() * 0.5 + 0.5
    if quantize:
        return (u * 255.0).clamp(0.0, 255.0).trunc().double(), 255.0
    return u.clamp(0.0, 1.0).double(), 1.0


def u8_to_image(u8):
    """uint8 [B, H, W, 3] (or [H, W, 3]) -> (fp64 [B, 3, H, W], 255)."""
    if u8.dim() == 3:
        u8 = u8.unsqueeze(0)
    return u8.detach().cpu().permute(0, 3, 1, 2).double().contiguous(), 255.0


def ssim_map(a, b, L, window=11, sigma=1.5, k1=0.01, k2=0.03):
    """fp64 [B, C, H, W] pairs -> the SSIM value at every valid position, [B, C, H - window + 1, W - window + 1]."""
    a, b = a.double(), b.double()
    B, C, H, W = a.shape
    g = gaussian_window(window, sigma)
    kh, kv = g.view(1, 1, 1, window), g.view(1, 1, window, 1)

    def blur(x):
        return F.conv2d(F.conv2d(x.reshape(B * C, 1, H, W), kh), kv).reshape(B, C, H - window + 1, W - window + 1)

    c1, c2 = (k1 * L) ** 2, (k2 * L) ** 2
    mu_a, mu_b = blur(a), blur(b)
    va, vb, cov = blur(a * a) - mu_a * mu_a, blur(b * b) - mu_b * mu_b, blur(a * b) - mu_a * mu_b
    return ((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (va + vb + c2))


def image_quality_ref(a, b, L, window=11, sigma=1.5, k1=0.01, k2=0.03):
    """{"psnr", "ssim", "mae", "mse"}: fp64 [B] each, of fp64 [B, C, H, W] images with data range L."""
    a, b = a.double(), b.double()
    d = a - b
    mse = (d * d).flatten(1).mean(1)
    mae = d.abs().flatten(1).mean(1)
    psnr = torch.where(mse == 0, torch.full_like(mse, math.inf), 10.0 * torch.log10(L * L / mse.clamp_min(1e-300)))
    ssim = ssim_map(a, b, L, window, sigma, k1, k2).flatten(1).mean(1)
    return {"psnr": psnr, "ssim": ssim, "mae": mae, "mse": mse}


def valid_positions(C, H, W, window=11):
    return (H - window + 1) * (W - window + 1) * C
