"""Throw-away measurement for DESIGN.md 3.15: the fused image-quality pass against the same metrics built from grouped
``F.conv2d`` calls (all a user had before: five blurred maps per channel through memory, two separable convolutions
each), and ``region_quality`` on a large device region.

    python scripts/image_quality_bench.py [--only fused|conv2d|region] [--iters 20] [--region 8192]

Times are HIP-event medians over ``--iters`` calls after a warm-up; run it under ``rocprofv3 --kernel-trace --stats``
with ``--only fused --iters 3`` to count launches and read the kernel times.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stain2stain_amd import image_quality, region_quality  # noqa: E402
from stain2stain_amd.image_metrics import gaussian_taps  # noqa: E402


def conv2d_quality(x, y, quantize=True):
    """The metrics from torch ops alone (fp32): the launch count is what it is."""
    u, v = x * 0.5 + 0.5, y * 0.5 + 0.5
    if quantize:
        a, b, L = (u * 255).clamp(0, 255).trunc(), (v * 255).clamp(0, 255).trunc(), 255.0
    else:
        a, b, L = u.clamp(0, 1), v.clamp(0, 1), 1.0
    B, C, H, W = a.shape
    g = torch.tensor(gaussian_taps(), dtype=torch.float32, device=a.device)
    kh, kv = g.view(1, 1, 1, -1).repeat(C, 1, 1, 1), g.view(1, 1, -1, 1).repeat(C, 1, 1, 1)
    blur = lambda t: F.conv2d(F.conv2d(t, kh, groups=C), kv, groups=C)
    ma, mb = blur(a), blur(b)
    va, vb, cov = blur(a * a) - ma * ma, blur(b * b) - mb * mb, blur(a * b) - ma * mb
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    ssim = (((2 * ma * mb + c1) * (2 * cov + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))).flatten(1).mean(1)
    d = a - b
    mse = (d * d).flatten(1).mean(1)
    return {"psnr": 10 * torch.log10(L * L / mse), "ssim": ssim, "mae": d.abs().flatten(1).mean(1), "mse": mse}


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["fused", "conv2d", "region"], default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--region", type=int, default=8192)
    args = ap.parse_args()
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(32, 3, 256, 256, generator=g) * 2 - 1).to(dev)
    y = (x.cpu() + 0.1 * torch.randn(32, 3, 256, 256, generator=g)).to(dev)
    conv = lambda v: ((v * 0.5 + 0.5) * 255).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    xu, yu = conv(x), conv(y)
    out = {}
    if args.only in (None, "fused"):
        out["fused_fp32_quantize_ms"] = timed(lambda: image_quality(x, y, quantize=True), args.iters)
        out["fused_fp32_unit_ms"] = timed(lambda: image_quality(x, y, quantize=False), args.iters)
        out["fused_uint8_ms"] = timed(lambda: image_quality(xu, yu), args.iters)
    if args.only in (None, "conv2d"):
        out["conv2d_fp32_quantize_ms"] = timed(lambda: conv2d_quality(x, y, True), args.iters)
        out["conv2d_fp32_unit_ms"] = timed(lambda: conv2d_quality(x, y, False), args.iters)
        a, b = image_quality(x, y), conv2d_quality(x, y)
        out["conv2d_vs_fused_ssim_maxdiff"] = float((a["ssim"] - b["ssim"]).abs().max())
    if args.only in (None, "region"):
        n = args.region
        p = torch.randint(0, 256, (n, n, 3), generator=g, dtype=torch.uint8).to(dev)
        t = (p.int() + torch.randint(-3, 4, (n, n, 3), device=dev)).clamp(0, 255).to(torch.uint8)
        out[f"region_{n}_device_ms"] = timed(lambda: region_quality(p, t), max(3, args.iters // 4))
        out[f"region_{n}_bytes"] = 2 * n * n * 3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
