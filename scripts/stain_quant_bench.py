"""Measurement for DESIGN.md 3.17: the fused stain-quantification pass against the same definition composed from torch
ops (a table gather, a 3 x 3 matmul, comparisons and reductions: every intermediate goes through memory), at 32 x 256^2
and on a large device region, with random bytes (the worst case for the table reads from LDS: 64 lanes, 64 different
entries) and with smooth images (neighbouring lanes read the same entries).

    python scripts/stain_quant_bench.py [--only fused|torch|region] [--iters 20] [--region 8192]

Times are HIP-event medians over ``--iters`` calls after a warm-up; GB/s are against the algorithmic traffic, 3 B per
pixel and image for uint8 and 12 B for fp32.  Run it under ``rocprofv3 --kernel-trace --stats`` with ``--only fused
--iters 3`` to read the kernel times.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stain2stain_amd import region_stain_agreement, region_stain_map, stain_agreement, stain_quantify, stain_separate  # noqa: E402
from stain2stain_amd.stain_quant import DEFAULT_THRESHOLDS, od_table, unmix_matrix  # noqa: E402


def torch_quantify(u8, white=220):
    """stain_quantify of uint8 [B, H, W, 3] from torch ops alone (fp32; the matmul may contract, so counts can differ by
    pixels that sit on a threshold)."""
    dev = u8.device
    od = od_table().to(dev)[u8.long()]
    c = od @ unmix_matrix("hdab").to(dev)
    tissue = u8.amin(-1) < white
    pos = tissue[..., None] & (c > torch.tensor(DEFAULT_THRESHOLDS, device=dev))
    n_t, n_p = tissue.flatten(1).sum(1), pos.flatten(1, 2).sum(1)
    od_sum = (c.clamp_min(0).double() * tissue[..., None]).flatten(1, 2).sum(1)
    den = n_t.clamp_min(1)[:, None]
    return {"tissue": n_t, "positive": n_p, "od_sum": od_sum, "burden": n_p / den, "mean_od": od_sum / den}


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


def smooth_u8(shape, dev):
    """Slowly varying bytes: the 64 lanes of a wave read a handful of table entries."""
    *lead, H, W, _ = shape
    yy = torch.arange(H, device=dev).view(H, 1, 1).float()
    xx = torch.arange(W, device=dev).view(1, W, 1).float()
    ch = torch.arange(3, device=dev).view(1, 1, 3).float()
    img = (128 + 100 * torch.sin(yy / 97.0 + ch) * torch.cos(xx / 131.0 - ch)).to(torch.uint8)
    return img.expand(*lead, H, W, 3).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["fused", "torch", "region"], default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--region", type=int, default=8192)
    args = ap.parse_args()
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    B, H = 32, 256
    u = torch.randint(0, 256, (B, H, H, 3), generator=g, dtype=torch.uint8).to(dev)
    v = torch.randint(0, 256, (B, H, H, 3), generator=g, dtype=torch.uint8).to(dev)
    us = smooth_u8((B, H, H, 3), dev)
    x = (u.permute(0, 3, 1, 2).float() / 127.5 - 1.0).contiguous()
    y = (v.permute(0, 3, 1, 2).float() / 127.5 - 1.0).contiguous()
    px = B * H * H
    out = {}

    def rate(key, ms, nbytes):
        out[key + "_ms"] = ms
        out[key + "_GBps"] = nbytes / ms / 1e6

    if args.only in (None, "fused"):
        rate("fused_u8_random", timed(lambda: stain_quantify(u), args.iters), 3 * px)
        rate("fused_u8_smooth", timed(lambda: stain_quantify(us), args.iters), 3 * px)
        rate("fused_u8_pair", timed(lambda: stain_agreement(u, v), args.iters), 6 * px)
        rate("fused_f32", timed(lambda: stain_quantify(x), args.iters), 12 * px)
        rate("fused_f32_pair", timed(lambda: stain_agreement(x, y), args.iters), 24 * px)
        rate("separate_u8", timed(lambda: stain_separate(u), args.iters), 15 * px)
    if args.only in (None, "torch"):
        out["torch_u8_ms"] = timed(lambda: torch_quantify(u), args.iters)
        a, b = stain_quantify(u), torch_quantify(u)
        out["torch_vs_fused_tissue_equal"] = bool(torch.equal(a["tissue"], b["tissue"]))
        out["torch_vs_fused_positive_maxdiff"] = int((a["positive"] - b["positive"]).abs().max())
    if args.only in (None, "region"):
        n = args.region
        it = max(3, args.iters // 4)
        p = torch.randint(0, 256, (n, n, 3), generator=g, dtype=torch.uint8).to(dev)
        rate(f"region_{n}_map_random", timed(lambda: region_stain_map(p), it), 3 * n * n)
        ps = smooth_u8((n, n, 3), dev)
        rate(f"region_{n}_map_smooth", timed(lambda: region_stain_map(ps), it), 3 * n * n)
        rate(f"region_{n}_pair", timed(lambda: region_stain_agreement(p, ps), it), 6 * n * n)
        out[f"region_{n}_torch_ms"] = timed(lambda: torch_quantify(p[None, : n // 4]), 3) * 4   # a quarter at a time: memory
    print(json.dumps(out))


if __name__ == "__main__":
    main()
