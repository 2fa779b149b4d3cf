"""Measurement for DESIGN.md 3.33: the calibration histograms against the quantification pass over the same bytes (the
traffic is the same, 3 B per pixel and image, so the ratio is the cost of the LDS atomics and the flush), on noisy bytes
and on a flat tissue colour (every pixel in one bin per stain: the worst case for same-address LDS atomics), the
threshold rules alone, the pair forms against ``stain_agreement``, and the same histogram composed from torch ops
(``stain_separate`` + a bin computation + ``torch.bincount`` per sample and stain), at 32 x 256^2 and on one large region.

    python scripts/stain_calibrate_bench.py [--iters 20] [--region 8192] [--out profiles/stain_calibrate_bench.json]

Times are HIP-event medians over ``--iters`` calls after a warm-up: whole calls, launches and allocations included.
Prints one JSON line and writes it to ``--out``."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stain2stain_amd import (match_thresholds, region_stain_agreement, region_stain_histogram, region_stain_map,  # noqa: E402
                             region_stain_pair_histogram, stain_agreement, stain_histogram, stain_pair_histogram,
                             stain_quantify, stain_separate, stain_thresholds)


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


def torch_histogram(u8, white=220):
    """stain_histogram of uint8 [B, H, W, 3] from torch ops: every intermediate goes through memory."""
    c = stain_separate(u8)                                                  # fp32 [B, 3, H, W]
    bins = (torch.ceil(c * 1024.0) - 1.0).clamp_(0.0, 4095.0).long()
    tissue = (u8.amin(-1) < white)[:, None].expand_as(bins)
    bins = torch.where(tissue, bins, torch.full_like(bins, 4096)).flatten(2)
    B = u8.shape[0]
    return torch.stack([torch.stack([torch.bincount(bins[n, k], minlength=4097)[:4096] for k in range(3)])
                        for n in range(B)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--region", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "stain_calibrate_bench.json"))
    args = ap.parse_args()
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    B, H, n = 32, 256, args.region
    it, rit = args.iters, max(5, args.iters // 2)
    flat_colour = torch.tensor([97, 74, 93], dtype=torch.uint8)            # a tissue colour: one bin per stain
    u = torch.randint(0, 256, (B, H, H, 3), generator=g, dtype=torch.uint8).to(dev)
    v = torch.randint(0, 256, (B, H, H, 3), generator=g, dtype=torch.uint8).to(dev)
    uf = flat_colour.to(dev).expand(B, H, H, 3).contiguous()
    out = {"shape_batch": [B, H, H], "shape_region": [n, n], "iters": it}

    def put(key, ms, nbytes=None):
        out[key + "_ms"] = round(ms, 5)
        if nbytes:
            out[key + "_GBps"] = round(nbytes / ms / 1e6, 1)

    px = B * H * H
    # (a), (b): the histogram against the quantification pass, noisy and flat
    put("batch_quantify_noisy", timed(lambda: stain_quantify(u), it), 3 * px)
    put("batch_quantify_flat", timed(lambda: stain_quantify(uf), it), 3 * px)
    put("batch_histogram_noisy", timed(lambda: stain_histogram(u), it), 3 * px)
    put("batch_histogram_flat", timed(lambda: stain_histogram(uf), it), 3 * px)
    put("batch_histogram_pooled_noisy", timed(lambda: stain_histogram(u, pool=True), it), 3 * px)
    put("batch_histogram_pooled_flat", timed(lambda: stain_histogram(uf, pool=True), it), 3 * px)
    # (c): the rules alone
    h = stain_histogram(u)
    put("batch_thresholds_96_rows", timed(lambda: stain_thresholds(h), it))
    hp = stain_histogram(u, pool=True)
    put("thresholds_3_rows", timed(lambda: stain_thresholds(hp), it))
    # (d): the pair forms
    put("batch_agreement_noisy", timed(lambda: stain_agreement(u, v), it), 6 * px)
    put("batch_pair_histogram_noisy", timed(lambda: stain_pair_histogram(u, v, target_threshold=205 / 1024), it), 6 * px)
    put("batch_pair_histogram_flat", timed(lambda: stain_pair_histogram(uf, uf, target_threshold=205 / 1024), it), 6 * px)
    p = stain_pair_histogram(u, v, target_threshold=205 / 1024)
    put("batch_match_thresholds_32_owners", timed(lambda: match_thresholds(p), it))
    # (e): the same histogram from torch ops
    put("batch_histogram_torch_ops", timed(lambda: torch_histogram(u), max(3, it // 4)))
    out["torch_ops_equal"] = bool(torch.equal(torch_histogram(u), stain_histogram(u)["hist"]))
    del u, v, uf
    # the region
    r = torch.randint(0, 256, (n, n, 3), generator=g, dtype=torch.uint8).to(dev)
    rf = flat_colour.to(dev).expand(n, n, 3).contiguous()
    rpx = n * n
    put("region_map_noisy", timed(lambda: region_stain_map(r), rit), 3 * rpx)
    put("region_map_flat", timed(lambda: region_stain_map(rf), rit), 3 * rpx)
    put("region_histogram_noisy", timed(lambda: region_stain_histogram(r), rit), 3 * rpx)
    put("region_histogram_flat", timed(lambda: region_stain_histogram(rf), rit), 3 * rpx)
    put("region_agreement", timed(lambda: region_stain_agreement(r, rf), rit), 6 * rpx)
    put("region_pair_histogram_noisy_vs_flat", timed(lambda: region_stain_pair_histogram(r, rf, target_threshold=205 / 1024), rit), 6 * rpx)
    put("region_pair_histogram_flat", timed(lambda: region_stain_pair_histogram(rf, rf, target_threshold=205 / 1024), rit), 6 * rpx)
    put("region_histogram_torch_ops", timed(lambda: torch_histogram(r[None, : n // 4]), 3) * 4)   # a quarter at a time: memory
    for a, b in (("batch_histogram_noisy", "batch_quantify_noisy"), ("batch_histogram_flat", "batch_histogram_noisy"),
                 ("region_histogram_noisy", "region_map_noisy"), ("region_histogram_flat", "region_histogram_noisy"),
                 ("batch_pair_histogram_noisy", "batch_agreement_noisy"), ("region_pair_histogram_flat", "region_agreement"),
                 ("batch_histogram_torch_ops", "batch_histogram_noisy"), ("region_histogram_torch_ops", "region_histogram_noisy")):
        out[f"ratio_{a}_over_{b}"] = round(out[a + "_ms"] / out[b + "_ms"], 3)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
