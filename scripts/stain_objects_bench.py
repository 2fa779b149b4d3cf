"""Measurement for DESIGN.md 3.19: object analysis of the positive mask on the GPU against ``stain_quantify`` alone on the
same data (what the burden costs without the objects) and against what one does without it: ``stain_separate`` ->
threshold -> ``.cpu()`` -> ``scipy.ndimage.label`` + ``bincount`` (the copy included), at 32 x 256^2 uint8 tiles and on
a 4096^2 device region of synthetic plaques (DAB discs on a noisy haematoxylin background).

    python scripts/stain_objects_bench.py [--iters 20] [--region 4096] [--out profiles/objects_bench.json]

Times are HIP-event medians over ``--iters`` calls after a warm-up (the host chain: wall-clock medians, it ends on the
host).  Prints one JSON line and, with ``--out``, writes it there."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stain2stain_amd import region_stain_map, region_stain_objects, stain_objects, stain_quantify, stain_separate  # noqa: E402
from stain2stain_amd.stain_quant import DEFAULT_THRESHOLDS, stain_matrix  # noqa: E402


def plaques(B, H, W, seed, per_mpx=400.0):
    """uint8 [B, H, W, 3] on the host: haematoxylin noise, ``per_mpx`` DAB discs of radius 2..12 per megapixel."""
    rng = np.random.default_rng(seed)
    conc = np.zeros((B, H, W, 3), np.float32)
    conc[..., 0] = rng.uniform(0.05, 0.5, size=(B, H, W))
    conc[..., 1] = np.where(rng.random((B, H, W)) < 0.01, 0.6, 0.02)          # single-pixel speckle
    n = max(1, int(per_mpx * H * W / 1e6))
    for b in range(B):
        for cy, cx, r in zip(rng.uniform(0, H, n), rng.uniform(0, W, n), rng.uniform(2.0, 12.0, n)):
            y0, y1, x0, x1 = max(int(cy - r), 0), min(int(cy + r) + 1, H), max(int(cx - r), 0), min(int(cx + r) + 1, W)
            yy, xx = np.mgrid[y0:y1, x0:x1]
            conc[b, y0:y1, x0:x1, 1][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 0.9
    od = conc.astype(np.float64) @ stain_matrix("hdab").numpy()
    return torch.from_numpy(np.clip(np.rint(255.0 * 10.0 ** (-od)), 0, 255).astype(np.uint8))


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


def wall(fn, iters):
    fn()
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return ms[len(ms) // 2]


def host_chain(u8, stain=1, min_area=1):
    """What one does without this module: concentrations on the GPU, the mask to the host, scipy there."""
    from scipy import ndimage
    c = stain_separate(u8)[:, stain]
    tissue = u8.amin(-1) < 220
    mask = (tissue & (c > DEFAULT_THRESHOLDS[stain])).cpu().numpy()
    counts = []
    for m in mask:
        lab, n = ndimage.label(m, structure=np.ones((3, 3)))
        area = np.bincount(lab.ravel(), minlength=n + 1)[1:]
        counts.append(int((area >= min_area).sum()))
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--region", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda"
    out = {"iters": args.iters}
    tiles = plaques(32, 256, 256, 1).to(dev)
    out["tiles_32x256_stain_objects_ms"] = timed(lambda: stain_objects(tiles, min_area=4, max_objects=64), args.iters)
    out["tiles_32x256_stain_objects_no_table_ms"] = timed(lambda: stain_objects(tiles, min_area=4), args.iters)
    out["tiles_32x256_stain_quantify_ms"] = timed(lambda: stain_quantify(tiles), args.iters)
    out["tiles_32x256_host_chain_ms"] = wall(lambda: host_chain(tiles, min_area=4), max(3, args.iters // 4))
    got = stain_objects(tiles, min_area=4)["count"].tolist()
    out["tiles_32x256_counts_equal_host_chain"] = got == host_chain(tiles, min_area=4)
    out["tiles_32x256_objects_per_tile"] = sum(got) / len(got)
    n = args.region
    it = max(3, args.iters // 4)
    region = plaques(1, n, n, 2)[0].to(dev)
    out[f"region_{n}_stain_objects_ms"] = timed(lambda: region_stain_objects(region, min_area=4, max_objects=4096), it)
    out[f"region_{n}_stain_objects_no_table_ms"] = timed(lambda: region_stain_objects(region, min_area=4), it)
    out[f"region_{n}_stain_map_ms"] = timed(lambda: region_stain_map(region), it)
    out[f"region_{n}_host_chain_ms"] = wall(lambda: host_chain(region[None], min_area=4), 3)
    r = region_stain_objects(region, min_area=4)
    out[f"region_{n}_objects"] = int(r["count"])
    out[f"region_{n}_counts_equal_host_chain"] = [int(r["count"])] == host_chain(region[None], min_area=4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
