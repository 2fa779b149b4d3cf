"""Measurement for DESIGN.md 3.24: mask morphology and boundary metrics on 32 masks of 256^2 and on one 4096^2 mask.

    python scripts/morphology_bench.py [--windows 7] [--inner 10] [--out profiles/morphology_bench.json]

Legs, each at uint8 [32, 256, 256] and [1, 4096, 4096] (blobs: discs of mixed radii with holes and specks):
       (a) ``distance_transform`` to the background, unbounded and with ``max_dist=16``
       (b) ``mask_morphology`` dilate 8, erode 8, close 8, open 4
       (c) ``fill_holes``, ``mask_boundary``
       (d) ``mask_boundary_agreement`` of the mask against itself shifted by (3, 4)
       (e) the worst case of the outward search: ``distance_transform(to="foreground")`` of a single site in a 4096^2
           mask (no column but one holds a site, so every pixel searches until it reaches that column)
       (f) the host chain (a) and (b) replace: ``.cpu()``, ``scipy.ndimage.distance_transform_edt`` /
           ``binary_dilation`` with the disc, back to the device; timed once with the wall clock

A time is the HIP-event time of a window of ``--inner`` back-to-back calls divided by ``--inner``, the median of
``--windows`` such windows, after a warm-up of every leg; the smallest and largest window are kept too.  GB/s is the
bytes the passes of a leg must move (``must_move``: the mask once per column pass, 16 B per column and segment of
bits and carries written and read, g 2 B per pixel written and read, the output once) over that time.  No pass mark is set
on any time.  Writes one JSON object to ``--out`` and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stain2stain_amd import (distance_transform, fill_holes, mask_boundary, mask_boundary_agreement,  # noqa: E402
                             mask_morphology)
from stain2stain_amd.morphology import SEGMENT  # noqa: E402


def blobs(B, H, W, seed, dev):
    """uint8 [B, H, W]: discs of radius 3..40 (scaled with the side), each with a hole, and 0.1 % specks."""
    g = torch.Generator(device=dev).manual_seed(seed)
    yy = torch.arange(H, device=dev)[:, None]
    xx = torch.arange(W, device=dev)[None, :]
    out = torch.zeros((B, H, W), dtype=torch.uint8, device=dev)
    n = max(8, H * W // 8192)
    for b in range(B):
        cy = torch.rand(n, device=dev, generator=g) * H
        cx = torch.rand(n, device=dev, generator=g) * W
        r = 3 + torch.rand(n, device=dev, generator=g) * 37
        for i in range(0, n, 8):                                     # in groups: the [8, H, W] intermediates stay small
            d2 = (yy[None] - cy[i:i + 8, None, None]) ** 2 + (xx[None] - cx[i:i + 8, None, None]) ** 2
            rr = r[i:i + 8, None, None] ** 2
            out[b] |= ((d2 <= rr) & (d2 > rr * 0.09)).any(0).to(torch.uint8)
        out[b] |= (torch.rand((H, W), device=dev, generator=g) < 0.001).to(torch.uint8)
    return out


def timed(fn, windows, inner):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def must_move(B, H, W, transforms, out_bytes):
    """Bytes per call: per transform the mask, bits + carries (16 B per column and segment, written and read), g twice."""
    hw, cols = B * H * W, B * ((H + SEGMENT - 1) // SEGMENT) * W
    return transforms * (hw + 2 * 16 * cols + 2 * 2 * hw) + out_bytes * hw


def leg(res, name, fn, nbytes, windows, inner):
    r = timed(fn, windows, inner)
    if nbytes:
        r["must_move_bytes"] = nbytes
        r["gb_per_s"] = nbytes / (r["ms"] * 1e-3) / 1e9
    res[name] = r
    print(f"{name}: {r['ms']:.4f} ms" + (f", {r['gb_per_s']:.1f} GB/s" if nbytes else ""), flush=True)


def host_chain(mask, what):
    from scipy import ndimage
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = mask.cpu().numpy() != 0
    if what == "edt":
        out = np.stack([ndimage.distance_transform_edt(x) for x in m])
    else:
        yy, xx = np.mgrid[-8:9, -8:9]
        out = np.stack([ndimage.binary_dilation(x, yy * yy + xx * xx <= 64) for x in m])
    torch.from_numpy(out).to(mask.device)
    torch.cuda.synchronize()
    return {"ms": (time.perf_counter() - t0) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morphology_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "windows": args.windows, "inner": args.inner, "legs": {}}
    for tag, (B, H, W) in (("32x256", (32, 256, 256)), ("1x4096", (1, 4096, 4096))):
        m = blobs(B, H, W, 7, dev)
        other = torch.roll(m, (3, 4), dims=(1, 2))
        L = res["legs"]
        w, i = args.windows, args.inner
        L[f"{tag}/foreground_fraction"] = float(m.float().mean())
        leg(L, f"{tag}/edt", lambda: distance_transform(m), must_move(B, H, W, 1, 4), w, i)
        leg(L, f"{tag}/edt_max16", lambda: distance_transform(m, max_dist=16), must_move(B, H, W, 1, 4), w, i)
        leg(L, f"{tag}/dilate8", lambda: mask_morphology(m, "dilate", 8), must_move(B, H, W, 1, 1), w, i)
        leg(L, f"{tag}/erode8", lambda: mask_morphology(m, "erode", 8), must_move(B, H, W, 1, 1), w, i)
        leg(L, f"{tag}/close8", lambda: mask_morphology(m, "close", 8), must_move(B, H, W, 2, 2), w, i)
        leg(L, f"{tag}/open4", lambda: mask_morphology(m, "open", 4), must_move(B, H, W, 2, 2), w, i)
        leg(L, f"{tag}/fill_holes", lambda: fill_holes(m), 0, w, i)
        leg(L, f"{tag}/boundary", lambda: mask_boundary(m), 2 * B * H * W, w, i)
        leg(L, f"{tag}/agreement", lambda: mask_boundary_agreement(m, other), 0, w, i)
        L[f"{tag}/host_edt"] = host_chain(m, "edt")
        L[f"{tag}/host_dilate8"] = host_chain(m, "dilate")
        print(f"{tag}/host_edt: {L[f'{tag}/host_edt']['ms']:.1f} ms, host_dilate8: {L[f'{tag}/host_dilate8']['ms']:.1f} ms",
              flush=True)
    single = torch.zeros((1, 4096, 4096), dtype=torch.uint8, device=dev)
    single[0, 0, 0] = 1
    leg(res["legs"], "1x4096/edt_single_site", lambda: distance_transform(single, to="foreground"),
        must_move(1, 4096, 4096, 1, 4), max(3, args.windows // 2), max(1, args.inner // 5))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
