"""Measurement for DESIGN.md 3.36: grey opening and background-corrected stain quantification on 32 tiles of 256^2 and on
one 4096^2 map.

    python scripts/background_bench.py [--windows 5] [--inner 10] [--out profiles/background_bench.json]

Legs, each at uint8 [32, 256, 256, 3] and [1, 4096, 4096, 3] (haematoxylin, a smooth DAB haze, DAB discs of mixed radii):
       (a) ``stain_histogram``: one pass over the same bytes, the floor
       (b) ``distance_transform`` of the raw positive mask: the nearest existing multi-pass morphology
       (c) ``concentration_bins``
       (d) ``grey_morphology(bins, "open", r, footprint)`` for r in 8, 32, 128 and both footprints
       (e) ``stain_quantify_corrected(tiles, r, footprint=...)`` (smooth = 2) for the same
       (f) the host chain (e) replaces, on ONE 256^2 tile: ``stain_separate``, ``.cpu()``,
           ``scipy.ndimage.white_tophat`` with the disc (r = 8 and 32), at most 16 threads; timed once with the wall clock;
           at r = 8 the GPU opening of that tile is also compared with scipy's erosion and dilation for equality

A time is the HIP-event time of a window of back-to-back calls divided by their number (``--inner`` calls, or as many
as fill 50 ms; a fifth of ``--inner`` at least for the radius-128 legs), the median of ``--windows`` such windows, after
a warm-up of every leg; the smallest and largest window are kept too.  ``ns_per_pixel`` is that time over B H W.  No pass
mark is set on any time.  Writes one JSON object to ``--out`` and prints it."""
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

from stain2stain_amd import (concentration_bins, distance_transform, grey_morphology, stain_histogram,  # noqa: E402
                             stain_matrix, stain_quantify_corrected, stain_separate)

RADII = (8, 32, 128)
THRESHOLD = 205 / 1024


def tiles(B, H, W, seed, dev):
    """uint8 [B, H, W, 3] by Beer-Lambert from H 0.1..0.5, a DAB haze of 0.05..0.45 and DAB discs of radius 3..40."""
    g = torch.Generator(device=dev).manual_seed(seed)
    yy = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    M = stain_matrix("hdab").to(dev).float()
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    n = max(8, H * W // 8192)
    for b in range(B):
        ph = torch.rand(4, device=dev, generator=g) * 6.28
        haze = 0.25 + 0.1 * torch.sin(yy / 97.0 + ph[0]) * torch.cos(xx / 131.0 + ph[1]) + 0.1 * torch.sin(xx / 61.0 + ph[2])
        cy = torch.rand(n, device=dev, generator=g) * H
        cx = torch.rand(n, device=dev, generator=g) * W
        r = 3 + torch.rand(n, device=dev, generator=g) * 37
        blob = torch.zeros((H, W), dtype=torch.bool, device=dev)
        for i in range(0, n, 8):                                     # in groups: the [8, H, W] intermediates stay small
            d2 = (yy[None] - cy[i:i + 8, None, None]) ** 2 + (xx[None] - cx[i:i + 8, None, None]) ** 2
            blob |= (d2 <= r[i:i + 8, None, None] ** 2).any(0)
        conc = torch.stack([0.1 + 0.4 * torch.rand((H, W), device=dev, generator=g),
                            haze + 0.5 * blob + 0.02 * torch.randn((H, W), device=dev, generator=g),
                            torch.zeros((H, W), device=dev)], -1).clamp_(min=0)
        out[b] = (255.0 * torch.pow(10.0, -(conc @ M))).round_().clamp_(0, 255).to(torch.uint8)
    return out


WINDOW_MS = 50.0             # a window holds at least this much work (``--inner`` calls, or more of a short leg)


def timed(fn, windows, inner):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(3):
        fn()
    b.record()
    b.synchronize()
    inner = int(min(max(inner, WINDOW_MS / max(a.elapsed_time(b) / 3, 1e-3)), 1000))
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "calls_per_window": inner}


def leg(res, name, fn, pixels, windows, inner):
    r = timed(fn, windows, inner)
    r["ns_per_pixel"] = r["ms"] * 1e6 / pixels
    res[name] = r
    print(f"{name}: {r['ms']:.4f} ms, {r['ns_per_pixel']:.4f} ns/pixel", flush=True)


def disc(r):
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    return yy * yy + xx * xx <= r * r


def host_chain(tile, r):
    """stain_separate, .cpu(), scipy's white top-hat of the DAB plane of one tile."""
    from scipy import ndimage
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c = stain_separate(tile)[0, 1].cpu().numpy()
    out = ndimage.white_tophat(c, footprint=disc(r))
    torch.from_numpy(out).to(tile.device)
    torch.cuda.synchronize()
    return {"ms": (time.perf_counter() - t0) * 1e3}


def equal_to_scipy(tile, r):
    from scipy import ndimage
    b = concentration_bins(tile)
    x = b[0].cpu().numpy()
    e = ndimage.grey_erosion(x, footprint=disc(r), mode="constant", cval=32767)
    want = ndimage.grey_dilation(e, footprint=disc(r), mode="constant", cval=-32768)
    return bool(np.array_equal(grey_morphology(b, "open", r)[0].cpu().numpy(), want))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "background_bench.json"))
    args = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "windows": args.windows, "inner": args.inner, "legs": {}}
    L = res["legs"]
    for tag, (B, H, W) in (("32x256", (32, 256, 256)), ("1x4096", (1, 4096, 4096))):
        t = tiles(B, H, W, 7, dev)
        bins = concentration_bins(t)
        raw = (bins >= 205).to(torch.uint8)
        px, w, i = B * H * W, args.windows, args.inner
        q0 = stain_quantify_corrected(t, None, THRESHOLD)
        L[f"{tag}/raw_burden"] = float(q0["burden"].mean())
        leg(L, f"{tag}/stain_histogram", lambda: stain_histogram(t), px, w, i)
        leg(L, f"{tag}/distance_transform", lambda: distance_transform(raw), px, w, i)
        leg(L, f"{tag}/concentration_bins", lambda: concentration_bins(t), px, w, i)
        for r in RADII:
            n = max(1, i // 5) if r == 128 else i
            for fp in ("disc", "square"):
                leg(L, f"{tag}/open_{fp}{r}", lambda: grey_morphology(bins, "open", r, fp), px, w, n)
                leg(L, f"{tag}/quantify_corrected_{fp}{r}",
                    lambda: stain_quantify_corrected(t, r, THRESHOLD, footprint=fp), px, w, n)
            L[f"{tag}/corrected_burden_disc{r}"] = float(stain_quantify_corrected(t, r, THRESHOLD)["burden"].mean())
        if tag == "32x256":
            for r in (8, 32):
                L[f"1x256/host_white_tophat_disc{r}"] = host_chain(t[:1], r)
                print(f"1x256/host_white_tophat_disc{r}: {L[f'1x256/host_white_tophat_disc{r}']['ms']:.1f} ms", flush=True)
                leg(L, f"1x256/quantify_corrected_disc{r}", lambda: stain_quantify_corrected(t[:1], r, THRESHOLD), H * W, w, i)
            L["1x256/open_disc8_equals_scipy"] = equal_to_scipy(t[:1], 8)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
