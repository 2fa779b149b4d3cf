"""Measurement for DESIGN.md 3.37: seeded component selection and hysteresis thresholding on 32 tiles of 256^2 and on one
4096^2 map.

    python scripts/hysteresis_bench.py [--windows 5] [--inner 10] [--out profiles/hysteresis_bench.json]

Legs, each at [32, 256, 256] and [1, 4096, 4096]:
       (a) on three byte masks (a sparse field: 2 % of the pixels; a dense field of discs; all foreground):
           ``label_components(mask)`` and ``select_components(mask, marker=mask)``, which labels the same components and
           keeps every one: the difference is the cost of the added passes (zero, seed, gate)
       (b) on uint8 tiles (haematoxylin, a smooth DAB haze, DAB discs with a dense core): ``stain_objects`` at one
           threshold against ``stain_objects_hysteresis`` without a radius, and ``stain_objects_corrected`` against
           ``stain_objects_hysteresis`` at radius 32
       (c) ``s2s_hyst_mask`` alone (bins and tissue byte in, the dual-threshold byte and its counts out) against
           ``stain_histogram`` over the same pixels, the one-pass floor
       (d) the host chain (a) replaces, once, with the wall clock, on the dense field of 32 tiles: ``.cpu()``,
           ``scipy.ndimage.label`` per tile, ``bincount`` of the labels under the marker

A time is the HIP-event time of a window of back-to-back calls divided by their number (``--inner`` calls, or as many as
fill 50 ms), the median of ``--windows`` such windows, after a warm-up of every leg; the smallest and largest window are
kept too.  ``ns_per_pixel`` is that time over B H W.  ``ratios`` holds seeded / plain for every pair.  No pass mark is
set on any time.  Writes one JSON object to ``--out`` and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from background_bench import leg  # noqa: E402
from stain2stain_amd import (concentration_bins, hysteresis, label_components, select_components,  # noqa: E402
                             stain_histogram, stain_matrix, stain_objects, stain_objects_corrected,
                             stain_objects_hysteresis)

LOW, HIGH, SINGLE = 128 / 1024, 320 / 1024, 205 / 1024
RADIUS = 32


def discs(B, H, W, seed, dev, lo=3.0, hi=20.0):
    """bool [B, H, W]: H W / 8192 discs of radius lo..hi per sample; (discs, their centres' cores of a third the radius)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    yy = torch.arange(H, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    n = max(8, H * W // 8192)
    out = torch.zeros((B, H, W), dtype=torch.bool, device=dev)
    core = torch.zeros((B, H, W), dtype=torch.bool, device=dev)
    for b in range(B):
        cy = torch.rand(n, device=dev, generator=g) * H
        cx = torch.rand(n, device=dev, generator=g) * W
        r = lo + torch.rand(n, device=dev, generator=g) * (hi - lo)
        for i in range(0, n, 8):                                     # in groups: the [8, H, W] intermediates stay small
            d2 = (yy[None] - cy[i:i + 8, None, None]) ** 2 + (xx[None] - cx[i:i + 8, None, None]) ** 2
            out[b] |= (d2 <= r[i:i + 8, None, None] ** 2).any(0)
            core[b] |= (d2 <= (r[i:i + 8, None, None] / 3) ** 2).any(0)
    return out, core


def tiles(B, H, W, seed, dev):
    """uint8 [B, H, W, 3] by Beer-Lambert: H 0.1..0.5, a DAB haze of 0.02..0.1, discs of +0.2 with cores of +0.4, noise."""
    g = torch.Generator(device=dev).manual_seed(seed)
    halo, core = discs(B, H, W, seed + 1, dev, 3.0, 12.0)
    M = stain_matrix("hdab").to(dev).float()
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, :]
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    for b in range(B):
        dab = 0.06 + 0.04 * torch.sin(xx / 61.0 + b) + 0.2 * halo[b] + 0.4 * core[b] \
            + 0.03 * torch.randn((H, W), device=dev, generator=g)
        conc = torch.stack([0.1 + 0.4 * torch.rand((H, W), device=dev, generator=g), dab,
                            torch.zeros((H, W), device=dev)], -1).clamp_(min=0)
        out[b] = (255.0 * torch.pow(10.0, -(conc @ M))).round_().clamp_(0, 255).to(torch.uint8)
    return out


def host_chain(mask, marker):
    """.cpu(), scipy.ndimage.label and the bincount of the labels under the marker, tile by tile; wall clock."""
    from scipy import ndimage
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m, k = mask.cpu().numpy() != 0, marker.cpu().numpy() != 0
    kept = 0
    for n in range(m.shape[0]):
        lab, cnt = ndimage.label(m[n], structure=np.ones((3, 3), bool))
        seeds = np.bincount(lab[k[n] & m[n]], minlength=cnt + 1)
        seeds[0] = 0
        kept += int((seeds > 0)[lab].sum())
    return {"ms": (time.perf_counter() - t0) * 1e3, "kept_pixels": kept}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hysteresis_bench.json"))
    args = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "windows": args.windows, "inner": args.inner, "legs": {},
           "ratios": {}}
    L, Q = res["legs"], res["ratios"]
    for tag, (B, H, W) in (("32x256", (32, 256, 256)), ("1x4096", (1, 4096, 4096))):
        px, w, i = B * H * W, args.windows, args.inner
        g = torch.Generator(device=dev).manual_seed(3)
        dense, core = discs(B, H, W, 5, dev)
        masks = {"sparse": (torch.rand((B, H, W), device=dev, generator=g) < 0.02).to(torch.uint8),
                 "discs": dense.to(torch.uint8), "full": torch.ones((B, H, W), dtype=torch.uint8, device=dev)}
        for name, m in masks.items():
            leg(L, f"{tag}/{name}/label_components", lambda: label_components(m), px, w, i)
            leg(L, f"{tag}/{name}/select_components", lambda: select_components(m, m), px, w, i)
            leg(L, f"{tag}/{name}/select_components_mask", lambda: select_components(m, m, return_mask=True), px, w, i)
            Q[f"{tag}/{name}/select_over_label"] = L[f"{tag}/{name}/select_components"]["ms"] / \
                L[f"{tag}/{name}/label_components"]["ms"]
            L[f"{tag}/{name}/objects"] = int(label_components(m)["count"].sum())
        t = tiles(B, H, W, 7, dev)
        leg(L, f"{tag}/stain_objects", lambda: stain_objects(t, thresholds=(SINGLE,) * 3), px, w, i)
        leg(L, f"{tag}/stain_objects_hysteresis", lambda: stain_objects_hysteresis(t, LOW, HIGH), px, w, i)
        leg(L, f"{tag}/stain_objects_corrected_r{RADIUS}", lambda: stain_objects_corrected(t, RADIUS, SINGLE), px, w, i)
        leg(L, f"{tag}/stain_objects_hysteresis_r{RADIUS}",
            lambda: stain_objects_hysteresis(t, LOW, HIGH, radius=RADIUS), px, w, i)
        Q[f"{tag}/hysteresis_over_stain_objects"] = L[f"{tag}/stain_objects_hysteresis"]["ms"] / L[f"{tag}/stain_objects"]["ms"]
        Q[f"{tag}/hysteresis_over_corrected_r{RADIUS}"] = L[f"{tag}/stain_objects_hysteresis_r{RADIUS}"]["ms"] / \
            L[f"{tag}/stain_objects_corrected_r{RADIUS}"]["ms"]
        for key, r in (("single", stain_objects(t, thresholds=(SINGLE,) * 3)), ("hysteresis", stain_objects_hysteresis(t, LOW, HIGH))):
            L[f"{tag}/{key}_count"] = int(r["count"].sum())
            L[f"{tag}/{key}_positive"] = int(r["positive"].sum())
        bins = concentration_bins(t)
        tissue = torch.ones((B, H, W), dtype=torch.uint8, device=dev)
        counts = torch.empty((B, 3), dtype=torch.int64, device=dev)
        byte = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        leg(L, f"{tag}/hyst_mask", lambda: hysteresis._dual_mask(bins.data_ptr(), tissue.data_ptr(), B, H, W, 0, H, 128, 320,
                                                                False, 1, counts, byte.data_ptr(), H * W, "bench"), px, w, i)
        leg(L, f"{tag}/stain_histogram", lambda: stain_histogram(t), px, w, i)
        Q[f"{tag}/hyst_mask_over_stain_histogram"] = L[f"{tag}/hyst_mask"]["ms"] / L[f"{tag}/stain_histogram"]["ms"]
        L[f"{tag}/hyst_mask"]["gb_per_s"] = 4.0 * px / (L[f"{tag}/hyst_mask"]["ms"] * 1e6)      # 3 bytes in, 1 out
        if tag == "32x256":
            cores = core.to(torch.uint8)
            L[f"{tag}/discs/host_label_bincount"] = host_chain(masks["discs"], cores)
            leg(L, f"{tag}/discs/select_components_cores", lambda: select_components(masks["discs"], cores), px, w, i)
            print(f"{tag}/discs/host_label_bincount: {L[f'{tag}/discs/host_label_bincount']['ms']:.1f} ms", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
