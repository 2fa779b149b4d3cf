"""Measurement for DESIGN.md 3.32: result rendering of a 4096^2 region with a sparse object field and a 16 x 16 map.

    python scripts/render_bench.py [--windows 9] [--inner 20] [--legs a,b,...] [--out profiles/render_bench.json]

Legs:  copy      the region's bytes through one ``shift_tiles`` launch (3 B in and 3 B out per pixel): the copy bound
       classes   ``render_classes`` of an int32 label image (discs on a 64-pixel lattice, 8 % of the pixels) and of the
                 same objects as a uint8 class mask, outline 1; fresh result and in place
       heat      ``render_heat`` of a 16 x 16 map at cell 256, interpolated and flat; fresh and in place with min_index
       compare   the three modes of ``compare_regions``
       thumb     ``downsample_region`` at 4 and 16, image and mask
       layers    ``render_region`` with an outline layer over a heat layer
       torch_*   the same definitions composed from torch ops in int32 (labels with outline 1, the flat heat map, the
                 blend, the factor-4 thumbnail), checked equal to the kernels' bytes

A time is the HIP-event time of a window of ``--inner`` back-to-back calls divided by ``--inner``, the median of
``--windows`` such windows, after a warm-up of every leg.  No pass mark is set on any time.  Writes one JSON object to
``--out`` and prints it.  ``--legs`` runs only the named legs, without the equality checks and ratios: for a run under
``rocprofv3 --kernel-trace --stats``, where every kernel name should stand for one configuration."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stain2stain_amd import (colormap, compare_regions, default_palette, downsample_region, render_classes,  # noqa: E402
                             render_heat, render_region, shift_tiles)
from stain2stain_amd.render import quantize_map  # noqa: E402

N, CELL, PITCH, RADIUS = 4096, 256, 64, 10


def object_field(dev):
    """int32 [N, N]: a disc of radius 10 on every node of a 64-pixel lattice, each with its own label."""
    ys = torch.arange(N, device=dev)
    cy, cx = ys // PITCH, ys // PITCH
    oy, ox = ys % PITCH - PITCH // 2, ys % PITCH - PITCH // 2
    inside = (oy[:, None] ** 2 + ox[None, :] ** 2) <= RADIUS * RADIUS
    labels = (cy[:, None] * (N // PITCH) + cx[None, :] + 1).to(torch.int32)
    return torch.where(inside, labels, torch.zeros_like(labels))


def mix(b, c, a):
    return (b * (256 - a) + c * a + 128) >> 8


def torch_labels(region, labels, pal, alpha):
    """The label overlay with outline 1 and the palette colour on the edge, from torch ops in int32."""
    ident = labels.clamp(min=0)
    k = torch.where(labels <= 0, torch.zeros_like(labels), (labels - 1) % 255 + 1).long()
    pad = torch.nn.functional.pad(ident, (1, 1, 1, 1), value=-1)
    edge = ((pad[:-2, 1:-1] != ident) | (pad[2:, 1:-1] != ident) | (pad[1:-1, :-2] != ident) | (pad[1:-1, 2:] != ident))
    edge &= ident != 0
    a = torch.where(edge, 256, torch.where(k > 0, alpha, 0)).to(torch.int32)[..., None]
    return mix(region.to(torch.int32), pal.to(torch.int32)[k], a).to(torch.uint8)


def torch_heat_flat(region, q, lut, alpha):
    idx = ((q.clamp(0, 65280) + 128) >> 8).long()
    idx = idx.repeat_interleave(CELL, 0).repeat_interleave(CELL, 1)
    return mix(region.to(torch.int32), lut.to(torch.int32)[idx], alpha).to(torch.uint8)


def torch_blend(a, b, alpha):
    return mix(a.to(torch.int32), b.to(torch.int32), alpha).to(torch.uint8)


def torch_thumb(region, f):
    s = region.to(torch.int32).reshape(N // f, f, N // f, f, 3).sum((1, 3))
    return ((2 * s + f * f) // (2 * f * f)).to(torch.uint8)


def window_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def median_ms(fn, windows, inner):
    return statistics.median(window_ms(fn, inner) for _ in range(windows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--legs", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("render_bench needs a GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(1)
    region = torch.randint(0, 256, (N, N, 3), dtype=torch.uint8, device=dev, generator=g)
    other = torch.randint(0, 256, (N, N, 3), dtype=torch.uint8, device=dev, generator=g)
    labels = object_field(dev)
    classes = ((labels - 1) % 255 + 1).where(labels > 0, torch.zeros_like(labels)).to(torch.uint8)
    values = torch.rand((N // CELL, N // CELL), device=dev, generator=g)
    q = quantize_map(values)
    pal, lut = default_palette().to(dev), colormap("heat").to(dev)
    zero = torch.zeros((1, 2), dtype=torch.int32, device=dev)
    work = region.clone()

    legs = {
        "copy_shift_tiles": lambda: shift_tiles(region[None], zero),
        "classes_labels": lambda: render_classes(region, labels),
        "classes_mask": lambda: render_classes(region, classes),
        "classes_labels_in_place": lambda: render_classes(work, labels, out=work),
        "classes_labels_outline4": lambda: render_classes(region, labels, outline=4),
        "heat_smooth": lambda: render_heat(region, q, CELL, quantized=True),
        "heat_flat": lambda: render_heat(region, q, CELL, quantized=True, smooth=False),
        "heat_smooth_in_place_min_index_128": lambda: render_heat(work, q, CELL, quantized=True, min_index=128, out=work),
        "compare_checker": lambda: compare_regions(region, other, "checker"),
        "compare_blend": lambda: compare_regions(region, other, "blend"),
        "compare_difference": lambda: compare_regions(region, other, "difference"),
        "thumb_4": lambda: downsample_region(region, 4),
        "thumb_16": lambda: downsample_region(region, 16),
        "thumb_mask_4": lambda: downsample_region(classes, 4),
        "layers_heat_then_outline": lambda: render_region(region, [("heat", q, CELL, {"quantized": True}),
                                                                   ("classes", labels, {"alpha": 0})]),
        "torch_labels": lambda: torch_labels(region, labels, pal, 96),
        "torch_heat_flat": lambda: torch_heat_flat(region, q, lut, 128),
        "torch_blend": lambda: torch_blend(region, other, 128),
        "torch_thumb_4": lambda: torch_thumb(region, 4),
    }
    only = [k for k in args.legs.split(",") if k]
    if only:
        legs = {k: legs[k] for k in only}
    for fn in legs.values():                                       # warm up: code objects, allocator, tables
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {"shape": {"region": N, "cell": CELL, "grid": N // CELL, "objects": (N // PITCH) ** 2,
                     "object_pixel_fraction": round(float((labels > 0).float().mean()), 4), "bytes_in_plus_out": 6 * N * N},
           "windows": args.windows, "inner": args.inner}
    if not only:
        out["equal_to_torch"] = {
            "labels": bool(torch.equal(legs["classes_labels"](), legs["torch_labels"]())),
            "mask_equals_labels": bool(torch.equal(legs["classes_mask"](), legs["classes_labels"]())),
            "heat_flat": bool(torch.equal(legs["heat_flat"](), legs["torch_heat_flat"]())),
            "blend": bool(torch.equal(legs["compare_blend"](), legs["torch_blend"]())),
            "thumb_4": bool(torch.equal(legs["thumb_4"](), legs["torch_thumb_4"]()))}
    ms = {}
    for k, fn in legs.items():
        slow = k.startswith("torch_")
        ms[k] = median_ms(fn, 3 if slow else args.windows, 2 if slow else args.inner)
    out["ms_per_call"] = {k: round(v, 5) for k, v in ms.items()}
    if not only:
        ratios(out, ms)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


def ratios(out, ms):
    copy = ms["copy_shift_tiles"]
    out["over_copy"] = {k: round(v / copy, 3) for k, v in ms.items() if not k.startswith(("torch_", "copy_"))}
    out["speedup_over_torch_ops"] = {"classes_labels": round(ms["torch_labels"] / ms["classes_labels"], 2),
                                     "heat_flat": round(ms["torch_heat_flat"] / ms["heat_flat"], 2),
                                     "compare_blend": round(ms["torch_blend"] / ms["compare_blend"], 2),
                                     "thumb_4": round(ms["torch_thumb_4"] / ms["thumb_4"], 2)}


if __name__ == "__main__":
    main()
