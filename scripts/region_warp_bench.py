"""Measurement for DESIGN.md 3.22: dense region alignment of a 4096^2 region at cell 256 (a 16 x 16 field).

    python scripts/region_warp_bench.py [--windows 9] [--inner 20] [--out profiles/region_warp_bench.json]

Legs:  (a) ``warp_region`` of the uint8 [4096, 4096, 3] target through a cleaned, non-constant field: 3 B read (four
           taps, mostly from cache) and 3 B written per pixel
       (b) the same bytes through one ``shift_tiles`` launch, the region as one tile moved by one integer shift: the
           existing copy-shaped yardstick for 3 B in and 3 B out per pixel
       (c) the same definition composed from torch ops: the field interpolated to a dense displacement with
           ``F.interpolate`` and the image sampled with ``F.grid_sample`` in fp32 (bilinear, zero padding) -- not exact
           and its fill differs, so only its interior is compared with (a)
       (d) ``clean_shift_field`` of the 16 x 16 field
       (e) the whole ``register_region``: shift field at radius 16, cleaning, warp

A time is the HIP-event time of a window of ``--inner`` back-to-back calls divided by ``--inner``, the median of
``--windows`` such windows, after a warm-up of every leg.  No pass mark is set on any time.  Writes one JSON object to
``--out`` and prints it."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stain2stain_amd import clean_shift_field, register_region, region_shift_field, shift_tiles, warp_region  # noqa: E402

N, CELL, RADIUS, PLANTED = 4096, 256, 16, (3, -5)


def synthetic_region_pair(dev, seed):
    """uint8 [N, N, 3] H&E and H-DAB regions sharing a smooth haematoxylin field; ``tgt[y + 3, x - 5]`` is the tissue at
    ``src[y, x]``."""
    g = torch.Generator(device=dev).manual_seed(seed)
    pad = 24
    size = N + 2 * pad
    field = torch.rand((1, 1, size // 4, size // 4), device=dev, generator=g)
    field = F.interpolate(field, size=(size, size), mode="bicubic").clamp(0, 1)[0, 0] ** 3 * 1.5
    dy, dx = PLANTED
    hs = field[pad:pad + N, pad:pad + N]
    ht = field[pad - dy:pad - dy + N, pad - dx:pad - dx + N]

    def render(h, vec):
        vec = torch.tensor(vec, device=dev)
        vec = vec / vec.norm(dim=1, keepdim=True)
        out = torch.empty((N, N, 3), dtype=torch.uint8, device=dev)
        for r in range(0, N, 512):                                   # in slabs: the fp32 intermediates stay small
            conc = torch.stack([h[r:r + 512], torch.rand((512, N), device=dev, generator=g) * 0.5], -1)
            conc = conc + 0.02 * torch.randn(conc.shape, device=dev, generator=g)
            out[r:r + 512] = (255.0 * torch.pow(10.0, -(conc @ vec))).round().clamp(0, 255).to(torch.uint8)
        return out

    src = render(hs, [[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]])
    tgt = render(0.7 * ht, [[0.650, 0.704, 0.286], [0.268, 0.570, 0.776]])
    return src, tgt


def torch_warp(img_f, field):
    """Leg (c): fp32 [1, 3, N, N] sampled through the field with torch ops; node centres are what ``align_corners=False``
    interpolates between, edges clamp as the definition does."""
    d = field.to(torch.float32).permute(2, 0, 1)[None] / 16.0                       # [1, 2, Gy, Gx] in pixels
    dense = F.interpolate(d, size=(N, N), mode="bilinear", align_corners=False)
    ys = torch.arange(N, device=img_f.device, dtype=torch.float32)
    gy = (ys[:, None] + dense[0, 0] + 0.5) * (2.0 / N) - 1.0
    gx = (ys[None, :] + dense[0, 1] + 0.5) * (2.0 / N) - 1.0
    return F.grid_sample(img_f, torch.stack([gx, gy], -1)[None], mode="bilinear", padding_mode="zeros",
                         align_corners=False)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_warp_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("region_warp_bench needs a GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    src, tgt = synthetic_region_pair(dev, 1)
    measured = region_shift_field(src, tgt, CELL, radius=RADIUS)
    cleaned = clean_shift_field(measured)
    # a non-constant field for the warp legs: the measured one plus a smooth sub-pixel ramp of up to 2 pixels
    G = N // CELL
    ramp = torch.linspace(-32, 32, G, device=dev).round().to(torch.int32)
    field = (cleaned["field"] + torch.stack([ramp[:, None].expand(G, G), ramp[None, :].expand(G, G)], -1)).contiguous()
    one_shift = torch.tensor([list(PLANTED)], dtype=torch.int32, device=dev)
    img_f = tgt.permute(2, 0, 1)[None].float()

    legs = {
        "a_warp_region": lambda: warp_region(tgt, field, CELL),
        "b_shift_tiles_one_launch": lambda: shift_tiles(tgt[None], one_shift),
        "d_clean_shift_field": lambda: clean_shift_field(measured),
        "e_register_region": lambda: register_region(src, tgt, CELL, radius=RADIUS),
        "c_torch_grid_sample_fp32": lambda: torch_warp(img_f, field),
    }
    for fn in legs.values():                                       # warm up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {"shape": {"region": N, "cell": CELL, "grid": G, "radius": RADIUS, "bytes_in_plus_out": 6 * N * N},
           "windows": args.windows, "inner": args.inner,
           "shift_field_recovers_planted": bool((measured["shift"] == one_shift[0]).all()),
           "cells_kept": int(cleaned["stats"][0]), "fill_iterations": int(cleaned["stats"][1])}
    warped = legs["a_warp_region"]()
    ref = legs["c_torch_grid_sample_fp32"]()[0].permute(1, 2, 0)
    m = 8
    diff = (warped[m:-m, m:-m].float() - ref[m:-m, m:-m]).abs()
    out["c_max_abs_difference_from_a_interior"] = round(float(diff.max()), 3)
    out["constant_field_equals_shift_tiles"] = bool(torch.equal(
        warp_region(tgt, (one_shift[0] * 16).repeat(G, G, 1), CELL), legs["b_shift_tiles_one_launch"]()[0]))
    ms = {}
    for k, fn in legs.items():
        slow = k.startswith(("c_", "e_"))
        ms[k] = median_ms(fn, 3 if slow else args.windows, 2 if slow else args.inner)
    out["ms_per_call"] = {k: round(v, 5) for k, v in ms.items()}
    out["GB_per_s"] = {k: round(6 * N * N / ms[k] * 1e-6, 1) for k in ("a_warp_region", "b_shift_tiles_one_launch")}
    out["a_over_b"] = round(ms["a_warp_region"] / ms["b_shift_tiles_one_launch"], 3)
    out["a_speedup_over_torch_ops"] = round(ms["c_torch_grid_sample_fp32"] / ms["a_warp_region"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
