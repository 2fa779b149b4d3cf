"""Measurement for DESIGN.md 3.27: splitting touching objects on 32 masks of 256^2 and on one of 4096^2.

    python scripts/split_bench.py [--windows 7] [--inner 10] [--out profiles/split_bench.json]

Three fields per size: ``sparse``, 60 small discs per 256^2 (radius 1.5..5, few touch), ``dense``, 140 discs per 256^2
(radius 4..11, most overlap a neighbour), and ``full``, the all-foreground mask whose distance map is one plateau of
``FAR``.  The 4096^2 mask is a 16 x 16 mosaic of 256^2 fields, so the objects have the same size at both sizes.  Legs:
  (a) ``split_objects``       the public call: the distance transform, the thirteen launches of s2s_split_label, with its
                              allocations
  (b) ``split_label``         the same with the distance map handed in (``d2=``): the splitting alone
  (c) ``distance_transform``  the transform alone
  (d) ``unsplit``             ``distance_transform`` + ``label_components`` over the same mask: what a caller paid for the
                              map and the unsplit objects before this feature; neither function changed
  (e) ``host_chain``          ``mask.cpu()`` -> scipy.ndimage.distance_transform_edt -> seeds where the distance equals its
                              7 x 7 maximum filter -> scipy.ndimage.watershed_ift, timed once with the wall clock
``ratio_split_over_unsplit`` = (a) / (d) and ``ratio_host_over_split`` = (e) / (a) are stored beside them, with the part,
basin and component counts of the field.

A time is the HIP-event time of a window of ``--inner`` back-to-back calls divided by ``--inner``, the median of
``--windows`` such windows, after a warm-up of every leg; the smallest and largest window are kept too.  No pass mark is
set on any time.  Writes one JSON object to ``--out`` and prints it."""
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

from stain2stain_amd import distance_transform, label_components, split_objects  # noqa: E402

FIELDS = {"sparse": (60, 1.5, 5.0), "dense": (140, 4.0, 11.0)}          # discs per 256^2, smallest and largest radius


def disc_fields(B, count, r_lo, r_hi, seed, dev):
    """uint8 [B, 256, 256]: ``count`` discs per sample."""
    g = torch.Generator(device=dev).manual_seed(seed)
    yy = torch.arange(256, device=dev)[:, None]
    xx = torch.arange(256, device=dev)[None, :]
    mask = torch.zeros((B, 256, 256), dtype=torch.uint8, device=dev)
    for b in range(B):
        cy = torch.rand(count, device=dev, generator=g) * 256
        cx = torch.rand(count, device=dev, generator=g) * 256
        r = r_lo + torch.rand(count, device=dev, generator=g) * (r_hi - r_lo)
        for i in range(0, count, 20):
            d2 = (yy[None] - cy[i:i + 20, None, None]) ** 2 + (xx[None] - cx[i:i + 20, None, None]) ** 2
            mask[b] |= (d2 <= r[i:i + 20, None, None] ** 2).any(0).to(torch.uint8)
    return mask


def field(name, big, seed, dev):
    """uint8 [32, 256, 256], or [1, 4096, 4096] as a mosaic of 256 fields."""
    if name == "full":
        return torch.ones((1, 4096, 4096) if big else (32, 256, 256), dtype=torch.uint8, device=dev)
    m = disc_fields(256 if big else 32, *FIELDS[name], seed, dev)
    if big:
        m = m.view(16, 16, 256, 256).permute(0, 2, 1, 3).reshape(1, 4096, 4096).contiguous()
    return m


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


def host_chain(mask):
    from scipy import ndimage
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    parts = 0
    for m in mask.cpu().numpy():
        d = ndimage.distance_transform_edt(m)
        seeds, _ = ndimage.label((d == ndimage.maximum_filter(d, size=7)) & (m > 0))
        cost = (65535 - np.minimum(d * 256.0, 65535.0)).astype(np.uint16)
        cost[m == 0] = 65535
        lab = ndimage.watershed_ift(cost, seeds.astype(np.int32))
        parts += len(np.unique(lab[m > 0]))
    return {"ms": (time.perf_counter() - t0) * 1e3, "parts": parts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "windows": args.windows, "inner": args.inner, "neck": 0.75,
           "connectivity": 8, "legs": {}}
    L = res["legs"]
    for tag, big in (("32x256", False), ("1x4096", True)):
        for k, name in enumerate(("sparse", "dense", "full")):
            mask = field(name, big, 11 + k, dev)
            key = f"{tag}/{name}"
            out = split_objects(mask)
            d2 = out["d2"]
            comp = label_components(mask)
            L[f"{key}/foreground_fraction"] = float((mask > 0).float().mean())
            L[f"{key}/components"] = int(comp["count"].sum())
            L[f"{key}/basins"] = int(out["basins"].sum())
            L[f"{key}/parts"] = int(out["count"].sum())
            legs = {"split_objects": lambda: split_objects(mask), "split_label": lambda: split_objects(mask, d2=d2),
                    "distance_transform": lambda: distance_transform(mask),
                    "unsplit": lambda: (distance_transform(mask), label_components(mask))}
            for leg, fn in legs.items():
                L[f"{key}/{leg}"] = r = timed(fn, args.windows, args.inner if not big else max(1, args.inner // 3))
                print(f"{key}/{leg}: {r['ms']:.4f} ms", flush=True)
            L[f"{key}/host_chain"] = h = host_chain(mask)
            print(f"{key}/host_chain: {h['ms']:.1f} ms", flush=True)
            L[f"{key}/ratio_split_over_unsplit"] = L[f"{key}/split_objects"]["ms"] / L[f"{key}/unsplit"]["ms"]
            L[f"{key}/ratio_host_over_split"] = h["ms"] / L[f"{key}/split_objects"]["ms"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
