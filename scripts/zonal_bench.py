"""Measurement for DESIGN.md 3.34: the zonal table against the quantification pass and the calibration histogram over the
same bytes (one more byte per pixel is read, so the ratio is the cost of the LDS table), on three zone maps: a constant
one (every wave takes the one-zone path), 64-pixel blocks (lanes uniform, waves mixed) and per-pixel random zones (every
pixel pays its own LDS atomics): the spread between them is the cost of the fallback path.  Then ``stain_zonal`` against
the loop of Z masked ``stain_quantify`` calls it replaces, the pair form against ``stain_agreement``, ``object_zones``
against the same table from ``torch.bincount`` over ``label * Z + zone``, and ``distance_zones``; at 32 x 256^2 and on
one large region.

    python scripts/zonal_bench.py [--iters 20] [--region 8192] [--zones 8] [--out profiles/zonal_bench.json] [--ablate]

``--ablate`` loads the -DS2S_ABLATE library, in which every wave takes the plain LDS atomics: the "before" of the one-zone
wave path (the results are the same); its numbers go to ``profiles/zonal_bench_ablate.json`` unless ``--out`` is given.
Times are HIP-event medians over ``--iters`` calls after a warm-up: whole calls, launches and allocations included.
Prints one JSON line and writes it to ``--out``."""
import argparse
import json
import os
import sys

if "--ablate" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import ablate_lib  # noqa: F401  (first: loads the -DS2S_ABLATE library)

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stain2stain_amd import (distance_zones, object_zones, region_stain_map, region_stain_zonal,  # noqa: E402
                             region_stain_zonal_agreement, region_stain_agreement, region_stain_histogram, stain_agreement,
                             stain_histogram, stain_quantify, stain_zonal, stain_zonal_agreement)


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


def zone_maps(shape, Z, g, dev):
    """{"constant", "blocks64", "random"}: uint8 zone maps of ``shape`` ([..., H, W]) with bytes below Z."""
    H, W = shape[-2:]
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    blocks = ((xx // 64 + 3 * (yy // 64)) % Z).to(torch.uint8)
    return {"constant": torch.full(shape, Z // 2, dtype=torch.uint8, device=dev),
            "blocks64": blocks.expand(shape).contiguous().to(dev),
            "random": torch.randint(0, Z, shape, generator=g, dtype=torch.uint8).to(dev)}


def masked_loop(u, zones, Z):
    """What stain_zonal replaces: Z passes over the bytes, each with a temporary whose other zones are glass."""
    return [stain_quantify(torch.where((zones == z)[..., None], u, torch.full_like(u, 255))) for z in range(Z)]


def bincount_overlap(labels, zones, Z, M):
    """overlap [B, M, Z] of object_zones from torch ops."""
    B = labels.shape[0]
    keep = (labels > 0) & (labels <= M) & (zones < Z)
    key = torch.where(keep, (labels.long() - 1) * Z + zones.long(), torch.full_like(labels, M * Z, dtype=torch.int64))
    return torch.stack([torch.bincount(key[n].flatten(), minlength=M * Z + 1)[:M * Z] for n in range(B)]).view(B, M, Z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--region", type=int, default=8192)
    ap.add_argument("--zones", type=int, default=8)
    ap.add_argument("--ablate", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = args.out or os.path.join(root, "profiles", "zonal_bench_ablate.json" if args.ablate else "zonal_bench.json")
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    B, H, n, Z = 32, 256, args.region, args.zones
    it, rit = args.iters, max(5, args.iters // 2)
    u = torch.randint(0, 256, (B, H, H, 3), generator=g, dtype=torch.uint8).to(dev)
    v = torch.randint(0, 256, (B, H, H, 3), generator=g, dtype=torch.uint8).to(dev)
    out = {"shape_batch": [B, H, H], "shape_region": [n, n], "zones": Z, "iters": it, "wave_path": not args.ablate}

    def put(key, ms, nbytes=None):
        out[key + "_ms"] = round(ms, 5)
        if nbytes:
            out[key + "_GBps"] = round(nbytes / ms / 1e6, 1)

    px = B * H * H
    maps = zone_maps((B, H, H), Z, g, dev)
    put("batch_quantify", timed(lambda: stain_quantify(u), it), 3 * px)
    put("batch_histogram", timed(lambda: stain_histogram(u), it), 3 * px)
    put("batch_agreement", timed(lambda: stain_agreement(u, v), it), 6 * px)
    for name, zm in maps.items():
        put(f"batch_zonal_{name}", timed(lambda: stain_zonal(u, zm, Z), it), 4 * px)
        put(f"batch_zonal_pooled_{name}", timed(lambda: stain_zonal(u, zm, Z, pool=True), it), 4 * px)
        put(f"batch_zonal_pair_{name}", timed(lambda: stain_zonal_agreement(u, v, zm, Z), it), 7 * px)
    z256 = torch.randint(0, 256, (B, H, H), generator=g, dtype=torch.uint8).to(dev)
    put("batch_zonal_random_256_zones", timed(lambda: stain_zonal(u, z256, 256), it), 4 * px)
    put("batch_masked_quantify_loop", timed(lambda: masked_loop(u, maps["blocks64"], Z), max(3, it // 4)))
    loop = masked_loop(u, maps["blocks64"], Z)
    zz = stain_zonal(u, maps["blocks64"], Z)
    out["masked_loop_equal"] = bool(all(torch.equal(loop[z]["positive"], zz["positive"][:, z]) and
                                        torch.equal(loop[z]["tissue"], zz["tissue"][:, z]) for z in range(Z)))
    # objects by zone: some 400 objects of 8 x 8 pixels per sample
    M = 512
    cells = torch.arange(1, 1 + (H // 12) ** 2, dtype=torch.int32).view(H // 12, H // 12)
    lab = torch.zeros((H, H), dtype=torch.int32)
    lab[: 12 * (H // 12), : 12 * (H // 12)] = cells.repeat_interleave(12, 0).repeat_interleave(12, 1)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(H), indexing="ij")
    lab[(yy % 12 >= 8) | (xx % 12 >= 8)] = 0
    labels = lab.expand(B, H, H).contiguous().to(dev)
    for name in ("blocks64", "random"):
        zm = maps[name]
        put(f"batch_object_zones_{name}", timed(lambda: object_zones(labels, zm, Z, max_objects=M), it), 5 * px)
        put(f"batch_object_overlap_bincount_{name}", timed(lambda: bincount_overlap(labels, zm, Z, M), max(3, it // 4)))
        out[f"bincount_equal_{name}"] = bool(torch.equal(
            bincount_overlap(labels, zm, Z, M).int(), object_zones(labels, zm, Z, max_objects=M, return_overlap=True)["overlap"]))
    mask = labels > 0
    put("batch_distance_zones_4_edges", timed(lambda: distance_zones(mask, [1, 2, 4, 8]), it))
    del u, v, maps, z256, labels, mask, loop, zz
    # the region
    r = torch.randint(0, 256, (n, n, 3), generator=g, dtype=torch.uint8).to(dev)
    r2 = torch.randint(0, 256, (n, n, 3), generator=g, dtype=torch.uint8).to(dev)
    rpx = n * n
    rmaps = zone_maps((n, n), Z, g, dev)
    put("region_map", timed(lambda: region_stain_map(r), rit), 3 * rpx)
    put("region_histogram", timed(lambda: region_stain_histogram(r), rit), 3 * rpx)
    put("region_agreement", timed(lambda: region_stain_agreement(r, r2), rit), 6 * rpx)
    for name, zm in rmaps.items():
        put(f"region_zonal_{name}", timed(lambda: region_stain_zonal(r, zm, Z), rit), 4 * rpx)
        put(f"region_zonal_pair_{name}", timed(lambda: region_stain_zonal_agreement(r, r2, zm, Z), rit), 7 * rpx)
    for a, b in (("batch_zonal_constant", "batch_quantify"), ("batch_zonal_constant", "batch_histogram"),
                 ("batch_zonal_blocks64", "batch_zonal_constant"), ("batch_zonal_random", "batch_zonal_constant"),
                 ("batch_zonal_pair_constant", "batch_agreement"), ("batch_zonal_pair_random", "batch_zonal_pair_constant"),
                 ("batch_masked_quantify_loop", "batch_zonal_blocks64"),
                 ("batch_object_overlap_bincount_blocks64", "batch_object_zones_blocks64"),
                 ("batch_object_overlap_bincount_random", "batch_object_zones_random"),
                 ("region_zonal_constant", "region_map"), ("region_zonal_constant", "region_histogram"),
                 ("region_zonal_random", "region_zonal_constant"), ("region_zonal_pair_constant", "region_agreement")):
        out[f"ratio_{a}_over_{b}"] = round(out[a + "_ms"] / out[b + "_ms"], 3)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
