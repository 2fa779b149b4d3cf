"""Measurement for DESIGN.md 3.23: tile quality control of 32 tiles of 256^2 and of a 4096^2 region.

    python scripts/qc_bench.py [--windows 9] [--inner 20] [--out profiles/qc_bench.json]

Legs:  (a) ``tile_qc`` of a uint8 [32, 256, 256, 3] batch
       (b) ``region_qc_map`` of a uint8 [4096, 4096, 3] GPU region at cell 256 (16 x 16 cells)
       (c) ``region_qc`` of the same region at tile 256, overlap 32 (19 x 19 overlapping tiles: 1.41 x the pixels)
       (a'), (b') the two launches of (a) and of (b) alone, through the C ABI with every buffer made once: what is left
           of a call's time is the wrapper (argument checks, allocations, the upload of the origins)
       (d) the yardstick: ``stain_quantify`` of the batch of (a) and ``region_stain_map`` of the region of (b), existing
           kernels that also read every byte once, with more arithmetic per pixel
       (e) the definition of (b) composed from torch ops: integer luma, an ``F.conv2d`` Laplacian (fp32 is exact for
           these integers), comparisons, per-cell sums in int64; its counts are compared with (b)'s

A time is the HIP-event time of a window of ``--inner`` back-to-back calls divided by ``--inner``, the median of
``--windows`` such windows, after a warm-up of every leg; the smallest and largest window are kept too.  GB/s counts the
image bytes once (3 B per pixel of the batch or the region), for (c) as well.  No pass mark is set on any time.  Writes
one JSON object to ``--out`` and prints it."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stain2stain_amd import ops, region_qc, region_qc_map, region_stain_map, stain_quantify, tile_qc  # noqa: E402

N, CELL, OVERLAP, BATCH = 4096, 256, 32, 32
WHITE, BLACK, INK, DARK = 220, 0, 40, 60


def synthetic_region(dev, seed):
    """uint8 [N, N, 3]: an H&E-like region (a smooth haematoxylin field on noisy eosin) with a glass margin, a green and
    a blue marker stroke and a black fold, so every class of pixel occurs."""
    g = torch.Generator(device=dev).manual_seed(seed)
    field = torch.rand((1, 1, N // 4, N // 4), device=dev, generator=g)
    h = F.interpolate(field, size=(N, N), mode="bicubic").clamp(0, 1)[0, 0] ** 3 * 1.5
    vec = torch.tensor([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]], device=dev)
    vec = vec / vec.norm(dim=1, keepdim=True)
    out = torch.empty((N, N, 3), dtype=torch.uint8, device=dev)
    for r in range(0, N, 512):                                       # in slabs: the fp32 intermediates stay small
        conc = torch.stack([h[r:r + 512], 0.2 + torch.rand((512, N), device=dev, generator=g) * 0.5], -1)
        conc = conc + 0.02 * torch.randn(conc.shape, device=dev, generator=g)
        out[r:r + 512] = (255.0 * torch.pow(10.0, -(conc.clamp(min=0) @ vec))).round().clamp(0, 255).to(torch.uint8)
    out[:, :300] = 240
    out[1000:1040, 500:3000] = torch.tensor([30, 150, 60], dtype=torch.uint8, device=dev)
    out[500:3000, 2000:2040] = torch.tensor([30, 60, 160], dtype=torch.uint8, device=dev)
    out[3000:3060, 1000:3500] = 20
    return out


def torch_qc_map(region):
    """Leg (e): int64 [G, G, 8] from torch ops."""
    a = region.to(torch.int32)
    R, Gc, B = a.unbind(-1)
    mx, mn = a.amax(-1), a.amin(-1)
    tissue = (mn < WHITE) & (mx >= BLACK)
    Y = (77 * R + 150 * Gc + 29 * B + 128) >> 8
    k = torch.tensor([[0.0, 1.0, 0.0], [1.0, -4.0, 1.0], [0.0, 1.0, 0.0]], device=region.device)[None, None]
    L = F.conv2d(Y.to(torch.float32)[None, None], k, padding=1)[0, 0].to(torch.int64)
    focus = tissue.clone()
    focus[0], focus[-1], focus[:, 0], focus[:, -1] = False, False, False, False
    zero = torch.zeros_like(L)
    maps = (tissue, focus, torch.where(focus, L, zero), torch.where(focus, L * L, zero),
            torch.where(tissue, Y.to(torch.int64), zero), tissue & (Gc - torch.maximum(R, B) >= INK),
            tissue & (B - R >= INK) & (Gc >= R), tissue & (mx < DARK))
    G = N // CELL
    return torch.stack([m.to(torch.int64).reshape(G, CELL, G, CELL).sum((1, 3)) for m in maps], -1)


def launches_only(img, origins, win):
    """The two launches of a call and nothing else: ``img`` contiguous uint8 [B, H, W, 3], every buffer made once."""
    B, H, W = (int(v) for v in img.shape[:3])
    n, L = int(origins.shape[0]), ops._L()
    nchunk = L.s2s_qc_chunks(win, win)
    slab = torch.empty((B * n * nchunk, 8), dtype=torch.int64, device=img.device)
    counts = torch.empty((B * n, 8), dtype=torch.int64, device=img.device)
    derived = torch.empty((B * n, 5), dtype=torch.float64, device=img.device)

    def run():
        rc = L.s2s_qc_windows_u8(img.data_ptr(), 3 * W, 3 * W * H, B, 0, H, H, W, origins.data_ptr(), n, win, win, 0, H,
                                 WHITE, BLACK, INK, DARK, slab.data_ptr(), ops._stream())
        rc = rc or L.s2s_qc_finalize(slab.data_ptr(), B * n, nchunk, 0, origins.data_ptr(), n, H, W, win, win,
                                     counts.data_ptr(), derived.data_ptr(), ops._stream())
        if rc:
            raise RuntimeError(f"qc launch failed with status {rc}")
        return counts
    return run


def window_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qc_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("qc_bench needs a GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    region = synthetic_region(dev, 1)
    tiles = torch.stack([region[CELL * (3 + i // 8):CELL * (4 + i // 8), CELL * (2 + i % 8):CELL * (3 + i % 8)]
                         for i in range(BATCH)]).contiguous()

    G = N // CELL
    cells = torch.tensor([[gy * CELL, gx * CELL] for gy in range(G) for gx in range(G)], dtype=torch.int32, device=dev)
    legs = {
        "a_launches_only": launches_only(tiles, torch.zeros((1, 2), dtype=torch.int32, device=dev), CELL),
        "b_launches_only": launches_only(region[None], cells, CELL),
        "a_tile_qc": lambda: tile_qc(tiles),
        "d_stain_quantify": lambda: stain_quantify(tiles),
        "b_region_qc_map": lambda: region_qc_map(region, CELL),
        "d_region_stain_map": lambda: region_stain_map(region, cell=CELL),
        "c_region_qc": lambda: region_qc(region, CELL, OVERLAP),
        "e_torch_ops_map": lambda: torch_qc_map(region),
    }
    for fn in legs.values():                                       # warm up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    m = legs["b_region_qc_map"]()
    whole = tile_qc(region[None])
    out = {"shape": {"region": N, "cell": CELL, "overlap": OVERLAP, "tiles": BATCH, "plan_tiles": int(
               legs["c_region_qc"]()["counts"].shape[0])},
           "windows": args.windows, "inner": args.inner,
           "region_counts": dict(zip(("tissue", "focus_n", "lap_sum", "lap_sq", "luma_sum", "green", "blue", "dark"),
                                     whole["counts"][0].tolist())),
           "region_focus": round(float(whole["focus"][0]), 3),
           "cells_add_up_to_the_region": bool(torch.equal(m["counts"].reshape(-1, 8).sum(0), whole["counts"][0])),
           "e_counts_equal_b": bool(torch.equal(legs["e_torch_ops_map"](), m["counts"])),
           "launches_only_equal_the_calls": bool(
               torch.equal(legs["b_launches_only"]().reshape(G, G, 8), m["counts"])
               and torch.equal(legs["a_launches_only"](), legs["a_tile_qc"]()["counts"]))}
    ms, spread = {}, {}
    for k, fn in legs.items():
        slow = k.startswith("e_")
        w = [window_ms(fn, 2 if slow else args.inner) for _ in range(3 if slow else args.windows)]
        ms[k], spread[k] = statistics.median(w), [round(min(w), 5), round(max(w), 5)]
    nbytes = {k: 3 * (BATCH * CELL * CELL if k in ("a_tile_qc", "a_launches_only", "d_stain_quantify") else N * N)
              for k in legs}
    out["ms_per_call"] = {k: round(v, 5) for k, v in ms.items()}
    out["ms_min_max_window"] = spread
    out["image_bytes"] = nbytes
    out["GB_per_s"] = {k: round(nbytes[k] / ms[k] * 1e-6, 1) for k in legs}
    out["a_over_d_stain_quantify"] = round(ms["a_tile_qc"] / ms["d_stain_quantify"], 3)
    out["b_over_d_region_stain_map"] = round(ms["b_region_qc_map"] / ms["d_region_stain_map"], 3)
    out["c_over_b"] = round(ms["c_region_qc"] / ms["b_region_qc_map"], 3)
    out["b_speedup_over_torch_ops"] = round(ms["e_torch_ops_map"] / ms["b_region_qc_map"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
