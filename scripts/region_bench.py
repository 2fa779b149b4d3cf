"""Whole-region translation on one GPU (stain2stain_amd.region.translate_region), one JSON line:
  * the wall time of one call and its MPix/s (host clock around the call, device synchronised at both ends; the mean
    of --repeat calls after one warm-up call that captures the sampler's graph);
  * the time inside the sampler calls (HIP events around each call) and the remainder of the call;
  * the gather / blend / finalise kernels' times per region call from a separate run of this script under
    `rocprofv3 --kernel-trace --stats` (a child process), with their achieved GB/s against algorithmic bytes.
Settings: default FlowUNet in bf16, a synthetic uint8 region, tile 256, overlap 32, batch 32, 50 Euler steps as a
graph.  --min-tissue F runs the call with ``min_tissue=F`` (background tiles skip the sampler) and
--background FRACTION makes that share of the region's rows glass (bytes >= --white; implies --min-tissue 0.5); the
line then also holds kept, skipped and sampler_calls, and the kernel table the tissue count, the skip weights and the
mixed finalise.  Usage: python scripts/region_bench.py [--size 4096] [--repeat 3] [--no-profile] [--out-dir DIR]
[--background FRACTION] [--min-tissue F] [--white 220]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from stain2stain_amd import FlowUNet, euler_generate, plan_region_batches, tissue_counts, translate_region
from stain2stain_amd.region import band_rows_for, plan_tiles

DEV = "cuda:0"
KERNELS = ("region_gather_kernel", "region_blend_kernel", "region_finalize_kernel")


def algorithmic_bytes(H, W, tile, overlap, batch, C=3):
    """Bytes each kernel has to move for one region call: gather reads the tiles' pixels and writes fp32 NCHW tiles
    (padded batches included); blend reads the tile outputs and reads + writes the ring rows a batch spans; finalise
    reads the accumulator, writes the uint8 image and clears the accumulator."""
    tops = plan_tiles(H, W, tile, overlap)[:, 0].tolist()
    N = len(tops)
    nb = -(-N // batch)
    gather = nb * batch * tile * tile * 3 * (1 + 4)
    blend = 0
    for b in range(nb):
        p0, pn = b * batch, min(batch, N - b * batch)
        rows = min(H, tops[p0 + pn - 1] + tile) - tops[p0]
        blend += pn * C * tile * tile * 4 + 2 * rows * W * (C + 1) * 4
    finalize = H * W * ((C + 1) * 4 * 2 + 3)
    return dict(zip(KERNELS, (gather, blend, finalize)))


SKIP_KERNELS = ("region_gather_kernel", "region_blend_kernel", "region_tissue_count_kernel",
                "region_skip_weight_kernel", "region_finalize_mixed_kernel")


def algorithmic_bytes_skipping(H, W, tile, overlap, batch, keep, C=3):
    """The same for a call with ``min_tissue``: gather and blend move the kept tiles only (padded sampler calls
    included); the count reads every tile's pixels once; the skip weights read and write the weight-ring rows of every
    range with a skipped tile; the mixed finalise reads both rings and the source, writes the uint8 image and clears
    both rings."""
    plan = plan_tiles(H, W, tile, overlap)
    tops = plan[:, 0].tolist()
    kept = keep.tolist()
    gather = blend = skip = 0
    for p0, p1 in plan_region_batches(plan, keep, batch, band_rows_for(H, W, tile, overlap, batch), tile):
        rows = min(H, tops[p1 - 1] + tile) - tops[p0]
        nk = sum(kept[p0:p1])
        if nk:
            gather += batch * tile * tile * 3 * (1 + 4)
            blend += nk * C * tile * tile * 4 + 2 * rows * W * (C + 1) * 4
        if nk < p1 - p0:
            skip += 2 * rows * W * 4
    count = sum(min(tile, H - y) * min(tile, W - x) * 3 for y, x in plan.tolist()) + 4 * len(tops)
    finalize = H * W * ((C + 1) * 4 * 2 + 4 * 2 + 3 + 3)
    return dict(zip(SKIP_KERNELS, (gather, blend, count, skip, finalize)))


def make_image(args):
    g = torch.Generator(device=DEV).manual_seed(1984)
    img = torch.randint(0, 256, (args.size, args.size, 3), generator=g, dtype=torch.uint8, device=DEV)
    glass = round(args.background * args.size)
    if glass:                                              # the lower rows are glass: bytes in [white, 255]
        img[args.size - glass:] = torch.randint(args.white, 256, (glass, args.size, 3), generator=g, dtype=torch.uint8,
                                                device=DEV)
    return img


def run(args):
    torch.manual_seed(1984)
    net = FlowUNet(precision="bf16").to(DEV).eval()
    img = make_image(args)
    spans = []

    def sampler(x):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = euler_generate(net, x, args.steps, graph=True)
        e1.record()
        spans.append((e0, e1))
        return out

    kw = dict(tile=args.tile, overlap=args.overlap, batch=args.batch)
    if args.min_tissue is not None:
        kw.update(min_tissue=args.min_tissue, white=args.white)
    translate_region(img, sampler, **kw)                   # warm-up: captures the graph, loads every kernel
    torch.cuda.synchronize()
    walls, samp = [], []
    for _ in range(args.repeat):
        spans.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        translate_region(img, sampler, **kw)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
        samp.append(sum(a.elapsed_time(b) for a, b in spans) / 1e3)
    return walls, samp, dict(translate_region.last_stats)


def profile(args):
    """Kernel times per region call from a child process under rocprofv3 (warm-up call + one call)."""
    out = os.path.join(args.out_dir, "rocprof")
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "region", "--",
           sys.executable, os.path.abspath(__file__), "--inner", "--repeat", "1", "--size", str(args.size),
           "--tile", str(args.tile), "--overlap", str(args.overlap), "--batch", str(args.batch),
           "--steps", str(args.steps), "--background", str(args.background), "--white", str(args.white)]
    if args.min_tissue is not None:
        cmd += ["--min-tissue", str(args.min_tissue)]
    rc = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=args.profile_timeout)
    if rc.returncode != 0:
        raise RuntimeError(f"rocprofv3 run failed ({rc.returncode}): {rc.stderr.decode()[-2000:]}")
    files = glob.glob(os.path.join(out, "**", "region_kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError(f"no region_kernel_stats.csv under {out}")
    calls_per_run = 2                                      # the warm-up call and the timed one
    if args.min_tissue is None:
        names, nbytes = KERNELS, algorithmic_bytes(args.size, args.size, args.tile, args.overlap, args.batch)
    else:
        counts, areas = tissue_counts(make_image(args), args.tile, args.overlap, white=args.white)
        keep = torch.tensor([c >= args.min_tissue * a for c, a in zip(counts.tolist(), areas.tolist())])
        nbytes = algorithmic_bytes_skipping(args.size, args.size, args.tile, args.overlap, args.batch, keep)
        names = tuple(k for k in SKIP_KERNELS if nbytes[k])  # no launch without a kept / a skipped tile
    res = {}
    for row in csv.DictReader(open(files[0])):
        for k in names:
            if k in row["Name"]:
                r = res.setdefault(k, {"launches": 0, "ns": 0.0})
                r["launches"] += int(row["Calls"])
                r["ns"] += float(row["TotalDurationNs"])
    for k in names:
        if k not in res:
            raise RuntimeError(f"{k} missing from the kernel statistics")
        r = res[k]
        ms = r["ns"] / calls_per_run / 1e6
        res[k] = {"ms_per_call": round(ms, 3), "launches_per_call": r["launches"] // calls_per_run,
                  "algorithmic_MB": round(nbytes[k] / 1e6, 1), "GB_s": round(nbytes[k] / (ms * 1e-3) / 1e9, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--background", type=float, default=0.0, help="share of the region's rows that is glass")
    ap.add_argument("--min-tissue", type=float, default=None, help="run with min_tissue (default 0.5 with --background)")
    ap.add_argument("--white", type=int, default=220)
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-timeout", type=int, default=300)
    ap.add_argument("--out-dir", default=None, help="where the rocprofv3 output goes (default: a new temporary directory)")
    ap.add_argument("--inner", action="store_true", help=argparse.SUPPRESS)   # the child under rocprofv3
    args = ap.parse_args()
    if not 0.0 <= args.background <= 1.0:
        raise SystemExit("region_bench: --background must lie in [0, 1]")
    if args.background and args.min_tissue is None:
        args.min_tissue = 0.5
    if not torch.cuda.is_available():
        raise SystemExit("region_bench: needs a GPU")
    if args.inner:
        run(args)
        return
    if not args.no_profile:
        args.out_dir = args.out_dir or tempfile.mkdtemp(prefix="region_bench_")
    kernels = None if args.no_profile else profile(args)
    walls, samp, st = run(args)
    wall = sum(walls) / len(walls)
    s = sum(samp) / len(samp)
    mpix = args.size * args.size / 1e6
    line = {"metric": "region_translate", "size": args.size, "tile": args.tile, "overlap": args.overlap,
            "batch": args.batch, "euler_steps": args.steps, "precision": "bf16", "tiles": st["tiles"],
            "batches": st["batches"], "band_rows": st["band_rows"], "background": args.background,
            "min_tissue": args.min_tissue, "kept": st["kept"], "skipped": st["skipped"],
            "sampler_calls": st["sampler_calls"],
            "accumulator_MB": round(st["accumulator_bytes"] / 1e6, 1),
            "wall_s": round(wall, 4), "wall_s_each": [round(w, 4) for w in walls], "MPix_s": round(mpix / wall, 3),
            "sampler_s": round(s, 4), "outside_sampler_s": round(wall - s, 4),
            "outside_sampler_pct": round(100 * (wall - s) / wall, 3)}
    if kernels is not None:
        line["kernels"] = kernels
        k_ms = sum(v["ms_per_call"] for v in kernels.values())
        line["region_kernels_pct_of_call"] = round(100 * k_ms / 1e3 / wall, 3)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
