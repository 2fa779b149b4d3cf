"""Measurement for DESIGN.md 3.26: object morphometry on 32 label images of 256^2 and on one of 4096^2.

    python scripts/object_features_bench.py [--windows 7] [--inner 10] [--out profiles/object_features_bench.json]

Two fields per size: ``sparse``, 300 small discs per sample labelled by ``label_components`` (the table holds 512
objects), and ``single``, the contention worst case of one object covering the image.  Legs:
  (a) ``shape_pass``        the two launches of s2s_objfeat_shape on zeroed tables, without and (``shape_pass_d2``) with the
                            distance map; GB/s over the bytes the pass must read (4 B per pixel of labels, 8 with d2)
  (b) ``intensity_u8``      the launch of s2s_objfeat_intensity_u8 (a wave of background reads no pixel, so its traffic
                            depends on the field: time only)
  (c) ``object_features``   the public call: shape, thickness, intensity, finalize, with its allocations
  (d) ``stain_mask_u8``     the plain-read yardstick: s2s_stain_mask_u8 over the same pixels, 3 B read + 1 B written
  (e) ``torch_ops``         the same integers composed from torch ops: ``bincount``, ``scatter_add`` and ``scatter_reduce``
                            over the flattened labels, i.e. one global atomic per pixel and quantity
  (f) ``host_scipy``        ``labels.cpu()`` and scipy.ndimage (sum_labels for the area and the five moments,
                            find_objects, maximum of d2), timed once with the wall clock

A time is the HIP-event time of a window of ``--inner`` back-to-back calls divided by ``--inner``, the median of
``--windows`` such windows, after a warm-up of every leg; the smallest and largest window are kept too.  No pass mark is
set on any time.  Writes one JSON object to ``--out`` and prints it."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stain2stain_amd import _native, distance_transform, label_components, object_features, ops  # noqa: E402
from stain2stain_amd.stain_quant import _kernel_args  # noqa: E402

OF = importlib.import_module("stain2stain_amd.object_features")
M = 512


def sparse_field(B, H, W, seed, dev):
    """int32 labels [B, H, W]: 300 discs per sample, radius 1.5..5 scaled with the side / 256."""
    g = torch.Generator(device=dev).manual_seed(seed)
    yy = torch.arange(H, device=dev)[:, None]
    xx = torch.arange(W, device=dev)[None, :]
    mask = torch.zeros((B, H, W), dtype=torch.uint8, device=dev)
    s = max(1.0, H / 1024)
    for b in range(B):
        cy = torch.rand(300, device=dev, generator=g) * H
        cx = torch.rand(300, device=dev, generator=g) * W
        r = (1.5 + torch.rand(300, device=dev, generator=g) * 3.5) * s
        for i in range(0, 300, 10):
            d2 = (yy[None] - cy[i:i + 10, None, None]) ** 2 + (xx[None] - cx[i:i + 10, None, None]) ** 2
            mask[b] |= (d2 <= r[i:i + 10, None, None] ** 2).any(0).to(torch.uint8)
    return label_components(mask)["labels"]


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


def leg(res, name, fn, nbytes, windows, inner):
    r = timed(fn, windows, inner)
    if nbytes:
        r["must_move_bytes"] = nbytes
        r["gb_per_s"] = nbytes / (r["ms"] * 1e-3) / 1e9
    res[name] = r
    print(f"{name}: {r['ms']:.4f} ms" + (f", {r['gb_per_s']:.1f} GB/s" if nbytes else ""), flush=True)


def torch_ops(labels, d2):
    """The integer table from torch ops: one atomic per pixel and quantity."""
    B, H, W = labels.shape
    lab = labels.long()
    key = (lab + torch.arange(B, device=lab.device)[:, None, None] * (M + 1)).reshape(-1).clamp_(max=B * (M + 1) - 1)
    n = B * (M + 1)
    yy = torch.arange(H, device=lab.device)[None, :, None].expand(B, H, W).reshape(-1)
    xx = torch.arange(W, device=lab.device)[None, None, :].expand(B, H, W).reshape(-1)
    p = torch.nn.functional.pad(lab, (1, 1, 1, 1), value=-1)
    e = ((p[:, :-2, 1:-1] != lab).long() + (p[:, 2:, 1:-1] != lab) + (p[:, 1:-1, :-2] != lab) + (p[:, 1:-1, 2:] != lab)).reshape(-1)
    out = [torch.bincount(key, minlength=n)]
    for v in (yy, xx, yy * yy, xx * xx, yy * xx, e, (e > 0).long()):
        out.append(torch.zeros(n, dtype=torch.int64, device=lab.device).scatter_add_(0, key, v))
    for v, red in ((yy, "amin"), (xx, "amin"), (yy, "amax"), (xx, "amax"), (d2.reshape(-1).long(), "amax")):
        out.append(torch.zeros(n, dtype=torch.int64, device=lab.device).scatter_reduce_(0, key, v, red, include_self=False))
    return out


def host_scipy(labels, d2):
    from scipy import ndimage
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lab, dist = labels.cpu().numpy(), d2.cpu().numpy()
    H, W = lab.shape[1:]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for l, d in zip(lab, dist):
        idx = np.arange(1, min(int(l.max()), M) + 1)
        for w in (np.ones_like(yy), yy, xx, yy * yy, xx * xx, yy * xx):
            ndimage.sum_labels(w, l, idx)
        ndimage.find_objects(l)
        ndimage.maximum(d, l, idx)
    return {"ms": (time.perf_counter() - t0) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "object_features_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "windows": args.windows, "inner": args.inner, "max_objects": M,
           "legs": {}}
    L = res["legs"]
    lib = ops._L()
    table, unmix = _kernel_args("hdab", (0.2, 0.2, 0.2))
    for tag, (B, H, W) in (("32x256", (32, 256, 256)), ("1x4096", (1, 4096, 4096))):
        w, i = args.windows, args.inner
        px = B * H * W
        img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev,
                            generator=torch.Generator(device=dev).manual_seed(5))
        mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        tissue = torch.zeros((B,), dtype=torch.int64, device=dev)

        def stain_mask():
            _native.check(lib.s2s_stain_mask_u8(img.data_ptr(), 3 * W, 3 * W * H, B, 0, H, H, W, table, unmix, 220, 0, 1,
                                                mask.data_ptr(), W, H * W, tissue.data_ptr(), ops._stream()), "mask")

        leg(L, f"{tag}/stain_mask_u8", stain_mask, 4 * px, w, i)
        for field, labels in (("sparse", sparse_field(B, H, W, 11, dev)),
                              ("single", torch.ones((B, H, W), dtype=torch.int32, device=dev))):
            d2 = distance_transform(labels > 0)
            t = OF._tables(dev, B, M, True, True)
            name = f"{tag}/{field}"
            L[f"{name}/objects_per_sample"] = float(labels.amax(dim=(1, 2)).float().mean())
            L[f"{name}/object_pixel_fraction"] = float((labels > 0).float().mean())
            leg(L, f"{name}/shape_pass", lambda: OF._shape_pass(labels, None, t, B, H, W, M, "bench"), 4 * px, w, i)
            leg(L, f"{name}/shape_pass_d2", lambda: OF._shape_pass(labels, d2, t, B, H, W, M, "bench"), 8 * px, w, i)
            leg(L, f"{name}/intensity_u8",
                lambda: OF._intensity_pass(labels, img, "u8", t, B, H, W, M, table, unmix, 1, "bench"), 0, w, i)
            leg(L, f"{name}/object_features", lambda: object_features(labels, M, image=img), 0, w, i)
            slow = field == "single"
            leg(L, f"{name}/torch_ops", lambda: torch_ops(labels, d2), 0, 3 if slow else w, 1 if slow else i)
            L[f"{name}/host_scipy"] = host_scipy(labels, d2)
            print(f"{name}/host_scipy: {L[f'{name}/host_scipy']['ms']:.1f} ms", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
