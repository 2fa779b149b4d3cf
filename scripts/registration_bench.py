"""Measurement for DESIGN.md 3.21: paired tile registration at B = 32, 256^2 tiles, radius 16.

    python scripts/registration_bench.py [--windows 9] [--inner 20] [--torch-inner 2] [--out profiles/registration_bench.json]

Legs:  (a) ``register_pairs`` at ``downsample=1``: two structure maps, 1089 shifts of a 224 x 224 template, the pick
       (b) the two-level form, ``downsample=4`` with refinement: radius 4 on 64^2 maps, then radius 4 at full resolution
       (c) the sums kernel of (a) alone, on maps made beforehand: its byte products per second
       (d) the definition of (a) composed from torch ops: per sample ``F.conv2d`` of the target map with the template
           as the filter (sum a b) and with a filter of ones on b and b^2, in fp32 -- the sums exceed 2^24, so unlike
           the kernels this leg is not exact; its picks are compared with (a)'s

A time is the HIP-event time of a window of ``--inner`` back-to-back calls divided by ``--inner``, the median of
``--windows`` such windows, after a warm-up of every leg.  The feature has no parent, so (d) is the only baseline and no
ratio is fixed in advance.  Writes one JSON object to ``--out`` (once after the fused legs, again with (d)) and prints it."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stain2stain_amd import ops, register_pairs, structure_map  # noqa: E402

B, HW, RADIUS = 32, 256, 16


def synthetic_pairs(dev, seed):
    """uint8 [B, HW, HW, 3] H&E and H-DAB tiles sharing a smooth haematoxylin field, the target displaced per sample."""
    g = torch.Generator(device=dev).manual_seed(seed)
    pad = 24
    field = torch.rand((B, 1, (HW + 2 * pad) // 4, (HW + 2 * pad) // 4), device=dev, generator=g)
    field = F.interpolate(field, size=(HW + 2 * pad, HW + 2 * pad), mode="bicubic").clamp(0, 1)[:, 0] ** 3 * 1.5
    shifts = torch.randint(-RADIUS, RADIUS + 1, (B, 2), device=dev, generator=g).tolist()
    hs = field[:, pad:pad + HW, pad:pad + HW]
    ht = torch.stack([field[n, pad - dy:pad - dy + HW, pad - dx:pad - dx + HW] for n, (dy, dx) in enumerate(shifts)])
    other = lambda: torch.rand((B, HW, HW), device=dev, generator=g) * 0.5     # noqa: E731

    def render(conc, vec):
        vec = torch.tensor(vec, device=dev)
        vec = vec / vec.norm(dim=1, keepdim=True)
        noisy = conc + 0.02 * torch.randn(conc.shape, device=dev, generator=g)
        return (255.0 * torch.pow(10.0, -(noisy @ vec))).round().clamp(0, 255).to(torch.uint8)

    src = render(torch.stack([hs, other()], -1), [[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]])
    tgt = render(torch.stack([0.7 * ht, other()], -1), [[0.650, 0.704, 0.286], [0.268, 0.570, 0.776]])
    return src, tgt, torch.tensor(shifts, dtype=torch.int32, device=dev)


def torch_register(a, b, R):
    """Leg (d): int64 [B, 2] picks from fp32 convolutions, per sample."""
    S = 2 * R + 1
    af, bf = a.float(), b.float()
    t = af[:, R:-R, R:-R]
    n = float(t[0].numel())
    ones = torch.ones_like(t[:1])[None]
    picks = []
    for s in range(a.shape[0]):
        x = bf[s][None, None]
        sab = F.conv2d(x, t[s][None, None])[0, 0]
        sb = F.conv2d(x, ones)[0, 0]
        sbb = F.conv2d(x * x, ones)[0, 0]
        sa, saa = t[s].sum(), (t[s] * t[s]).sum()
        score = (n * sab - sa * sb) / torch.sqrt((n * saa - sa * sa) * (n * sbb - sb * sb)).clamp_min(1e-30)
        picks.append(score.reshape(-1).argmax())
    k = torch.stack(picks)
    return torch.stack([k // S - R, k % S - R], dim=1)


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
    ap.add_argument("--torch-inner", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "registration_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("registration_bench needs a GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    src, tgt, planted = synthetic_pairs(dev, 1)
    a, b = structure_map(src, "hed"), structure_map(tgt, "hdab")
    S = 2 * RADIUS + 1
    tsum = torch.empty((B, 3), dtype=torch.int64, device=dev)
    sums = torch.empty((B, S, S, 3), dtype=torch.int64, device=dev)
    L = ops._L()

    def sums_only():
        rc = L.s2s_register_sums(a.data_ptr(), b.data_ptr(), B, HW, HW, RADIUS, 0, tsum.data_ptr(), sums.data_ptr(),
                                 ops._stream())
        assert rc == 0, rc

    legs = {
        "a_register_pairs_ds1": lambda: register_pairs(src, tgt, radius=RADIUS),
        "b_register_pairs_ds4_refine": lambda: register_pairs(src, tgt, radius=RADIUS, downsample=4),
        "c_sums_kernel_ds1": sums_only,
    }
    for fn in legs.values():                                       # warm up: code objects, allocator
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    one = legs["a_register_pairs_ds1"]()
    two = legs["b_register_pairs_ds4_refine"]()
    n = (HW - 2 * RADIUS) ** 2
    out = {"shape": {"B": B, "tile": HW, "radius": RADIUS, "shifts": S * S, "template_pixels": n},
           "windows": args.windows, "inner": args.inner,
           "a_recovers_planted": bool(torch.equal(one["shift"], planted)),
           "b_recovers_planted": bool(torch.equal(two["shift"], planted)),
           "a_min_margin": round(float(one["margin"].min()), 4)}
    ms = {k: median_ms(fn, args.windows, args.inner) for k, fn in legs.items()}
    out["ms_per_call"] = {k: round(v, 5) for k, v in ms.items()}
    out["tile_pairs_per_s"] = {k: round(B / v * 1e3) for k, v in ms.items()}
    products = B * S * S * n
    out["byte_products_per_call"] = products
    out["sums_kernel_byte_products_per_s"] = round(products / ms["c_sums_kernel_ds1"] * 1e3)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")

    write()
    torch_leg = lambda: torch_register(a, b, RADIUS)                # noqa: E731
    picks = torch_leg()                                             # also the warm-up: the library picks its algorithms
    torch.cuda.synchronize()
    out["d_picks_equal_a"] = bool(torch.equal(picks.to(torch.int32), one["shift"]))
    ms["d_torch_conv2d_fp32"] = median_ms(torch_leg, 3, args.torch_inner)
    out["ms_per_call"]["d_torch_conv2d_fp32"] = round(ms["d_torch_conv2d_fp32"], 4)
    out["a_speedup_over_torch_ops"] = round(ms["d_torch_conv2d_fp32"] / ms["a_register_pairs_ds1"], 1)
    write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
