"""Measurement for DESIGN.md 3.20: the fused paired augmentation at the benchmark's input shape (B = 16, 512^2 sources,
256^2 crops of synthetic H&E).

    python scripts/augment_bench.py [--reps 5] [--windows 9] [--inner 50] [--out profiles/augment_bench.json]

Legs:  (a) ``paired_crop_flip_normalize`` (what bench.py calls)      (b) ``paired_augment`` without maps
       (c) (b) with both stain maps     (d) (c) with the class mask     (e) (d) with every sample transposed
       (f) the definition of (d) composed from torch ops (gathers, a batched matmul, exp2, where, permute)

A time is the HIP-event time of a window of ``--inner`` back-to-back calls divided by ``--inner``, the median of
``--windows`` such windows: the calls are a few microseconds of traffic each, so this is the rate at which a training
loop can issue them, host work included.  Legs (a) and (b) alternate, ``--reps`` medians each; the spread of (a) is the
relative range of its medians, and (b), which does the job of (a), passes when its median of medians is not above (a)'s
by more than that spread.  ``bytes`` is the algorithmic traffic of a call: each source byte read once, each output
written once.  Writes one JSON object to ``--out`` and prints it."""
import argparse
import json
import os
import random
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stain2stain_amd import paired_augment, sample_stain_jitter, stain_jitter_maps  # noqa: E402
from stain2stain_amd.data import paired_crop_flip_normalize, sample_crop_flip_params  # noqa: E402
from stain2stain_amd.stain_quant import od_table  # noqa: E402

B, HW, S, WHITE = 16, 512, 256, 230


def synthetic_he(shape, dev, seed):
    """uint8 [..., 3]: gamma-distributed haematoxylin and eosin concentrations, a quarter bare glass."""
    torch.manual_seed(seed)
    g = torch.Generator(device=dev).manual_seed(seed)
    vec = torch.tensor([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]], device=dev)
    vec = vec / vec.norm(dim=1, keepdim=True)
    conc = torch.empty((*shape, 2), device=dev)
    conc[..., 0] = torch.distributions.Gamma(2.0, 1 / 0.22).sample(torch.Size(shape)).to(dev)
    conc[..., 1] = torch.distributions.Gamma(2.0, 1 / 0.18).sample(torch.Size(shape)).to(dev)
    img = 255.0 * torch.pow(10.0, -(conc @ vec))
    bare = torch.rand(shape, device=dev, generator=g) < 0.25
    img[bare] = 245.0
    return img.round().clamp(0, 255).to(torch.uint8)


def torch_augment(src, tgt, mask, params, maps_s, maps_t, table, white):
    """Leg (f): (src fp32, tgt fp32, mask fp32, src u8, tgt u8) from torch ops; params / maps already on the device."""
    n = src.shape[0]
    ar = torch.arange(S, device=src.device)
    top, left, hf, vf, tr = (params[:, k, None] for k in range(5))
    ys = top + torch.where(vf.bool(), S - 1 - ar, ar)
    xs = left + torch.where(hf.bool(), S - 1 - ar, ar)
    bi = torch.arange(n, device=src.device)[:, None, None]
    swap = tr.bool()[:, :, None]

    def geo(img):
        f = img[bi, ys[:, :, None], xs[:, None, :]]
        return torch.where(swap if f.dim() == 3 else swap[..., None], f.transpose(1, 2), f)

    def colour(f, maps):
        od = table[f.long()].reshape(n, -1, 3)
        od2 = torch.baddbmm(maps[:, None, 9:], od, maps[:, :9].reshape(n, 3, 3))
        u = (255.0 * torch.exp2(od2 * -3.321928094887362)).round().clamp(0, 255).to(torch.uint8).reshape(f.shape)
        return torch.where((f.amin(-1) >= white)[..., None], f, u)

    def net(u):
        return ((u.float() / 255.0 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()

    us, ut = colour(geo(src), maps_s), colour(geo(tgt), maps_t)
    return net(us), net(ut), geo(mask).float()[:, None], us, ut


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("augment_bench needs a GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    src, tgt = synthetic_he((B, HW, HW), dev, 1), synthetic_he((B, HW, HW), dev, 2)
    mask = torch.randint(0, 4, (B, HW, HW), dtype=torch.uint8, device=dev)
    rng = random.Random(0)
    p4 = sample_crop_flip_params(B, (HW, HW), S, rng)
    p5 = torch.cat([p4, torch.zeros((B, 1), dtype=torch.int32)], dim=1)
    p5t = torch.cat([p4, torch.ones((B, 1), dtype=torch.int32)], dim=1)
    ms_, mt_ = (stain_jitter_maps(sample_stain_jitter(B, rng=rng), s) for s in ("hed", "hdab"))
    maps = {"src_map": ms_, "tgt_map": mt_, "white": WHITE}
    table = od_table().to(dev)
    dp5, dms, dmt = p5.to(dev).long(), ms_.to(dev), mt_.to(dev)

    legs = {
        "a_paired_crop_flip_normalize": lambda: paired_crop_flip_normalize(src, tgt, p4, S),
        "b_paired_augment": lambda: paired_augment(src, tgt, p4, S),
        "c_maps": lambda: paired_augment(src, tgt, p5, S, **maps),
        "d_maps_mask": lambda: paired_augment(src, tgt, p5, S, mask_u8=mask, **maps),
        "e_maps_mask_transposed": lambda: paired_augment(src, tgt, p5t, S, mask_u8=mask, **maps),
        "f_torch_ops": lambda: torch_augment(src, tgt, mask, dp5, dms, dmt, table, WHITE),
    }
    px = B * S * S
    nbytes = {"a_paired_crop_flip_normalize": px * (6 + 24), "b_paired_augment": px * (6 + 24),
              "c_maps": px * (6 + 24), "d_maps_mask": px * (7 + 28), "e_maps_mask_transposed": px * (7 + 28),
              "f_torch_ops": px * (7 + 28)}
    for fn in legs.values():                                       # warm up every leg: code objects, allocator, pinned pool
        for _ in range(5):
            fn()
    torch.cuda.synchronize()

    out = {"shape": {"B": B, "source": HW, "crop": S}, "windows": args.windows, "inner": args.inner,
           "bytes_per_tile_pair": {k: v // B for k, v in nbytes.items()}}
    # same results first: (b) against (a) bit for bit, (f) against (d) to the level that rounding may move
    a, b = legs["a_paired_crop_flip_normalize"](), legs["b_paired_augment"]()
    out["b_equals_a"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
    d = paired_augment(src, tgt, p5, S, mask_u8=mask, return_u8=True, **maps)
    f = legs["f_torch_ops"]()
    out["f_vs_d_max_level_diff"] = int(max((d[3].int() - f[3].int()).abs().max(), (d[4].int() - f[4].int()).abs().max()))
    out["f_vs_d_bytes_differing"] = int((d[3] != f[3]).sum() + (d[4] != f[4]).sum())
    out["f_vs_d_mask_equal"] = bool(torch.equal(d[2], f[2]))

    ra, rb = [], []
    for _ in range(args.reps):                                     # alternate: other work shares the host
        ra.append(median_ms(legs["a_paired_crop_flip_normalize"], args.windows, args.inner))
        rb.append(median_ms(legs["b_paired_augment"], args.windows, args.inner))
    ma, mb = statistics.median(ra), statistics.median(rb)
    spread = (max(ra) - min(ra)) / min(ra)
    out["a_medians_ms"] = [round(v, 5) for v in ra]
    out["b_medians_ms"] = [round(v, 5) for v in rb]
    out["a_spread"] = round(spread, 4)
    out["b_over_a"] = round(mb / ma, 4)
    out["b_not_slower_than_a_within_spread"] = bool(mb <= ma * (1.0 + spread))
    ms = {"a_paired_crop_flip_normalize": ma, "b_paired_augment": mb}
    for k in ("c_maps", "d_maps_mask", "e_maps_mask_transposed", "f_torch_ops"):
        ms[k] = median_ms(legs[k], args.windows, max(5, args.inner // 5) if k == "f_torch_ops" else args.inner)
    out["ms_per_call"] = {k: round(v, 5) for k, v in ms.items()}
    out["tile_pairs_per_s"] = {k: round(B / v * 1e3) for k, v in ms.items()}
    out["algorithmic_GBps"] = {k: round(nbytes[k] / v / 1e6, 1) for k, v in ms.items()}
    out["d_speedup_over_torch_ops"] = round(ms["f_torch_ops"] / ms["d_maps_mask"], 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
