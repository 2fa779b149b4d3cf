"""Measurement for DESIGN.md 3.18: Macenko stain normalisation, fit and apply, against the same definition composed
from torch ops on the GPU (table gathers, matmuls, masks, bincounts: every intermediate goes through memory), on an N^2
device region and on a 32 x 256^2 batch of synthetic H&E, with ``stain_quantify`` on the same bytes as the comparable
bandwidth-bound kernel of section 3.17.

    python scripts/stain_norm_bench.py [--only fused|torch] [--iters 20] [--region 4096]

Times are HIP-event medians over ``--iters`` calls after a warm-up.  GB/s are against the algorithmic traffic: a fit
reads the bytes three times (9 B per pixel), each of its passes 3 B; apply reads 3 B and writes 3 B (uint8) or 12 B
(fp32).  A fit also waits for three small read-backs and an eigen-decomposition on the host, which its time includes;
the three passes are timed on their own as well.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stain2stain_amd import REFERENCE_HE, fit_stains, normalize_region, stain_normalize, stain_quantify  # noqa: E402
from stain2stain_amd.stain_norm import (CONC_MAX, NB, angle_histogram, concentration_histogram, max_conc_from_histograms,  # noqa: E402
                                        moments, q_table, u_beta, vectors_from_histogram)
from stain2stain_amd.stain_quant import od_table, unmix_matrix  # noqa: E402


def synthetic_he(shape, dev, seed=0):
    """uint8 [..., H, W, 3]: gamma-distributed haematoxylin and eosin concentrations, a quarter bare glass."""
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


def torch_fit(u8, alpha=1.0, beta=0.15, pct=99.0):
    """fit_stains from torch ops alone (fp32; matmuls may contract, so a bin can differ by pixels on an edge)."""
    dev = u8.device
    px = u8.reshape(-1, 3)
    keep = px.amax(-1) <= u_beta(beta)
    idx = px[keep].long()
    q = q_table().to(dev).long()[idx]
    n = q.shape[0]
    s1 = q.sum(0).double()
    s2 = (q.double().T @ q.double())
    cov = (s2 / n - torch.outer(s1, s1) / n ** 2) / 2.0 ** 24
    w, v = torch.linalg.eigh(cov.cpu())
    v1, v2 = v[:, 2], v[:, 1]
    v1 = -v1 if v1.sum() < 0 else v1
    v2 = -v2 if v2[v2.abs().argmax()] < 0 else v2
    plane = torch.stack([v1, v2], 1).float()
    od = od_table().to(dev)[idx]
    xy = od @ plane.to(dev)
    d = xy.abs().sum(1)
    s = xy[:, 1] / d
    bins = ((s + 1) * (NB / 2)).floor().clamp(0, NB - 1).long()[d != 0]
    vectors = vectors_from_histogram(torch.bincount(bins, minlength=NB).cpu(), plane, alpha)
    c = od @ unmix_matrix(vectors).to(dev)[:, :2]
    cb = (c * (NB / CONC_MAX)).floor().clamp(0, NB - 1).long()
    hists = torch.stack([torch.bincount(cb[:, k], minlength=NB) for k in range(2)]).cpu()
    return vectors, max_conc_from_histograms(hists, pct)


def torch_apply(u8, fit, reference=REFERENCE_HE):
    dev = u8.device
    od = od_table().to(dev)[u8.long()]
    c = od @ unmix_matrix(fit.vectors).to(dev)[:, :2]
    c = c * (reference.max_conc / fit.max_conc).float().to(dev)
    od2 = c @ reference.vectors.float().to(dev)
    return (255.0 * torch.exp2(od2 * -3.321928094887362)).round().clamp(0, 255).to(torch.uint8)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["fused", "torch"], default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--region", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    n = args.region
    inputs = {f"region_{n}": synthetic_he((n, n), dev, 1), "batch_32x256": synthetic_he((32, 256, 256), dev, 2)}
    out = {}

    def rate(key, ms, nbytes):
        out[key + "_ms"] = round(ms, 4)
        out[key + "_GBps"] = round(nbytes / ms / 1e6, 1)

    for name, img in inputs.items():
        px = img.numel() // 3
        batch = img if img.dim() == 4 else img[None]
        fit = fit_stains(img)
        if args.only in (None, "fused"):
            rate(f"{name}_fit", timed(lambda: fit_stains(img), args.iters), 9 * px)
            rate(f"{name}_moments", timed(lambda: moments(img), args.iters), 3 * px)
            rate(f"{name}_angle_hist", timed(lambda: angle_histogram(img, fit.plane), args.iters), 3 * px)
            rate(f"{name}_conc_hist", timed(lambda: concentration_histogram(img, fit.vectors), args.iters), 3 * px)
            apply = (lambda: stain_normalize(img, fit)) if img.dim() == 4 else (lambda: normalize_region(img, fit))
            rate(f"{name}_apply_u8", timed(apply, args.iters), 6 * px)
            rate(f"{name}_apply_f32", timed(lambda: stain_normalize(batch, fit, network_input=True), args.iters), 15 * px)
            rate(f"{name}_stain_quantify", timed(lambda: stain_quantify(batch), args.iters), 3 * px)
        if args.only in (None, "torch"):
            it = max(3, args.iters // 4)
            out[f"{name}_torch_fit_ms"] = round(timed(lambda: torch_fit(img), it), 4)
            out[f"{name}_torch_apply_ms"] = round(timed(lambda: torch_apply(img, fit), it), 4)
            tv, tc = torch_fit(img)
            out[f"{name}_torch_vs_fused_vector_maxdiff"] = float((tv - fit.vectors).abs().max())
            out[f"{name}_torch_vs_fused_max_conc_maxdiff"] = float((tc - fit.max_conc).abs().max())
            diff = (torch_apply(img, fit).int() - stain_normalize(batch, fit).reshape(img.shape).int()).abs()
            out[f"{name}_torch_vs_fused_apply_maxdiff"] = int(diff.max())
        if args.only is None:
            out[f"{name}_fit_speedup"] = round(out[f"{name}_torch_fit_ms"] / out[f"{name}_fit_ms"], 1)
            out[f"{name}_apply_speedup"] = round(out[f"{name}_torch_apply_ms"] / out[f"{name}_apply_u8_ms"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
