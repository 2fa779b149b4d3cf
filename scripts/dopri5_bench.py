"""Batch-wide vs per-sample dopri5 on the default FlowUNet (bf16, 256 x 256), DESIGN.md section 3.12.

For each batch size the same inputs are solved by turns with
  wide      dopri5_generate(net, x, graph=True)              (today's API: captures the forward on every call)
  wide_c    the same loop on one GraphedVelocity kept across calls (the batch-wide solver without its capture cost)
  per       dopri5_generate(net, x, per_sample=True, graph=True)  (cached capture of a whole attempted step)
and one JSON line per (batch, mode) reports ms per solve (median), attempted steps, ms per attempted step, network
evaluations and, for the per-sample mode, attempted steps per tile (min / median / max).

Kernel times: run once more under ``rocprofv3 --kernel-trace --stats -- python scripts/dopri5_bench.py --reps 1`` and
read the s2s dp_* kernels against axpy_kernel / ode_err_* in the stats file."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1984)
    a = ap.parse_args()
    from stain2stain_amd import FlowUNet, dopri5_generate, dopri5_integrate
    from stain2stain_amd.samplers import GraphedVelocity, _eval_mode, _prep_source
    torch.manual_seed(a.seed)
    net = FlowUNet(precision="bf16").cuda().eval()

    def wide_cached(gv, x):
        with _eval_mode(net):
            return dopri5_integrate(lambda t, y: gv(t, y).clone(), _prep_source(x), return_stats=True)

    for B in [int(v) for v in a.batches.split(",")]:
        g = torch.Generator().manual_seed(a.seed + B)
        x = (torch.rand(B, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
        gv = GraphedVelocity(net, _prep_source(x), None)
        modes = {"wide": lambda: dopri5_generate(net, x, return_stats=True, graph=True),
                 "wide_c": lambda: wide_cached(gv, x),
                 "per": lambda: dopri5_generate(net, x, return_stats=True, graph=True, per_sample=True)}
        for fn in modes.values():                         # warm-up (captures, packed weights)
            fn()
        times = {k: [] for k in modes}
        stats = {}
        for _ in range(a.reps):                           # alternate the modes within one run
            for k, fn in modes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, st = fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
                stats[k] = st
        gv.close()
        for k in modes:
            st = stats[k]
            attempted = st["attempted"] if k == "per" else st["accepted"] + st["rejected"]
            ms = statistics.median(times[k])
            row = {"batch": B, "mode": k, "ms_per_solve": round(ms, 3), "ms_min": round(min(times[k]), 3),
                   "attempted": attempted, "ms_per_attempted_step": round(ms / max(attempted, 1), 3),
                   "evaluations": 2 + 6 * attempted}
            if k == "per":
                per_tile = [x + y for x, y in zip(st["accepted"], st["rejected"])]
                row["tile_steps_min_median_max"] = [min(per_tile), statistics.median(per_tile), max(per_tile)]
                row["host_reads"] = st["host_reads"]
            print(json.dumps(row), flush=True)
        net._s2s_dopri5_graph.close()


if __name__ == "__main__":
    main()
