"""Cost of the EMA of the weights on one GPU (HIP events, milliseconds), one JSON line each:
  * CFMTrainer.step at 16 x 256^2 bf16 with and without ``ema_decay``, eager and ``graph=True`` (the two trainers
    alternate in rounds, so clock drift hits both alike);
  * the fused Adam + EMA kernel against the plain Adam kernel over the network's flat buffer, with the algorithmic-byte
    rate of each (Adam: read p g m v, write p m v = 28 B per parameter; + EMA: read and write the average = 36 B).
Usage: python scripts/ema_bench.py [--iters N] [--rounds R]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from stain2stain_amd import CFMTrainer, FlowUNet, ops

DEV = "cuda:0"


def timeit(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def step_times(graph, iters, rounds):
    x0 = torch.rand(16, 3, 256, 256, device=DEV) * 2 - 1
    x1 = torch.rand(16, 3, 256, 256, device=DEV) * 2 - 1
    t = torch.rand(16, device=DEV)
    trainers = {}
    for name, decay in (("off", None), ("on", 0.999)):
        torch.manual_seed(0)
        net = FlowUNet(3, [64, 128, 256, 512, 1024], 3, 256, precision="bf16").to(DEV).train()
        trainers[name] = CFMTrainer(net, graph=graph, ema_decay=decay)
    ms = {"off": [], "on": []}
    for _ in range(rounds):
        for name, tr in trainers.items():
            ms[name].append(timeit(lambda: tr.step(x0, x1, t), iters))
    for tr in trainers.values():
        tr.close()
    off, on = min(ms["off"]), min(ms["on"])
    return {"what": "cfm_step", "graph": graph, "shape": "16x256^2 bf16", "ms_ema_off": round(off, 3),
            "ms_ema_on": round(on, 3), "added_us": round((on - off) * 1e3, 1), "added_pct": round(100 * (on / off - 1), 2),
            "rounds_off": [round(x, 3) for x in ms["off"]], "rounds_on": [round(x, 3) for x in ms["on"]]}


def kernel_times(iters):
    net = FlowUNet(3, [64, 128, 256, 512, 1024], 3, 256, precision="bf16")
    n = sum(p.numel() for p in net.parameters())
    p, g, m, v = (torch.randn(n, device=DEV) * 0.01 for _ in range(4))
    v = v.abs()
    e = p.clone()
    adam = timeit(lambda: ops.adam_step_(p, g, m, v, 10, 1e-4, weight_decay=1e-5), iters)
    fused = timeit(lambda: ops.adam_ema_step_(p, g, m, v, e, 10, 1e-4, weight_decay=1e-5, ema_weight=0.001), iters)
    return {"what": "adam_kernels", "params": n, "adam_us": round(adam * 1e3, 1), "adam_TB_per_s": round(28 * n / (adam * 1e-3) / 1e12, 2),
            "adam_ema_us": round(fused * 1e3, 1), "adam_ema_TB_per_s": round(36 * n / (fused * 1e-3) / 1e12, 2),
            "added_us": round((fused - adam) * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    print(json.dumps(kernel_times(10 * a.iters)), flush=True)
    for graph in (False, True):
        print(json.dumps(step_times(graph, a.iters, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
