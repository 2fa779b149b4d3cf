"""Evaluation-pass timings on one GPU (HIP events, milliseconds per batch), one JSON line each:
  * CFMTrainer.evaluate at 16 x 256^2 bf16 next to CFMTrainer.step on the same box;
  * MultiTaskTrainer.evaluate (binary mask head) at 8 x 512^2 bf16, next to its step;
  * the forward-only head + MSE kernel (64 -> 3, 16 x 256^2, bf16 activation) and its algorithmic-byte rate, next to
    head_fwd + mse_loss.
Usage: python scripts/eval_bench.py [--iters N]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from stain2stain_amd import (CFMTrainer, FlowMatchingDecoder, FlowUNet, MultiTaskTrainer, SegmentationDecoder,
                             SharedEncoder, ops)

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    torch.manual_seed(0)

    # CFM at the benchmark's shape
    net = FlowUNet(3, [64, 128, 256, 512, 1024], 3, 256, precision="bf16").to(DEV).train()
    tr = CFMTrainer(net)
    x0 = torch.rand(16, 3, 256, 256, device=DEV) * 2 - 1
    x1 = torch.rand(16, 3, 256, 256, device=DEV) * 2 - 1
    t = torch.rand(16, device=DEV)
    step_ms = timeit(lambda: tr.step(x0, x1, t), a.iters)
    eval_ms = timeit(lambda: tr.evaluate(x0, x1, t), a.iters)
    print(json.dumps({"what": "cfm", "shape": "16x256^2 bf16", "step_ms": round(step_ms, 3),
                      "evaluate_ms": round(eval_ms, 3), "ratio": round(eval_ms / step_ms, 3)}))
    tr.close()
    del tr, net

    # multitask (binary mask head) at 8 x 512^2
    feats = [64, 128, 256, 512, 1024]
    enc = SharedEncoder(3, feats).to(DEV).train()
    fdec = FlowMatchingDecoder(1024, feats[:-1][::-1], 3, 256).to(DEV).train()
    sdec = SegmentationDecoder(1024, feats[:-1][::-1], 1).to(DEV).train()
    mt = MultiTaskTrainer(enc, fdec, sdec)
    s = torch.rand(8, 3, 512, 512, device=DEV) * 2 - 1
    g = torch.rand(8, 3, 512, 512, device=DEV) * 2 - 1
    m = (torch.rand(8, 1, 512, 512, device=DEV) < 0.3).float()
    tm = torch.rand(8, device=DEV)
    mstep = timeit(lambda: mt.step(s, g, m, tm), max(3, a.iters // 2))
    meval = timeit(lambda: mt.evaluate(s, g, m, tm), max(3, a.iters // 2))
    print(json.dumps({"what": "multitask", "shape": "8x512^2 bf16 binary", "step_ms": round(mstep, 3),
                      "evaluate_ms": round(meval, 3), "ratio": round(meval / mstep, 3)}))
    mt.close()
    del mt, enc, fdec, sdec

    # the head + MSE kernel alone
    B, H, W, C, cout = 16, 256, 256, 64, 3
    x = (torch.randn(B, H, W, C, device=DEV)).to(torch.bfloat16)
    w = torch.randn(cout, C, device=DEV) / 8
    b = torch.randn(cout, device=DEV)
    u = torch.randn(B, cout, H, W, device=DEV)
    k_ms = timeit(lambda: ops.head_mse_eval(x, w, b, u), 10 * a.iters)
    two_ms = timeit(lambda: ops.mse_loss(ops.head_fwd(x, w, b), u, want_grad=False), 10 * a.iters)
    nbytes = B * H * W * (C * 2 + cout * 4)
    print(json.dumps({"what": "head_mse_eval", "shape": "16x256^2x64->3 bf16", "us": round(k_ms * 1e3, 1),
                      "TB_per_s": round(nbytes / (k_ms * 1e-3) / 1e12, 2),
                      "head_fwd_plus_mse_us": round(two_ms * 1e3, 1)}))


if __name__ == "__main__":
    main()
