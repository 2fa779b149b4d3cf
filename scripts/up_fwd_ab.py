"""Up-sampling forward at the benchmark's four launches (B = 16, bf16, output in the upper half of a concat buffer, the
16^2 launch with the time bias): the register-window kernel against the row-sweep kernel it replaced, device-event time
per launch and a bit-equality check.  S2S_UP_BAND=n overrides the source rows per work item (read once per process)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stain2stain_amd import ops  # noqa: E402

REPS = 20


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def main():
    torch.manual_seed(0)
    band = os.environ.get("S2S_UP_BAND", "default")
    for B, h, C in [(16, 128, 128), (16, 64, 256), (16, 32, 512), (16, 16, 1024)]:
        x = torch.randn(B, h, h, C, device="cuda").to(torch.bfloat16)
        bias = torch.randn(B, C, device="cuda") if h == 16 else None
        cats = [torch.zeros(B, 2 * h, 2 * h, 2 * C, device="cuda", dtype=torch.bfloat16) for _ in range(2)]
        new, old = cats[0][..., C:], cats[1][..., C:]
        t_new = timed(lambda: ops.upsample2x_fwd(x, new, bias))
        t_old = timed(lambda: ops.upsample2x_fwd(x, old, bias, _reference=True))
        mb = (x.numel() + new.numel()) * 2 / 1e6
        print(f"band {band} {h}^2 C{C}: new {t_new:.1f} us ({mb / t_new:.2f} TB/s), row sweep {t_old:.1f} us "
              f"({mb / t_old:.2f} TB/s), equal {torch.equal(cats[0], cats[1])}", flush=True)


if __name__ == "__main__":
    main()
