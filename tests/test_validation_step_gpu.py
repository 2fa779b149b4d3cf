"""MultiTaskFlowMatchingModule.validation_step / test_step against the reference's own steps
(tests/golden/eval_steps.npz, written by tests/golden/make_golden_eval.py): the logged key set and flags, the values,
no change to the module, inference mode followed by a training step, and the bf16 mode's metrics."""
import json
import os

import numpy as np
import pytest
import torch

from stain2stain_amd import (ConditionalFlowMatcher, FlowMatchingDecoder, MultiTaskFlowMatchingModule,
                             SegmentationDecoder, SharedEncoder, evaluation)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_steps.npz")
CASES = ["binary", "mc", "mc_ign"]


class FixedTimeMatcher(ConditionalFlowMatcher):
    """The fixture's recorded t instead of a draw."""

    def __init__(self, t):
        super().__init__(0.0)
        self.t = t

    def sample_location_and_conditional_flow(self, x0, x1, t=None, return_noise=False):
        return super().sample_location_and_conditional_flow(x0, x1, self.t, return_noise)


@pytest.fixture(scope="module")
def fix():
    return dict(np.load(FIX))


def build_module(fix, case, precision="fp32"):
    state = {k[len(f"{case}/state/"):]: torch.from_numpy(v) for k, v in fix.items() if k.startswith(f"{case}/state/")}
    ncls = state["seg_decoder.outc.weight"].shape[0]
    enc = SharedEncoder(3, [16, 32], precision=precision)
    fdec = FlowMatchingDecoder(32, [16], 3, 32, precision=precision)
    sdec = SegmentationDecoder(32, [16], ncls, precision=precision)
    t = torch.from_numpy(fix[f"{case}/t"]).to(DEV)
    mod = MultiTaskFlowMatchingModule(enc, fdec, sdec, FixedTimeMatcher(t), time_emb_dim=32,
                                      num_classes=None if case == "binary" else ncls,
                                      ignore_index=int(fix[f"{case}/ignore_index"]))
    mod.load_state_dict(state)
    return mod.to(DEV).eval()


def batch_of(fix, case):
    return tuple(torch.from_numpy(fix[f"{case}/{k}"]).to(DEV) for k in ("source", "target", "mask"))


def recorded(mod):
    logs = []

    def log(key, value, **flags):
        logs.append((key, value, flags))
    mod.log = log
    return logs


def snapshot(mod):
    return {k: v.detach().clone() for k, v in mod.state_dict().items()}


@pytest.mark.parametrize("case", CASES)
def test_steps_match_reference(fix, case):
    mod = build_module(fix, case)
    batch = batch_of(fix, case)
    before = snapshot(mod)
    logs = recorded(mod)
    for stage, fn in (("val", mod.validation_step), ("test", mod.test_step)):
        logs.clear()
        fn(batch, 0)
        want = json.loads(str(fix[f"{case}/{stage}/keys"]))
        assert [[k, f] for k, _, f in logs] == want
        for (key, value, _), ref in zip(logs, fix[f"{case}/{stage}/values"]):
            got = float(value)
            if key.endswith(("dice_coef", "iou")):
                assert got == float(np.float32(ref)), (key, got, ref)
            else:
                assert abs(got - ref) <= 1e-3 * max(1.0, abs(ref)), (key, got, ref)
    assert not mod.training
    after = snapshot(mod)
    assert all(torch.equal(before[k], after[k]) for k in before)


@pytest.mark.parametrize("case", ["binary", "mc"])
def test_inference_mode_then_training_step(fix, case):
    mod = build_module(fix, case)
    batch = batch_of(fix, case)
    recorded(mod)
    with torch.inference_mode():
        mod.validation_step(batch, 0)
        mod.test_step(batch, 0)
    mod.train()
    opt = torch.optim.Adam(mod.parameters(), lr=1e-4)
    loss = mod.training_step(batch, 0)
    loss.backward()
    opt.step()
    mod.eval()
    with torch.inference_mode():
        mod.validation_step(batch, 0)
    assert torch.isfinite(loss).item()


def _ref_metrics_binary(z, mask):
    pred = torch.sigmoid(z) > 0.5
    m = mask.long()
    inter = (pred * m).sum()
    dice = (2.0 * inter + 1e-7) / (pred.sum() + m.sum() + 1e-7)
    iou = (inter + 1e-7) / ((pred | m).float().sum() + 1e-7)
    return float(dice), float(iou)


def _ref_metrics_mc(z, mask, C, ignore_index):
    pred = torch.argmax(z, dim=1)
    d, i = [], []
    for c in range(C):
        if c == ignore_index:
            continue
        pc, tc = pred == c, mask == c
        inter = (pc & tc).float().sum()
        d.append((2.0 * inter + 1e-7) / (pc.float().sum() + tc.float().sum() + 1e-7))
        i.append((inter + 1e-7) / ((pc | tc).float().sum() + 1e-7))
    return float(torch.stack(d).mean()), float(torch.stack(i).mean())


@pytest.mark.parametrize("case", CASES)
def test_bf16_metrics_follow_own_logits(fix, case):
    mod = build_module(fix, case, precision="bf16")
    batch = batch_of(fix, case)
    d = mod.evaluation_values(batch)
    with torch.no_grad():
        z = evaluation.mask_logits(mod.encoder, mod.seg_decoder, batch[0]).cpu()
    mask = batch[2].cpu()
    if case == "binary":
        ref = _ref_metrics_binary(z, mask)
    else:
        ref = _ref_metrics_mc(z, mask, z.shape[1], mod.ignore_index)
    assert (float(d["dice_coef"]), float(d["iou"])) == ref
    for k in ("total", "flow", "seg"):
        assert torch.isfinite(d[k]).item()
