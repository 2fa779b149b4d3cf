"""Generate tests/golden/eval_steps.npz from the REFERENCE's own validation_step / test_step.

Runs only in the build container (needs the reference checkout, path in S2S_REFERENCE); the output is data only and
committed, the reference source never is.  Usage:

    python tests/golden/make_golden_eval.py

The reference's LightningModules import lightning, torchcfm, torchdyn and wandb, none of which is installed, so this
script puts small stand-ins into ``sys.modules`` before importing them:
  * ``lightning.LightningModule``: an ``nn.Module`` with a no-op ``save_hyperparameters`` and a ``log`` that records
    (key, value, flags);
  * ``torchcfm.conditional_flow_matching.ConditionalFlowMatcher``: independent coupling at sigma = 0
    (xt = t x1 + (1-t) x0, ut = x1 - x0) whose t is set by this script (recorded in the fixture);
  * ``torchdyn.core.NeuralODE`` and ``wandb``: unused placeholders.
Then the modules' own validation_step and test_step run under eval() / no_grad for three cases: the binary mask head
(conditional_flow_matching_multitask.py), the multiclass head with C = 5 and ignore_index = -100, and C = 5 with
ignore_index = 2 (conditional_flow_matching_multitask_multiclassloss.py).  Networks are tiny ([16, 32] features,
32 x 32 tiles, batch 4, time embedding 32); a few train-mode forwards first make the BatchNorm running statistics
non-trivial, and the multiclass head's 1x1 weights are scaled by 600 so that its logits
spread.  The data seed is screened so that no binary logit lies within 1e-3 of the threshold and no multiclass
argmax is within 1e-3 of a tie: the GPU's fp32 logits then give the same thresholded counts.
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("S2S_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
FEATS, HW, BATCH, TDIM, NCLS = [16, 32], 32, 4, 32, 5


class _StubLightningModule(nn.Module):
    def save_hyperparameters(self, *args, **kwargs):
        pass

    def log(self, key, value, **flags):
        self.logged.append((key, float(value), dict(flags)))


class _StubCFM:
    def __init__(self, sigma: float = 0.0):
        self.sigma = sigma
        self.t = None

    def sample_location_and_conditional_flow(self, x0, x1):
        t = self.t
        tb = t.view(-1, *([1] * (x0.dim() - 1)))
        return t, tb * x1 + (1 - tb) * x0, x1 - x0


def _install_stubs():
    light = types.ModuleType("lightning")
    light.LightningModule = _StubLightningModule
    cfm = types.ModuleType("torchcfm")
    cfm_sub = types.ModuleType("torchcfm.conditional_flow_matching")
    cfm_sub.ConditionalFlowMatcher = _StubCFM
    cfm.conditional_flow_matching = cfm_sub
    dyn = types.ModuleType("torchdyn")
    dyn_core = types.ModuleType("torchdyn.core")
    dyn_core.NeuralODE = object
    dyn.core = dyn_core
    sys.modules.update({"lightning": light, "torchcfm": cfm, "torchcfm.conditional_flow_matching": cfm_sub,
                        "torchdyn": dyn, "torchdyn.core": dyn_core, "wandb": types.ModuleType("wandb")})


def _build(kind: str, ignore_index: int):
    from src.models.components.shared_encoder import SharedEncoder
    from src.models.components.task_decoders import FlowMatchingDecoder, SegmentationDecoder
    torch.manual_seed(1984)
    enc = SharedEncoder(3, list(FEATS))
    fdec = FlowMatchingDecoder(FEATS[-1], FEATS[:-1][::-1], 3, TDIM)
    if kind == "binary":
        from src.models.conditional_flow_matching_multitask import MultiTaskFlowMatchingLitModule as M
        sdec = SegmentationDecoder(FEATS[-1], FEATS[:-1][::-1], 1)
        mod = M(enc, fdec, sdec, _StubCFM(0.0), time_emb_dim=TDIM)
    else:
        from src.models.conditional_flow_matching_multitask_multiclassloss import MultiTaskFlowMatchingLitModule as M
        sdec = SegmentationDecoder(FEATS[-1], FEATS[:-1][::-1], NCLS)
        mod = M(enc, fdec, sdec, _StubCFM(0.0), num_classes=NCLS, time_emb_dim=TDIM, ignore_index=ignore_index)
        with torch.no_grad():           # wider logit gaps: a screened draw (no near-tie argmax) exists at this size
            sdec.outc.weight.mul_(600.0)
    mod.logged = []
    # non-trivial running statistics: a few train-mode forwards of both heads
    g = torch.Generator().manual_seed(7)
    mod.train()
    with torch.no_grad():
        for _ in range(3):
            x = torch.rand(BATCH, 3, HW, HW, generator=g) * 2 - 1
            mod.forward_flow(torch.rand(BATCH, generator=g), x)
            mod.forward_segmentation(x)
    mod.eval()
    return mod


def _draw(mod, kind: str, ignore_index: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    src = torch.rand(BATCH, 3, HW, HW, generator=g) * 2 - 1
    tgt = torch.rand(BATCH, 3, HW, HW, generator=g) * 2 - 1
    t = torch.rand(BATCH, generator=g)
    with torch.no_grad():
        z = mod.forward_segmentation(src)
    if kind == "binary":
        mask = (torch.rand(BATCH, 1, HW, HW, generator=g) < 0.4).long()
        ok = bool(z.abs().min() > 1e-3)
    else:
        mask = torch.randint(0, NCLS, (BATCH, HW, HW), generator=g)
        top = z.topk(2, dim=1).values
        ok = bool((top[:, 0] - top[:, 1]).min() > 1e-3)
    return ok, src, tgt, t, mask


def main():
    sys.path.insert(0, REF)
    _install_stubs()
    out = {}
    for case, kind, ign in (("binary", "binary", -100), ("mc", "multiclass", -100), ("mc_ign", "multiclass", 2)):
        mod = _build(kind, ign)
        for seed in range(100, 400):
            ok, src, tgt, t, mask = _draw(mod, kind, ign, seed)
            if ok:
                break
        else:
            raise RuntimeError(f"{case}: no screened draw")
        mod.flow_matcher.t = t
        logs = {}
        with torch.no_grad():
            for stage, fn in (("val", mod.validation_step), ("test", mod.test_step)):
                mod.logged = []
                fn((src, tgt, mask), 0)
                logs[stage] = mod.logged
        out[f"{case}/source"] = src.numpy()
        out[f"{case}/target"] = tgt.numpy()
        out[f"{case}/mask"] = mask.numpy()
        out[f"{case}/t"] = t.numpy()
        out[f"{case}/ignore_index"] = np.array(ign)
        out[f"{case}/seed"] = np.array(seed)
        for k, v in mod.state_dict().items():
            out[f"{case}/state/{k}"] = v.detach().cpu().numpy()
        for stage, entries in logs.items():
            out[f"{case}/{stage}/keys"] = np.array(json.dumps([[k, f] for k, _, f in entries]))
            out[f"{case}/{stage}/values"] = np.array([v for _, v, _ in entries], dtype=np.float64)
        print(case, "seed", seed, {s: [(k, round(v, 6)) for k, v, _ in e] for s, e in logs.items()})
    np.savez_compressed(os.path.join(OUT, "eval_steps.npz"), **out)


if __name__ == "__main__":
    main()
