"""Flow-matching step logic around the network, mirroring the reference's LightningModule surface.

  reference                                                               here
  ----------------------------------------------------------------------  ---------------------------
  torchcfm.ConditionalFlowMatcher.sample_location_and_conditional_flow    ConditionalFlowMatcher
    (third-party, call site src/models/conditional_flow_matching.py:66)
  ConditionalFlowMatchingLitModule.model_step / training_step /           ConditionalFlowMatchingModule
    configure_optimizers / generate (conditional_flow_matching.py:53-170)
  the ``solver:`` entry generate reads (:147-163)                         SolverConfig, _solver_setting, _solver_method
  NeuralODE(...).trajectory in generate (:157-170, torchdyn, absent)      _solve -> samplers.solve (samplers.py)

``ConditionalFlowMatchingModule`` subclasses ``lightning.LightningModule`` when Lightning is
importable and ``torch.nn.Module`` otherwise (this image has no Lightning), with the same method
names, argument meaning and return values, so the reference's training loop can drive it.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import torch

from . import evaluation, ops, samplers
from .samplers import (FIXED_STEP_METHODS, SOLVER_METHODS, GraphedVelocity, _Dopri5Graph,  # noqa: F401 -- re-exported:
                       _FixedStepGraph, _FixedStepRK, _PerSampleDopri5, _RK_TABLEAUS,     # this module was their home
                       _check_fixed_step, _eval_mode, _params, _prep_source, dopri5_generate, dopri5_integrate,
                       euler_generate, euler_integrate, fixed_step_coefficients, fixed_step_evaluations,
                       fixed_step_generate, fixed_step_integrate, fixed_step_node_times)

try:  # pragma: no cover - Lightning is not installed in the build image
    from lightning import LightningModule as _Base
except Exception:  # noqa: BLE001
    class _Base(torch.nn.Module):
        def log(self, *args, **kwargs) -> None:
            pass


class ConditionalFlowMatcher:
    """Independent-coupling conditional flow matching: xt = t x1 + (1-t) x0 + sigma eps, ut = x1 - x0."""

    def __init__(self, sigma: float = 0.0):
        self.sigma = float(sigma)

    def sample_location_and_conditional_flow(self, x0: torch.Tensor, x1: torch.Tensor,
                                             t: Optional[torch.Tensor] = None, return_noise: bool = False):
        if t is None:
            t = torch.rand(x0.shape[0], device=x0.device, dtype=torch.float32)
        eps = torch.randn_like(x0) if (self.sigma != 0.0 or return_noise) else None
        xt, ut = ops.cfm_sample(x0.contiguous().float(), x1.contiguous().float(), t.contiguous().float(),
                                self.sigma, eps)
        return (t, xt, ut, eps) if return_noise else (t, xt, ut)


class _MSE(torch.autograd.Function):
    """mean((v-u)^2) with the fused loss/gradient kernel."""

    @staticmethod
    def forward(ctx, v: torch.Tensor, u: torch.Tensor):
        loss, dv = ops.mse_loss(v.detach().contiguous(), u.detach().contiguous(), want_grad=True)
        ctx.save_for_backward(dv)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        (dv,) = ctx.saved_tensors
        return dv * gloss, None


class SolverConfig:
    """Stand-in for the reference's ``solver:`` entry (a partial of torchdyn's ``NeuralODE``,
    configs/model/conditional_flow_matching.yaml:32-38): the attributes ``generate`` reads from it."""

    def __init__(self, solver: str = "dopri5", sensitivity: str = "adjoint", atol: float = 1e-4, rtol: float = 1e-4):
        self.solver, self.sensitivity, self.atol, self.rtol = solver, sensitivity, atol, rtol


def _solver_setting(solver, name: str, default):
    """``solver.<name>`` as the reference reads it (conditional_flow_matching.py:158-163: attribute if present, else
    the default); the keyword of a ``functools.partial`` -- what Hydra's ``_partial_: true`` builds -- is honoured too."""
    if hasattr(solver, name):
        return getattr(solver, name)
    kw = getattr(solver, "keywords", None)
    if isinstance(kw, dict) and name in kw:
        return kw[name]
    return default


def _solver_method(solver, method: Optional[str] = None) -> str:
    """The solver name a ``generate`` call runs: ``method`` when given, else ``solver.solver`` (attribute or keyword of a
    partial), else dopri5; a name outside ``SOLVER_METHODS`` raises ValueError before anything touches the GPU."""
    method = method or _solver_setting(solver, "solver", "dopri5")
    if not isinstance(method, str) or method not in SOLVER_METHODS:
        raise ValueError(f"solver method must be one of {', '.join(map(repr, SOLVER_METHODS))}, got {method!r}")
    return method


def _solve(module, f, source_img: torch.Tensor, num_steps: int, method: Optional[str], atol: Optional[float],
           rtol: Optional[float], graph: bool = False, per_sample: bool = False) -> torch.Tensor:
    """The ODE solve shared by every ``generate``: like the reference it refuses to run without a solver, puts the
    module in eval mode and LEAVES it there (``self.eval()``, conditional_flow_matching.py:147-150), integrates with
    the solver's method / tolerances (dopri5, 1e-4 when it names none) and returns the end point x(1).  ``method``
    overrides the solver's choice: "euler" is the ``num_steps`` fixed-step solve of BASELINE.json configs[3], the other
    names of ``FIXED_STEP_METHODS`` ("midpoint", "heun", "rk4", "rk4_38") ``num_steps`` steps of that Runge-Kutta scheme.
    ``per_sample=True`` (dopri5 only): every sample gets its own step size, so it does not depend on its batch mates."""
    if module.solver is None:
        raise ValueError("Solver is not initialized. Cannot perform inference.")
    module.eval()
    method = _solver_method(module.solver, method)
    atol = _solver_setting(module.solver, "atol", 1e-4) if atol is None else atol
    rtol = _solver_setting(module.solver, "rtol", 1e-4) if rtol is None else rtol
    return samplers.solve(f, _prep_source(source_img), method, num_steps, atol, rtol, graph=graph,
                          per_sample=per_sample)


class ConditionalFlowMatchingModule(_Base):
    """Same surface as the reference's ConditionalFlowMatchingLitModule (logging hooks left out)."""

    def __init__(self, net: torch.nn.Module, flow_matcher: Optional[ConditionalFlowMatcher] = None, solver=None,
                 optimizer=None, scheduler=None, compile: bool = False, log_images: bool = False,
                 n_images_log: int = 5):
        super().__init__()
        self.net = net
        self.flow_matcher = flow_matcher or ConditionalFlowMatcher(0.0)
        self.solver, self.optimizer, self.scheduler = solver, optimizer, scheduler
        self.log_images, self.n_images_log = log_images, n_images_log

    def forward(self, t: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        return self.net(t, x)

    def model_step(self, batch: Tuple[torch.Tensor, ...]) -> torch.Tensor:
        x0, x1 = batch[:2]
        t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(x0, x1)
        vt = self.forward(t, xt)
        return _MSE.apply(vt, ut)

    def training_step(self, batch, batch_idx: int) -> torch.Tensor:
        loss = self.model_step(batch)
        self.log("train/loss", loss, on_step=True, on_epoch=True, prog_bar=True, sync_dist=True)
        return loss

    def validation_step(self, batch, batch_idx: int) -> None:
        self.log("val/loss", self.model_step(batch), on_step=False, on_epoch=True, prog_bar=True, sync_dist=True)

    def test_step(self, batch, batch_idx: int) -> None:
        self.log("test/loss", self.model_step(batch), on_step=False, on_epoch=True, prog_bar=True, sync_dist=True)

    def configure_optimizers(self) -> Dict[str, Any]:
        optimizer = self.optimizer(params=self.parameters())
        if self.scheduler is not None:
            return {"optimizer": optimizer,
                    "lr_scheduler": {"scheduler": self.scheduler(optimizer=optimizer), "monitor": "val/loss",
                                     "interval": "epoch", "frequency": 1}}
        return {"optimizer": optimizer}

    @torch.no_grad()
    def generate(self, source_img: torch.Tensor, num_steps: int = 100, method: Optional[str] = None,
                 atol: Optional[float] = None, rtol: Optional[float] = None, graph: bool = False,
                 per_sample: bool = False) -> torch.Tensor:
        """x(1) of dx/dt = net(t, x), x(0) = source (conditional_flow_matching.py:133-170): the solver's method --
        adaptive dopri5 at atol = rtol = 1e-4 unless ``self.solver`` says otherwise; ``num_steps`` only defined the
        reference's output grid and plays no role for the end point -- or, with ``method="euler"``, ``num_steps``
        fixed Euler steps.  Raises without a solver and leaves the module in eval mode, as the reference does.
        ``graph=True`` replays the network evaluation as a captured hipGraph (the reference samples one tile at a time,
        infer_simple_flowmatching.py:73-83, where the eager path is launch-bound).  ``per_sample=True``: dopri5 with a
        step size per sample (``dopri5_integrate``), each result independent of its batch mates."""
        return _solve(self, self.net, source_img, num_steps, method, atol, rtol, graph, per_sample)


class _WeightedMSE(torch.autograd.Function):
    """sum(w (v-u)^2) / (sum(w) + 1e-8), w = 1 + lam * mask, with the fused loss/gradient kernels."""

    @staticmethod
    def forward(ctx, v: torch.Tensor, u: torch.Tensor, mask: torch.Tensor, lam: float):
        loss, dv = ops.weighted_mse(v.detach().float(), u.detach().float(), mask.detach(), lam, want_grad=True)
        ctx.save_for_backward(dv)
        return loss[0]

    @staticmethod
    def backward(ctx, gloss):
        (dv,) = ctx.saved_tensors
        return dv * gloss, None, None, None


class ROIWeightedFlowMatchingModule(ConditionalFlowMatchingModule):
    """conditional_flow_matching_masked.py:60-91 -- batches are (source, target, mask); pixels inside the mask
    count ``1 + roi_lambda`` times in the flow-matching MSE (``roi_lambda`` attribute, default 10 as :78)."""

    roi_lambda: float = 10.0

    def model_step(self, batch) -> torch.Tensor:
        x0, x1, mask = batch
        t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(x0, x1)
        return _WeightedMSE.apply(self.forward(t, xt), ut, mask, float(getattr(self, "roi_lambda", 10.0)))


class ROICharbonnierFlowMatchingModule(ConditionalFlowMatchingModule):
    """conditional_flow_matching_ROI_loss.py:64-97 -- flow-matching MSE plus ``lambda_roi`` times the Charbonnier
    distance between xt and x1 inside the mask (a data-only term: it shifts the logged loss, not the gradients)."""

    lambda_roi: float = 1.0

    def model_step(self, batch) -> torch.Tensor:
        x0, x1, mask = batch
        t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(x0, x1)
        loss_fm = _MSE.apply(self.forward(t, xt), ut)
        roi = ops.charbonnier_roi(xt, x1.float(), mask, 1e-3, 1e-8)[0]
        return loss_fm + float(getattr(self, "lambda_roi", 1.0)) * roi


class MaskConditionedFlowMatchingModule(ConditionalFlowMatchingModule):
    """conditional_flow_matching_conditional_mask.py:54-82 (``mask_toggle=False``) and
    conditional_flow_matching_conditional_toggle_mask.py:54-103 (``mask_toggle=True``: the training step zeroes the
    mask with probability 1/2, drawn with ``torch.rand(1).item()`` like the reference).  The mask is the fourth
    input channel of ``net`` (``in_channels: 4``)."""

    def __init__(self, *args, mask_toggle: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.mask_toggle = mask_toggle

    def forward(self, t: torch.Tensor, x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        return self.net(t, torch.cat([x, mask.to(x.dtype)], dim=1))

    def model_step(self, batch, use_mask_toggle: bool = False) -> torch.Tensor:
        x0, x1, mask = batch
        if use_mask_toggle and torch.rand(1).item() < 0.5:
            mask = torch.zeros_like(mask)
        t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(x0, x1)
        return _MSE.apply(self.forward(t, xt, mask), ut)

    def training_step(self, batch, batch_idx: int) -> torch.Tensor:
        loss = self.model_step(batch, use_mask_toggle=self.mask_toggle)
        self.log("train/loss", loss, on_step=True, on_epoch=True, prog_bar=True, sync_dist=True)
        return loss

    @torch.no_grad()
    def generate(self, source_img: torch.Tensor, mask: torch.Tensor, num_steps: int = 100,
                 method: Optional[str] = None, atol: Optional[float] = None, rtol: Optional[float] = None,
                 per_sample: bool = False) -> torch.Tensor:
        """conditional_flow_matching_conditional_mask.py:143-199: the mask rides along as a constant fourth channel."""
        if source_img.dim() == 3:
            source_img, mask = source_img.unsqueeze(0), mask.unsqueeze(0)
        return _solve(self, lambda t, x: self.forward(t, x, mask), source_img, num_steps, method, atol, rtol,
                      per_sample=per_sample)


class ClassConditionalFlowMatchingModule(ConditionalFlowMatchingModule):
    """class_conditional_flow_matching.py:39-71,130-190 -- batches are (source, target, target_label); the label
    conditions the network call ``net(t, x, y=y)``; ``generate(source, target_class, num_steps)``."""

    def forward(self, t: torch.Tensor, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return self.net(t, x, y=y)

    def model_step(self, batch) -> torch.Tensor:
        x0, x1, label = batch
        t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(x0, x1)
        return _MSE.apply(self.forward(t, xt, label.long()), ut)

    @torch.no_grad()
    def generate(self, source_img: torch.Tensor, target_class, num_steps: int = 100, method: Optional[str] = None,
                 atol: Optional[float] = None, rtol: Optional[float] = None, per_sample: bool = False) -> torch.Tensor:
        """class_conditional_flow_matching.py:130-190: ``target_class`` an int or a [B] tensor."""
        if source_img.dim() == 3:
            source_img = source_img.unsqueeze(0)
        B, dev = source_img.shape[0], source_img.device
        y = (torch.tensor([target_class] * B, device=dev) if isinstance(target_class, int)
             else target_class.to(dev))

        def f(t, x):
            return self.net(t, x, y=(y.expand(x.shape[0]) if y.dim() == 0 else y[:x.shape[0]]))

        return _solve(self, f, source_img, num_steps, method, atol, rtol, per_sample=per_sample)


class _SegLoss(torch.autograd.Function):
    """dw * Dice(sigmoid(z), g) + (1-dw) * BCEWithLogits(z, g) with the fused two-pass kernel."""

    @staticmethod
    def forward(ctx, z: torch.Tensor, g: torch.Tensor, smooth: float, dice_weight: float):
        out, dz = ops.seg_loss(z.detach().float(), g.detach(), smooth, dice_weight, want_grad=True)
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(out[1], out[2])
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, gseg, gdice, gbce):
        (dz,) = ctx.saved_tensors
        return dz * gseg, None, None, None


class _SegLossMulticlass(torch.autograd.Function):
    """dw * softmax-Dice + (1-dw) * CrossEntropy on class-index targets."""

    @staticmethod
    def forward(ctx, z: torch.Tensor, target: torch.Tensor, ignore_index: int, smooth: float, dice_weight: float):
        out, dz = ops.seg_loss_multiclass(z.detach().float(), target, ignore_index, smooth, dice_weight,
                                          want_grad=True)
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(out[1], out[2])
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, gseg, gdice, gce):
        (dz,) = ctx.saved_tensors
        return dz * gseg, None, None, None, None


class MultiTaskFlowMatchingModule(_Base):
    """Same surface as the reference's MultiTaskFlowMatchingLitModule
    (src/models/conditional_flow_matching_multitask.py:57-257,391-417): shared encoder, flow head A, mask head B,
    L = L_FM + seg_loss_weight * (dice_weight * Dice + (1 - dice_weight) * BCE).  Logging hooks left out."""

    def __init__(self, encoder, flow_decoder, seg_decoder, flow_matcher: Optional[ConditionalFlowMatcher] = None,
                 solver=None, optimizer=None, scheduler=None, compile: bool = False, log_images: bool = False,
                 seg_loss_weight: float = 1.0, dice_weight: float = 0.5, n_images_log: int = 5,
                 time_emb_dim: int = 256, num_classes: Optional[int] = None, ignore_index: int = -100):
        """``num_classes`` None: binary mask head, Dice + BCE (conditional_flow_matching_multitask.py).  An integer
        selects the multiclass form, softmax Dice + CrossEntropy on class-index masks
        (conditional_flow_matching_multitask_multiclassloss.py:92-159)."""
        super().__init__()
        self.num_classes, self.ignore_index = num_classes, ignore_index
        from .components import TimeEmbedding
        self.encoder, self.flow_decoder, self.seg_decoder = encoder, flow_decoder, seg_decoder
        self.time_embedding = TimeEmbedding(time_emb_dim)
        self.flow_matcher = flow_matcher or ConditionalFlowMatcher(0.0)
        self.solver, self.optimizer, self.scheduler = solver, optimizer, scheduler
        self.seg_loss_weight, self.dice_weight = seg_loss_weight, dice_weight
        self.dice_smooth = 1.0

    def forward_flow(self, t: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        bottleneck, skips = self.encoder(x)
        return self.flow_decoder(bottleneck, skips, self.time_embedding(t))

    def forward_segmentation(self, x: torch.Tensor) -> torch.Tensor:
        bottleneck, skips = self.encoder(x)
        return self.seg_decoder(bottleneck, skips)

    def compute_segmentation_loss(self, pred_mask: torch.Tensor, target_mask: torch.Tensor):
        if self.num_classes is not None:
            if target_mask.dim() == 4 and target_mask.shape[1] == 1:
                target_mask = target_mask.squeeze(1)
            seg, dice, ce = _SegLossMulticlass.apply(pred_mask, target_mask.long(), self.ignore_index,
                                                     self.dice_smooth, self.dice_weight)
            return seg, {"dice": dice, "ce": ce, "seg_total": seg}
        seg, dice, bce = _SegLoss.apply(pred_mask, target_mask.float(), self.dice_smooth, self.dice_weight)
        return seg, {"dice": dice, "bce": bce, "seg_total": seg}

    def model_step(self, batch):
        source_img, target_img, gt_mask = batch
        t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(source_img, target_img)
        flow_loss = _MSE.apply(self.forward_flow(t, xt), ut)
        seg_loss, d = self.compute_segmentation_loss(self.forward_segmentation(source_img), gt_mask)
        total = flow_loss + self.seg_loss_weight * seg_loss
        second = "ce" if self.num_classes is not None else "bce"
        return total, {"total": total, "flow": flow_loss, "seg": seg_loss, "seg_dice": d["dice"],
                       "seg_" + second: d[second]}

    def training_step(self, batch, batch_idx: int) -> torch.Tensor:
        loss, d = self.model_step(batch)
        for k, v in d.items():
            self.log(f"train/{k}_loss", v, on_step=True, on_epoch=True, prog_bar=(k == "total"), sync_dist=True)
        return loss

    # the reference's validation / test logging: (key suffix, value key, prog_bar); every call is on_step=False,
    # on_epoch=True, sync_dist=True (conditional_flow_matching_multitask.py:306-343, 359-381,
    # conditional_flow_matching_multitask_multiclassloss.py:348-371, 424-476)
    _LOSS_KEYS = (("loss", "total", True), ("flow_loss", "flow", False), ("seg_loss", "seg", True))
    _METRIC_KEYS = (("dice_coef", "dice_coef", True), ("iou", "iou", True))

    def _log_keys(self, stage: str):
        keys = list(self._LOSS_KEYS)
        if stage == "val":
            second = "seg_ce" if self.num_classes is not None else "seg_bce"
            keys += [("seg_dice", "seg_dice", False), (second, second, False)]
            if self.num_classes is None:         # the multiclass reference has its validation metrics commented out
                keys += list(self._METRIC_KEYS)
        else:
            keys += list(self._METRIC_KEYS)
        return keys

    def evaluation_values(self, batch) -> Dict[str, torch.Tensor]:
        """Every value of the validation / test steps for one batch as device scalars: {"total", "flow", "seg",
        "seg_dice", "seg_bce" | "seg_ce", "dice_coef", "iou"}.  The networks run in the mode they are in (Lightning sets
        eval mode: BatchNorm from the running statistics), through the forward-only head + MSE and segmentation
        metric kernels; the mask head runs once (the reference's second forward_segmentation is the same in eval mode)."""
        source_img, target_img, gt_mask = batch
        with evaluation.eval_grad_mode():
            t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(source_img, target_img)
            return evaluation.multitask_values(
                self.encoder, self.flow_decoder, self.seg_decoder, self.time_embedding.dim, source_img, xt, t, ut,
                gt_mask, self.num_classes, self.ignore_index, self.dice_smooth, self.dice_weight, self.seg_loss_weight)

    def _eval_step(self, batch, stage: str) -> None:
        d = self.evaluation_values(batch)
        for suffix, key, bar in self._log_keys(stage):
            self.log(f"{stage}/{suffix}", d[key], on_step=False, on_epoch=True, prog_bar=bar, sync_dist=True)

    def validation_step(self, batch, batch_idx: int) -> None:
        self._eval_step(batch, "val")

    def test_step(self, batch, batch_idx: int) -> None:
        self._eval_step(batch, "test")

    def configure_optimizers(self) -> Dict[str, Any]:
        params = (list(self.encoder.parameters()) + list(self.flow_decoder.parameters())
                  + list(self.seg_decoder.parameters()))
        optimizer = self.optimizer(params=params)
        if self.scheduler is not None:
            return {"optimizer": optimizer,
                    "lr_scheduler": {"scheduler": self.scheduler(optimizer=optimizer), "monitor": "val/loss",
                                     "interval": "epoch", "frequency": 1}}
        return {"optimizer": optimizer}

    @torch.no_grad()
    def generate(self, source_img: torch.Tensor, num_steps: int = 100, method: Optional[str] = None,
                 atol: Optional[float] = None, rtol: Optional[float] = None, per_sample: bool = False):
        """(generated image, mask probabilities / class map) like the reference's generate (:419-484): the module goes
        to eval mode and stays there, the mask head runs once on the source, the flow is integrated with the solver's
        method (dopri5 at 1e-4 by default; ``method="euler"`` = ``num_steps`` fixed steps)."""
        if self.solver is None:
            raise ValueError("Solver is not initialized. Cannot perform inference.")
        self.eval()
        if source_img.dim() == 3:
            source_img = source_img.unsqueeze(0)
        logits = self.forward_segmentation(source_img)
        if self.num_classes is not None:       # class map, as the multiclass reference returns (:536-537)
            pred_mask = torch.argmax(torch.softmax(logits, dim=1), dim=1, keepdim=True)
        else:
            pred_mask = torch.sigmoid(logits)
        return (_solve(self, self.forward_flow, source_img, num_steps, method, atol, rtol, per_sample=per_sample),
                pred_mask)
