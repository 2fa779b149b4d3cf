"""Validation / test passes of the flow-matching models and their epoch accumulation.

  reference                                                                  here
  -------------------------------------------------------------------------  --------------------------------------
  MultiTaskFlowMatchingLitModule.validation_step / test_step                 flow_matching.MultiTaskFlowMatchingModule
    (conditional_flow_matching_multitask.py:297-389,                           .validation_step / .test_step, and
     conditional_flow_matching_multitask_multiclassloss.py:339-476)            MultiTaskTrainer.evaluate
  ConditionalFlowMatchingLitModule.validation_step (model_step's loss)       CFMTrainer.evaluate
  self.log(..., on_epoch=True, sync_dist=True) epoch means                   EvalAccumulator

An evaluation pass runs the network forward in the mode its modules are in (eval mode: BatchNorm from the running
statistics, folded into the convolution epilogue), then the forward-only flow head + MSE kernel and the one-pass
segmentation loss + metric kernel (csrc/eval_metrics.hip).  It writes no gradient, no optimiser state and, in eval mode,
no running statistic, and it never waits for the device.
"""
from __future__ import annotations

import contextlib
import types
from typing import Dict, Iterable, Optional

import torch
import torch.distributed as dist

from . import engine, ops
from .ddp import _active


@contextlib.contextmanager
def eval_grad_mode():
    """No autograd and NOT inference mode, whatever the caller runs under (Lightning 2 validates inside
    ``torch.inference_mode()``): tensors an evaluation pass caches for later -- folded BatchNorm tables, packed weights,
    workspaces -- must stay ordinary tensors, or the next training step that updates them in place would raise."""
    with torch.inference_mode(False), torch.no_grad():
        yield


def flow_loss(encoder, flow_decoder, time_dim: int, xt: torch.Tensor, t: torch.Tensor, ut: torch.Tensor,
              encoder_training: bool = False, decoder_training: bool = False) -> torch.Tensor:
    """mean((flow_decoder(encoder(xt), t) - ut)^2) as a device scalar; the head + MSE never materialise v."""
    dt = encoder.compute_dtype
    ectx = engine.encoder_forward(encoder._blocks, xt.float().contiguous(), dt, encoder_training)
    feats = ectx.feats
    temb = ops.time_embedding(t.float().contiguous(), time_dim)
    dctx = engine.decoder_forward(flow_decoder, feats[-1], feats[:-1][::-1], temb, dt, decoder_training,
                                  with_head=False)
    outc = flow_decoder.outc
    return ops.head_mse_eval(dctx.lows[-1], outc.weight, outc.bias, ut)


def mask_logits(encoder, seg_decoder, source: torch.Tensor, encoder_training: bool = False,
                decoder_training: bool = False) -> torch.Tensor:
    dt = encoder.compute_dtype
    ectx = engine.encoder_forward(encoder._blocks, source.float().contiguous(), dt, encoder_training)
    feats = ectx.feats
    return engine.decoder_forward(seg_decoder, feats[-1], feats[:-1][::-1], None, dt, decoder_training).v


class GenerationEval:
    """What a trainer's ``evaluate_generation`` keeps between calls: per network (live / EMA) the eval-mode velocity
    ``f(t, x)`` and the holder its captured sampler step is cached on (``samplers._GraphedStep.cached`` matches a capture
    on the callable's identity, so the callable has to persist).  The velocity runs the engine forward with
    ``training=False`` -- BatchNorm from the running statistics -- whatever mode the modules are in, so no module mode
    is touched.  A capture is rebuilt when ``engine.mutation_epoch`` moves, which every optimiser step does."""

    def __init__(self):
        self._slots = {}

    def velocity(self, key, encoder, flow_decoder, time_dim: int):
        slot = self._slots.get(key)
        if slot is None or slot[2] is not encoder or slot[3] is not flow_decoder:
            if slot is not None:
                self._close(slot[1])

            def f(t: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
                dt = encoder.compute_dtype
                if t.dim() == 0 or t.shape[0] != x.shape[0]:
                    t = t.reshape(-1)[:1].expand(x.shape[0])
                feats = engine.encoder_forward(encoder._blocks, x.float().contiguous(), dt, False).feats
                temb = ops.time_embedding(t.float().contiguous(), time_dim)
                return engine.decoder_forward(flow_decoder, feats[-1], feats[:-1][::-1], temb, dt, False).v

            slot = self._slots[key] = (f, types.SimpleNamespace(), encoder, flow_decoder)
        return slot[0], slot[1]

    @staticmethod
    def _close(holder) -> None:
        from . import samplers
        samplers.close_cached(holder)

    def holders(self):
        """The objects the captured steps are cached on, one per network used so far."""
        return [slot[1] for slot in self._slots.values()]

    def close(self) -> None:
        for slot in self._slots.values():
            self._close(slot[1])
        self._slots.clear()


def generation_values(state: GenerationEval, key, encoder, flow_decoder, time_dim: int, x0: torch.Tensor,
                      x1: torch.Tensor, num_steps: int, method: str, graph: bool, quantize: bool,
                      accumulator: Optional["EvalAccumulator"], stain: Optional[dict] = None) -> Dict[str, torch.Tensor]:
    """``x0`` carried to t = 1 by ``samplers.solve`` on the eval-mode network, scored against ``x1``
    (``image_metrics.image_quality``): the per-sample {"psnr", "ssim", "mae", "mse"}.  ``method="dopri5"`` runs the
    per-sample controller (``per_sample=True``, as ``region.multitask_sampler`` does), so that a sample's score does not
    depend on its batch mates, at the default tolerances; ``num_steps`` plays no role then.  ``stain`` (a dict of
    ``stain_quant.stain_agreement``'s arguments) adds "stain/burden_abs_err", "stain/dice" and "stain/iou".  The caller
    sets the workspace owner and the grad mode."""
    from . import image_metrics, samplers, stain_quant
    if method not in samplers.SOLVER_METHODS:
        raise ValueError(f"method must be one of {', '.join(map(repr, samplers.SOLVER_METHODS))}, got {method!r}")
    f, holder = state.velocity(key, encoder, flow_decoder, time_dim)
    x = samplers._prep_source(x0)
    pred = samplers.solve(f, x, method, num_steps, graph=graph, per_sample=method == "dopri5",
                          cache_on=holder if graph else None)
    target = x1.detach().float().contiguous()
    values = image_metrics.image_quality(pred, target, quantize=quantize)
    if stain is not None:
        values.update(stain_quant.agreement_values(pred, target, stain))
    if accumulator is not None:
        accumulator.add({k: v.mean() for k, v in values.items()}, int(x.shape[0]))
    return values


def segmentation_values(logits: torch.Tensor, mask: torch.Tensor, num_classes: Optional[int], ignore_index: int,
                        dice_smooth: float, dice_weight: float) -> Dict[str, torch.Tensor]:
    """{"seg", "seg_dice", "seg_bce" | "seg_ce", "dice_coef", "iou"} of one batch (device scalars): the loss terms of
    compute_segmentation_loss and the metrics of test_step (the binary validation_step's too)."""
    if num_classes is not None:
        out, _ = ops.seg_eval_multiclass(logits, mask, ignore_index, dice_smooth, dice_weight)
        second = "seg_ce"
    else:
        g = mask if mask.dtype in (torch.float32, torch.uint8, torch.bool) else mask.float()
        out, _ = ops.seg_eval_binary(logits, g.reshape(logits.shape), dice_smooth, dice_weight)
        second = "seg_bce"
    return {"seg": out[0], "seg_dice": out[1], second: out[2], "dice_coef": out[3], "iou": out[4]}


def multitask_values(encoder, flow_decoder, seg_decoder, time_dim: int, source: torch.Tensor, xt: torch.Tensor,
                     t: torch.Tensor, ut: torch.Tensor, mask: torch.Tensor, num_classes: Optional[int],
                     ignore_index: int, dice_smooth: float, dice_weight: float,
                     seg_loss_weight: float) -> Dict[str, torch.Tensor]:
    """Every value the multitask validation / test steps log, keyed like the reference's loss_dict plus the metrics:
    {"total", "flow", "seg", "seg_dice", "seg_bce" | "seg_ce", "dice_coef", "iou"}.  The encoder runs on xt, then on the
    source (the reference's order, which matters for its running statistics in train mode); the mask head runs once."""
    flow = flow_loss(encoder, flow_decoder, time_dim, xt, t, ut, encoder.training, flow_decoder.training)
    logits = mask_logits(encoder, seg_decoder, source, encoder.training, seg_decoder.training)
    d = segmentation_values(logits, mask, num_classes, ignore_index, dice_smooth, dice_weight)
    d["flow"] = flow
    d["total"] = flow + float(seg_loss_weight) * d["seg"]
    return d


class EvalAccumulator:
    """Epoch means of per-batch evaluation values, kept on the device.

    ``add(values, batch_size)`` adds ``batch_size * value`` to an fp64 sum per key and ``batch_size`` to the count:
    a stack, a cast and two in-place adds on tiny tensors, no host synchronisation.  ``compute(process_group)`` packs
    the sums and the count into one tensor, all-reduces it (SUM) once over the group when torch.distributed is running
    with more than one rank, and divides: the result is the batch-size-weighted mean over every batch of every rank.
    That is what Lightning logs for ``self.log(key, value, on_epoch=True, sync_dist=True)`` with its default mean
    reduction (the weighted sum and the summed batch sizes are each reduced over the ranks before the division).
    Every rank must call ``compute`` and hold the same keys: pass ``keys`` (and ``device``) up front when a rank may see
    no batch at all."""

    def __init__(self, keys: Optional[Iterable[str]] = None, device=None):
        self._keys = sorted(keys) if keys is not None else None
        self._device = torch.device(device) if device is not None else None
        self._buf: Optional[torch.Tensor] = None       # fp64 [len(keys) sums | count]

    @property
    def keys(self):
        return list(self._keys) if self._keys is not None else []

    def _ensure(self, device) -> torch.Tensor:
        if self._buf is None:
            self._device = self._device or device
            self._buf = torch.zeros(len(self._keys) + 1, dtype=torch.float64, device=self._device)
        return self._buf

    def add(self, values: Dict[str, torch.Tensor], batch_size: int) -> None:
        if self._keys is None:
            self._keys = sorted(values)
        if sorted(values) != self._keys:
            raise KeyError(f"EvalAccumulator holds {self._keys}, got {sorted(values)}")
        if int(batch_size) <= 0:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        dev = next((v.device for v in values.values() if torch.is_tensor(v)), self._device or torch.device("cpu"))
        with eval_grad_mode():         # (the buffer is updated in place across modes)
            buf = self._ensure(dev)
            vec = torch.stack([torch.as_tensor(values[k], device=buf.device).detach().reshape(()).to(torch.float32)
                               for k in self._keys])
            k = len(self._keys)
            buf[:k].add_(vec.to(torch.float64), alpha=int(batch_size))
            buf[k:].add_(int(batch_size))

    def compute(self, process_group=None) -> Dict[str, torch.Tensor]:
        """{key: fp32 device scalar}, the global weighted mean (one collective when distributed)."""
        if self._keys is None:
            raise RuntimeError("EvalAccumulator.compute before any add() and without keys")
        with eval_grad_mode():
            buf = self._ensure(self._device or torch.device("cpu")).clone()
            if _active(process_group):
                dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=process_group)
            k = len(self._keys)
            mean = (buf[:k] / buf[k]).to(torch.float32)
        return {key: mean[i] for i, key in enumerate(self._keys)}

    def reset(self) -> None:
        if self._buf is not None:
            with eval_grad_mode():
                self._buf.zero_()
