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
