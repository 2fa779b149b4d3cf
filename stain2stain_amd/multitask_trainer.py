"""One optimisation step of the multitask model (BASELINE.json configs[4]) without autograd:

    t, xt, ut   <- probability path sample                       (conditional_flow_matching_multitask.py:224)
    flow loss   <- mean((flow_decoder(encoder(xt), t) - ut)^2)   (:228-231)
    seg loss    <- dw Dice + (1 - dw) BCE on seg_decoder(encoder(source))   (:236-246; softmax Dice + CE with num_classes)
    total       <- flow + seg_loss_weight * seg                   (:249)
    grads       <- backward through both heads and BOTH encoder passes (the encoder's gradients add up)
    params      <- one Adam over encoder + flow_decoder + seg_decoder (:391-417)

The shared encoder runs twice per step (on xt, then on the source image: BatchNorm's running statistics are updated in
that order, as in the reference), so this step is 668 GFLOP per 256x256 tile against the plain flow step's 334 -- "the
best showcase for conv throughput" (SURVEY 8f).  The module path (``MultiTaskFlowMatchingModule`` under autograd +
any torch optimiser) computes the same numbers; this class is its fused form: the engine's passes directly, the flow
head + MSE in one kernel, weight gradients on a side HIP stream, parameters / gradients / Adam moments in flat fp32
buffers in backward-completion order (gradient buckets are contiguous slices), one fused Adam, one batched repack.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.distributed as dist

from . import engine, evaluation, morphology, ops
from .components import FlowMatchingDecoder, SegmentationDecoder, SharedEncoder
from .ddp import all_reduce_mean_scalar
from .ema import TrainerEMA
from .fused_step import FlatParams


def _layer_groups(named: Dict[str, torch.nn.Parameter], prefix: str, owner: str) -> List[List[Tuple[str, torch.nn.Parameter]]]:
    """The two conv + BatchNorm layers of a DoubleConv in the order their backward finishes: (3, 4) before (0, 1)."""
    out = []
    for idx in (("3.", "4."), ("0.", "1.")):
        out.append([(f"{owner}.{n}", p) for n, p in named.items() if any(n.startswith(prefix + i) for i in idx)])
    return out


def _decoder_groups(dec, owner: str) -> List[List[Tuple[str, torch.nn.Parameter]]]:
    """engine.decoder_backward's on_group_done order: head, Up blocks from the last, then the time path (if any)."""
    named = dict(dec.named_parameters())
    groups = [[(f"{owner}.{n}", p) for n, p in named.items() if n.startswith("outc.")]]
    for i in range(len(dec.ups) - 1, -1, -1):
        groups += _layer_groups(named, f"ups.{i}.conv.double_conv.", owner)
    if getattr(dec, "time_mlp", None) is not None:
        groups.append([(f"{owner}.{n}", p) for n, p in named.items() if n.startswith("time_")])
    return groups


def _encoder_groups(enc, owner: str) -> List[List[Tuple[str, torch.nn.Parameter]]]:
    named = dict(enc.named_parameters())
    groups = []
    for i in range(len(enc.downs) - 1, -1, -1):
        groups += _layer_groups(named, f"downs.{i}.maxpool_conv.1.double_conv.", owner)
    return groups + _layer_groups(named, "inc.double_conv.", owner)


class MultiTaskTrainer:
    """Fused training step for ``SharedEncoder`` + ``FlowMatchingDecoder`` + ``SegmentationDecoder`` (their parameters
    become views of this trainer's flat buffers; ``state_dict`` / ``load_state_dict`` of the modules keep working).

    ``num_classes`` None: binary mask head, Dice + BCE; an integer: softmax Dice + CrossEntropy on class-index masks
    (conditional_flow_matching_multitask_multiclassloss.py:92-159), ``ignore_index`` as there.

    ``ema_decay``: an exponential moving average of the weights of all three networks, as CFMTrainer's (``ema_model()``
    returns the averaged (encoder, flow_decoder, seg_decoder); the state layout is AveragedModel's over
    ``torch.nn.ModuleDict(encoder=..., flow_decoder=..., seg_decoder=...)``)."""

    def __init__(self, encoder: SharedEncoder, flow_decoder: FlowMatchingDecoder, seg_decoder: SegmentationDecoder,
                 time_emb_dim: int = 256, lr: float = 1e-4, weight_decay: float = 1e-5,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, seg_loss_weight: float = 1.0,
                 dice_weight: float = 0.5, dice_smooth: float = 1.0, num_classes: Optional[int] = None,
                 ignore_index: int = -100, sigma: float = 0.0, bucket_mb: float = 4.0, process_group=None,
                 sync_loss: bool = True, max_bucket_mb: float = 16.0, sharded_optimizer: bool = False,
                 ema_decay: Optional[float] = None, ema_buffers: bool = True):
        dev = next(encoder.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("stain2stain_amd: MultiTaskTrainer needs the networks on a GPU (HIP-only implementation)")
        if not (encoder.compute_dtype == flow_decoder.compute_dtype == seg_decoder.compute_dtype):
            raise ValueError("encoder and decoders must share one precision")
        self.encoder, self.flow_decoder, self.seg_decoder = encoder, flow_decoder, seg_decoder
        self.time_emb_dim, self.sigma = time_emb_dim, sigma
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, tuple(betas), eps
        self.seg_loss_weight, self.dice_weight, self.dice_smooth = seg_loss_weight, dice_weight, dice_smooth
        self.num_classes, self.ignore_index = num_classes, ignore_index
        self.pg, self.sync_loss = process_group, sync_loss
        self._dtype = encoder.compute_dtype
        # backward-completion order: mask head and its Up blocks, flow head, its Up blocks and time MLP, then the encoder
        # (whose gradients are complete only when the SECOND of its two backward passes has run)
        groups = _decoder_groups(seg_decoder, "seg_decoder") + _decoder_groups(flow_decoder, "flow_decoder") \
            + _encoder_groups(encoder, "encoder")
        n_named = sum(1 for m in (encoder, flow_decoder, seg_decoder) for _ in m.parameters())
        if sum(len(g) for g in groups) != n_named or any(not g for g in groups):
            raise RuntimeError("parameter grouping does not cover the networks")
        self.fp = FlatParams(groups, bucket_mb, process_group, max_bucket_mb, sharded_optimizer)
        gr = self.fp.grads
        self.grads_enc = {k[len("encoder."):]: v for k, v in gr.items() if k.startswith("encoder.")}
        self.grads_flow = {k[len("flow_decoder."):]: v for k, v in gr.items() if k.startswith("flow_decoder.")}
        self.grads_seg = {k[len("seg_decoder."):]: v for k, v in gr.items() if k.startswith("seg_decoder.")}
        from .ddp import broadcast_from_rank0
        broadcast_from_rank0([b for m in (encoder, flow_decoder, seg_decoder) for b in m.buffers()], process_group)
        self.packer = engine.Conv3x3Packer(list(encoder._blocks) + list(flow_decoder.up_blocks)
                                           + list(seg_decoder.up_blocks), self._dtype)
        self._side = ops.side_stream_for(dev)
        self.overlap_wgrad = True
        self.fuse_tail = True           # the flow decoder's tail without its last activation, as CFMTrainer.fuse_tail
        # both decoders: no stored activation in front of an up-sampling but the first, as CFMTrainer.lazy_up.  The two
        # encoder passes keep their bottleneck: the step-wise suite reads every encoder layer's activation from this step
        self.lazy_up = True
        self._group = 0
        self._eval_owner = object()         # evaluate()'s workspaces, released by close()
        self._generation = evaluation.GenerationEval()      # evaluate_generation()'s velocities and captured steps
        self._ema = None
        if ema_decay is not None:
            self.fp.enable_ema(ema_decay)
            self._ema = TrainerEMA(self.fp, [encoder, flow_decoder, seg_decoder], ema_buffers)

    @property
    def step_count(self) -> int:
        return self.fp.step_count

    def _group_done(self) -> None:
        self.fp.bucketer.mark_ready_ordered(self._group, self._side if self.overlap_wgrad else None)
        self._group += 1

    # ------------------------------------------------------------------------------------------
    def forward_backward(self, source: torch.Tensor, target: torch.Tensor, mask: torch.Tensor,
                         t: Optional[torch.Tensor] = None, want_outputs: bool = False):
        """Gradients of the local batch into the flat buffer (+ async exchange).  Returns (losses, outputs): ``losses`` =
        {"total", "flow", "seg", "seg_dice", "seg_bce" | "seg_ce"} as device scalars (the reference's logging keys,
        conditional_flow_matching_multitask.py:251-257); ``outputs`` = {"v", "logits"} (NCHW fp32) when asked."""
        enc, fdec, sdec = self.encoder, self.flow_decoder, self.seg_decoder
        dt = self._dtype
        x0, x1 = source.float().contiguous(), target.float().contiguous()
        B = x0.shape[0]
        if t is None:
            t = torch.rand(B, device=x0.device, dtype=torch.float32)
        t = t.float().contiguous()
        eps_noise = torch.randn_like(x0) if self.sigma != 0.0 else None
        xt, ut = ops.cfm_sample(x0, x1, t, self.sigma, eps_noise)
        # forward: encoder(xt) -> flow head, then encoder(source) -> mask head (the reference's order, :228-236)
        lazy = self.lazy_up and not want_outputs
        ectx1 = engine.encoder_forward(enc._blocks, xt, dt, True)
        temb = ops.time_embedding(t, self.time_emb_dim)
        f1 = ectx1.feats
        dctx_f = engine.decoder_forward(fdec, f1[-1], f1[:-1][::-1], temb, dt, True, with_head=False,
                                        fuse_tail=self.fuse_tail and not want_outputs, lazy_up=lazy)
        ectx2 = engine.encoder_forward(enc._blocks, x0, dt, True)
        f2 = ectx2.feats
        dctx_s = engine.decoder_forward(sdec, f2[-1], f2[:-1][::-1], None, dt, True, lazy_up=lazy)
        logits = dctx_s.v
        if dctx_f.lows[-1] is None:     # fused tail (engine.decoder_tail_loss)
            g_head = None
            flow, v = engine.decoder_tail_loss(fdec, dctx_f, ut, self.grads_flow, want_v=want_outputs)
        else:
            flow, g_head, v = ops.head_loss_fused(dctx_f.lows[-1], fdec.outc.weight.detach(),
                                                  fdec.outc.bias.detach() if fdec.outc.bias is not None else None, ut,
                                                  self.grads_flow["outc.weight"], self.grads_flow.get("outc.bias"),
                                                  want_v=want_outputs)
        w = float(self.seg_loss_weight)
        if self.num_classes is not None:
            tgt = mask[:, 0] if (mask.dim() == 4 and mask.shape[1] == 1) else mask
            seg3, dz = ops.seg_loss_multiclass(logits, tgt.long(), self.ignore_index, self.dice_smooth, self.dice_weight,
                                               want_grad=True, grad_scale=w, validate=False)
        else:
            seg3, dz = ops.seg_loss(logits, mask.float().reshape(logits.shape), self.dice_smooth, self.dice_weight,
                                    want_grad=True, grad_scale=w)
        total = flow + w * seg3[0]                                       # (two device scalars: the logged total, :249)
        self.fp.bucketer.start_step()
        self._group = 0
        with engine.side_scope(self._side if self.overlap_wgrad else None):
            L = len(f1) - 1
            dbs, dss, _ = engine.decoder_backward(sdec, dctx_s, dz, self.grads_seg, on_group_done=self._group_done)
            dbf, dsf, _ = engine.decoder_backward(fdec, dctx_f, None, self.grads_flow, g_head=g_head,
                                                  on_group_done=self._group_done)
            # the encoder's two passes: the source pass writes its gradients, the xt pass adds to them and closes the groups
            engine.encoder_backward(enc._blocks, ectx2, [dss[L - 1 - l] for l in range(L)] + [dbs], self.grads_enc)
            engine.encoder_backward(enc._blocks, ectx1, [dsf[L - 1 - l] for l in range(L)] + [dbf], self.grads_enc,
                                    accumulate=True, on_group_done=self._group_done)
        second = "seg_ce" if self.num_classes is not None else "seg_bce"
        losses = {"total": total, "flow": flow, "seg": seg3[0], "seg_dice": seg3[1], second: seg3[2]}
        return losses, ({"v": v, "logits": logits} if want_outputs else None)

    def optimizer_step(self) -> None:
        engine.join_side(self._side)
        self.fp.adam(self.lr, self.betas, self.eps, self.wd)
        if self._ema is not None:
            self._ema.update_buffers()
        self.packer.repack()
        engine.mutation_epoch[0] += 1
        if self._ema is not None:
            self._ema.after_step()

    # ------------------------------------------------------------------------------------------
    # exponential moving average of the weights (ema_decay=)
    def _ema_on(self) -> TrainerEMA:
        if self._ema is None:
            raise RuntimeError("stain2stain_amd: this trainer keeps no EMA (construct it with ema_decay=...)")
        return self._ema

    def ema_model(self) -> Tuple[SharedEncoder, FlowMatchingDecoder, SegmentationDecoder]:
        """The averaged (encoder, flow_decoder, seg_decoder): persistent eval-mode copies whose parameters are views of
        the flat EMA buffer (see CFMTrainer.ema_model).  A collective with ``sharded_optimizer``."""
        return tuple(self._ema_on().modules())

    def _ema_container(self) -> torch.nn.ModuleDict:
        enc, fdec, sdec = self._ema_on().copies
        return torch.nn.ModuleDict(dict(encoder=enc, flow_decoder=fdec, seg_decoder=sdec))

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """AveragedModel's layout over ModuleDict(encoder, flow_decoder, seg_decoder): ``n_averaged`` + ``module.*``."""
        ema = self._ema_on()
        ema.modules()
        return ema.state_dict(self._ema_container().state_dict())

    def load_ema_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        self._ema_on().load_state_dict(sd, self._ema_container())

    def step(self, source: torch.Tensor, target: torch.Tensor, mask: torch.Tensor,
             t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One training step on this rank's shard of the global batch; returns the (rank-mean) total loss."""
        losses, _ = self.forward_backward(source, target, mask, t)
        total = losses["total"]
        work = all_reduce_mean_scalar(total, self.pg) if self.sync_loss else None
        self.optimizer_step()
        if work is not None:
            work.wait()
            total = total / dist.get_world_size(self.pg)
        return total

    def evaluate(self, source: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, t: Optional[torch.Tensor] = None,
                 accumulator: Optional[evaluation.EvalAccumulator] = None,
                 use_ema: bool = False, boundary: Optional[dict] = None) -> Dict[str, torch.Tensor]:
        """The validation / test values of one batch as device scalars: {"loss", "flow_loss", "seg_loss", "seg_dice",
        "seg_bce" | "seg_ce", "dice_coef", "iou"} (the reference's logging suffixes; dice_coef / iou as its test_step
        computes them, per-class means in the multiclass form).  Path sample, eval-mode forward of both heads
        (BatchNorm from the running statistics), forward-only head + MSE, one-pass segmentation loss + metrics.  Touches
        no training state, never waits for the device, runs no collective (``accumulator.compute()`` does, once) and
        uses workspaces of its own.  ``accumulator``: the batch is added to it with weight ``source.shape[0]``.
        ``use_ema``: score the averaged networks (``ema_model()``; a collective with ``sharded_optimizer``).
        ``boundary``: arguments of ``mask_boundary_agreement`` (``{}`` for its defaults); the binary head's
        ``logits > 0`` is scored against ``mask > 0`` and the batch means of hd, assd and surface_dice are added as
        "boundary/hd", "boundary/assd" and "boundary/surface_dice" (fp64).  Binary form only."""
        if boundary is not None:
            if self.num_classes is not None:
                raise ValueError("MultiTaskTrainer.evaluate: boundary metrics are defined for the binary mask head only")
            morphology._check_agreement(**{"tolerance": 2, "percentile": 95, **boundary}, what="MultiTaskTrainer.evaluate")
        with ops.workspace_owner(self._eval_owner), evaluation.eval_grad_mode():
            x0, x1 = source.float().contiguous(), target.float().contiguous()
            if t is None:
                t = torch.rand(x0.shape[0], device=x0.device, dtype=torch.float32)
            t = t.float().contiguous()
            eps_noise = torch.randn_like(x0) if self.sigma != 0.0 else None
            xt, ut = ops.cfm_sample(x0, x1, t, self.sigma, eps_noise)
            enc, fdec, sdec = self.ema_model() if use_ema else (self.encoder, self.flow_decoder, self.seg_decoder)
            flow = evaluation.flow_loss(enc, fdec, self.time_emb_dim, xt, t, ut)
            logits = evaluation.mask_logits(enc, sdec, x0)
            d = evaluation.segmentation_values(logits, mask, self.num_classes, self.ignore_index, self.dice_smooth,
                                               self.dice_weight)
            second = "seg_ce" if self.num_classes is not None else "seg_bce"
            out = {"loss": flow + float(self.seg_loss_weight) * d["seg"], "flow_loss": flow, "seg_loss": d["seg"],
                   "seg_dice": d["seg_dice"], second: d[second], "dice_coef": d["dice_coef"], "iou": d["iou"]}
            if boundary is not None:
                B, H, W = logits.shape[0], logits.shape[-2], logits.shape[-1]
                a = morphology.mask_boundary_agreement((logits > 0).reshape(B, H, W), (mask > 0).reshape(B, H, W),
                                                       **boundary)
                out.update({f"boundary/{k}": a[k].mean() for k in ("hd", "assd", "surface_dice")})
        if accumulator is not None:
            accumulator.add(out, x0.shape[0])
        return out

    def evaluate_generation(self, source: torch.Tensor, target: torch.Tensor, num_steps: int = 50,
                            method: str = "euler", graph: bool = False, use_ema: bool = False,
                            accumulator: Optional[evaluation.EvalAccumulator] = None,
                            quantize: bool = True, stain: Optional[dict] = None) -> Dict[str, torch.Tensor]:
        """Image quality of the flow head's generated batch against the paired ``target``: per-sample {"psnr", "ssim",
        "mae", "mse"} (fp32 [B] device tensors), as ``CFMTrainer.evaluate_generation``.  The reference's ``generate``
        also returns the mask; it plays no role here.  ``method="dopri5"``: the per-sample controller, as there.  Touches no training state and uses ``evaluate``'s workspaces.
        ``stain``: the stain-agreement keys, as there."""
        enc, fdec, _ = self.ema_model() if use_ema else (self.encoder, self.flow_decoder, self.seg_decoder)
        with ops.workspace_owner(self._eval_owner), evaluation.eval_grad_mode():
            return evaluation.generation_values(self._generation, bool(use_ema), enc, fdec, self.time_emb_dim, source,
                                                target, num_steps, method, graph, quantize, accumulator, stain)

    def close(self) -> None:
        """Release evaluate()'s workspaces and evaluate_generation()'s captured sampler steps."""
        self._generation.close()
        ops.release_workspaces(self._eval_owner)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
