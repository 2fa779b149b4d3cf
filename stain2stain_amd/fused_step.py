"""Host-side machinery shared by the fused trainers (trainer.CFMTrainer, multitask_trainer.MultiTaskTrainer,
pix2pix_engine.Pix2PixTrainer):

  * ``FlatParams``     parameters of a network as views of one flat fp32 buffer, with flat gradient / Adam-moment
                       buffers in backward-completion order (gradient buckets are contiguous slices), the bucketer and
                       the fused Adam over it; optionally a flat EMA of the parameters, updated inside that Adam pass
  * ``CapturedStep``   an optimisation step replayed as ONE captured hipGraph: eager warm-up, capture, static inputs,
                       the Adam scalars in device memory
"""
from __future__ import annotations

import warnings
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import ops
from .ddp import ALIGN, GradBucketer, broadcast_from_rank0


class FlatParams:
    """Parameters of one network as views of a flat fp32 buffer + flat gradient / Adam-moment buffers.

    ``groups``: [[(name, parameter), ...], ...] in the order the backward pass completes them."""

    def __init__(self, groups: List[List[Tuple[str, torch.nn.Parameter]]], bucket_mb: float, process_group,
                 max_bucket_mb: float = 16.0, sharded: bool = False):
        dev = groups[0][0][1].device
        sizes, offs, off = [], {}, 0
        self.group_range: List[Tuple[int, int]] = []
        for g in groups:
            start = off
            for name, p in g:
                offs[name] = off
                off += (p.numel() + 7) // 8 * 8            # 32-byte aligned views
            off = (off + ALIGN - 1) // ALIGN * ALIGN       # groups (layers) divide into aligned shards for <= 8 ranks
            sizes.append(off - start)
            self.group_range.append((start, off))
        self.p = torch.zeros(off, dtype=torch.float32, device=dev)
        self.g = torch.zeros(off, dtype=torch.float32, device=dev)
        self.m = torch.zeros(off, dtype=torch.float32, device=dev)
        self.v = torch.zeros(off, dtype=torch.float32, device=dev)
        self.grads: Dict[str, torch.Tensor] = {}
        self.slot: Dict[str, Tuple[int, int]] = {}
        with torch.no_grad():
            for g in groups:
                for name, p in g:
                    o, n = offs[name], p.numel()
                    self.p[o:o + n].copy_(p.detach().reshape(-1))
                    p.data = self.p[o:o + n].view(p.shape)
                    p.grad = self.g[o:o + n].view(p.shape)
                    self.grads[name] = p.grad
                    self.slot[name] = (o, n)
        self.bucketer = GradBucketer(self.g, sizes, bucket_mb, process_group, max_bucket_mb,
                                     "reduce_scatter" if sharded else "allreduce")
        self.step_count = 0
        broadcast_from_rank0([self.p], process_group)
        self.ema: Optional[torch.Tensor] = None        # enable_ema()
        self.ema_decay, self.n_averaged, self.ema_w = None, 0, None

    def enable_ema(self, decay: float) -> None:
        """Keep an exponential moving average of the parameters in ``ema`` (same slots as ``p``): every ``adam`` then
        runs the fused Adam + EMA kernel, ``ema = lerp(ema, p_new, w)`` with w = 1 on the first update (a copy) and
        ``1 - decay`` after -- torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(decay), updated after
        every optimiser step.  With a sharded optimiser each rank averages its own shards only (``gather_ema``)."""
        self.ema_decay = ops.check_ema_decay(decay)
        self.ema = self.p.clone()
        self.n_averaged = 0
        self.ema_w = ops.EmaWeightSlot(self.p.device)

    def ema_weight(self) -> float:
        return ops.ema_weight(self.n_averaged, self.ema_decay)

    def gather_ema(self) -> None:
        """Sharded optimiser: every rank's EMA shards to every rank (a COLLECTIVE in that mode, like ``state_dict``);
        otherwise nothing to do."""
        if self.ema is not None and self.n_averaged > 0:
            self.bucketer.all_gather(self.ema)

    def adam(self, lr: float, betas: Tuple[float, float], eps: float, weight_decay: float,
             hyper_dev: Optional[torch.Tensor] = None) -> None:
        """``hyper_dev``: the Adam scalars in device memory (a captured step; the caller advances ``step_count`` and
        refreshes them before each replay) instead of kernel arguments."""
        self.bucketer.wait_all()
        w = None
        if hyper_dev is None:
            self.step_count += 1
            if self.ema is not None:        # (the weight goes to device memory too: the trainers' BatchNorm-buffer EMA)
                w = self.ema_weight()
                self.ema_w.push(w)
        for lo, hi in self.bucketer.shards():              # everything, or this rank's slices in sharded mode
            self._adam_slice(lo, hi, lr, betas, eps, weight_decay, hyper_dev, w)
        if w is not None:
            self.n_averaged += 1
        self.bucketer.all_gather(self.p)

    def adam_group(self, group: int, lr: float, betas: Tuple[float, float], eps: float, weight_decay: float,
                   hyper_dev: Optional[torch.Tensor] = None) -> None:
        """Adam on the slice of parameter group ``group`` alone (the step counter is the caller's: ``begin_step``), for
        the update-in-backward of a trainer without a gradient exchange.  Adam is element-wise: the slices of all groups
        together are exactly ``adam``."""
        if self.ema is not None:
            raise NotImplementedError("stain2stain_amd: the per-group Adam (update in backward) has no EMA")
        self._adam_slice(*self.group_range[group], lr, betas, eps, weight_decay, hyper_dev)

    def _adam_slice(self, lo: int, hi: int, lr, betas, eps, weight_decay, hyper_dev, ema_w: Optional[float] = None) -> None:
        p, g, m, v = self.p[lo:hi], self.g[lo:hi], self.m[lo:hi], self.v[lo:hi]
        if self.ema is not None:
            if hyper_dev is None:
                ops.adam_ema_step_(p, g, m, v, self.ema[lo:hi], self.step_count, lr, betas[0], betas[1], eps, weight_decay,
                                   self.bucketer.grad_scale, ema_w)
            else:
                ops.adam_ema_step_dev_(p, g, m, v, self.ema[lo:hi], hyper_dev, self.ema_w.dev)
        elif hyper_dev is None:
            ops.adam_step_(p, g, m, v, self.step_count, lr, betas[0], betas[1], eps, weight_decay, self.bucketer.grad_scale)
        else:
            ops.adam_step_dev_(p, g, m, v, hyper_dev)

    def state_dict(self) -> Dict:
        """Adam state by parameter name.  Sharded optimiser: the moments are all-gathered first (a collective: every rank
        calls), so the dump is complete on every rank."""
        if self.bucketer.mode == "reduce_scatter" and self.bucketer.enabled and self.step_count > 0:
            self.bucketer.all_gather(self.m)
            self.bucketer.all_gather(self.v)
        out = {"step": self.step_count, "exp_avg": {}, "exp_avg_sq": {}}
        for name, (o, n) in self.slot.items():
            shape = self.grads[name].shape
            out["exp_avg"][name] = self.m[o:o + n].view(shape).clone()
            out["exp_avg_sq"][name] = self.v[o:o + n].view(shape).clone()
        return out

    def load_state_dict(self, sd: Dict) -> None:
        if set(sd["exp_avg"]) != set(self.slot) or set(sd["exp_avg_sq"]) != set(self.slot):
            raise ValueError("optimizer state does not match this network's parameters")
        for name, (o, n) in self.slot.items():
            for buf, key in ((self.m, "exp_avg"), (self.v, "exp_avg_sq")):
                t = sd[key][name]
                if tuple(t.shape) != tuple(self.grads[name].shape):
                    raise ValueError(f"optimizer state {name}: shape {tuple(t.shape)} != {tuple(self.grads[name].shape)}")
                buf[o:o + n].copy_(t.reshape(-1))
        self.step_count = int(sd["step"])


class CapturedStep:
    """A trainer's ``graph=True`` step: ONE captured hipGraph per batch shape (forward, loss, backward with the side-stream
    fork / joins, [gradient exchange], Adam, repack) replayed instead of ~200 Python-issued launches.  The first step of a
    shape runs eagerly (it is also the warm-up: module load, LDS attributes, workspaces), the second captures.  Same
    kernels in the same order: bit-equal to the eager step.  The host only copies the inputs into the static buffers and
    refreshes the eight Adam scalars (step count -> bias corrections, scheduler -> lr) in device memory before a replay.

    Holds the warm key, the graph with its static inputs and output and the pinned Adam-scalar ring; ``close()`` drops
    them."""

    _warned_multi_rank = False

    def __init__(self):
        self.close()

    def close(self) -> None:
        self.key = self.warm_key = self.graph = self.inputs = self.out = self.hyper = None

    def run(self, key, inputs: Sequence[torch.Tensor], body: Callable, flat_params: Sequence[FlatParams],
            hyper: Tuple[float, Tuple[float, float], float, float]) -> torch.Tensor:
        """One step: ``body(*inputs, hyper_dev)`` returns the step's output tensor and runs Adam on every ``FlatParams``
        of ``flat_params`` (scalars from kernel arguments when ``hyper_dev`` is None, else from device memory); ``key``
        names what a captured graph is valid for; ``hyper`` = (lr, betas, eps, weight_decay).  Every step counter moves
        only once its step has run (a failed warm-up or capture does not count as a step)."""
        bk = flat_params[0].bucketer
        if bk.enabled and dist.get_backend(bk.pg) != "nccl":
            raise RuntimeError("stain2stain_amd: graph=True captures the gradient exchange; only RCCL ('nccl') "
                               "collectives can be captured")
        if bk.enabled and not CapturedStep._warned_multi_rank:
            CapturedStep._warned_multi_rank = True
            warnings.warn("stain2stain_amd: graph=True with a gradient exchange captures the RCCL collectives; this has "
                          "only been exercised at world size 1 (S2S_FORCE_DDP) -- treat it as experimental", stacklevel=3)
        counts = [fp.step_count for fp in flat_params]
        averaged = [fp.n_averaged for fp in flat_params]
        if len(set(counts)) != 1:
            raise RuntimeError("graph=True: the optimisers must have taken the same number of steps")
        if self.hyper is None:
            self.hyper = ops.AdamHyperRing(inputs[0].device)
        if self.key != key:
            if self.warm_key != key:       # first step of this shape: eager
                self.warm_key, self.key, self.graph, self.inputs, self.out = key, None, None, None, None
                try:
                    return body(*inputs, None)
                except BaseException:
                    for fp, n, a in zip(flat_params, counts, averaged):
                        fp.step_count, fp.n_averaged = n, a
                    raise
            static = [torch.empty_like(x, dtype=torch.float32).contiguous() for x in inputs]
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with ops.capture_graph(graph):
                out = body(*static, self.hyper.dev)
            self.key, self.graph, self.inputs, self.out = key, graph, static, out
        for s, x in zip(self.inputs, inputs):
            s.copy_(x)
        lr, betas, eps, wd = hyper
        self.hyper.push(ops.adam_hyper(counts[0] + 1, lr, betas[0], betas[1], eps, wd, bk.grad_scale))
        for fp in flat_params:
            if fp.ema is not None:          # the EMA weight of this update, read by the captured kernels
                fp.ema_w.push(fp.ema_weight())
        self.graph.replay()
        for fp in flat_params:
            fp.step_count += 1
            if fp.ema is not None:
                fp.n_averaged += 1
        return self.out.clone()
