"""One whole optimisation step of the stain-translation model without autograd:

    t, xt, ut  <- probability path sample        (conditional_flow_matching.py:66)
    v          <- U-Net(t, xt)                    (:69)
    loss       <- mean((v-ut)^2)                  (:72)
    grads      <- backward through the U-Net      (Lightning automatic optimisation)
    grads      <- bucketed RCCL all-reduce, overlapped with the rest of the backward (DDP, C1)
    params     <- Adam                            (configure_optimizers, :112-131)

This is the path ``bench.py`` times.  The LightningModule-compatible path (autograd Functions in
components.py + any torch optimiser) produces the same numbers; this class removes the autograd /
optimiser Python overhead, keeps all parameters, gradients and Adam moments in three flat fp32
buffers and overlaps communication with compute.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.distributed as dist

from . import engine, evaluation, ops
from .components import FlowUNet
from .ema import TrainerEMA
from .ddp import all_reduce_mean_scalar, broadcast_from_rank0
from .fused_step import CapturedStep, FlatParams


def _param_groups(net: FlowUNet) -> List[List[Tuple[str, str, torch.nn.Parameter]]]:
    """Parameters grouped in the order the backward pass finishes them, one group per conv + BatchNorm LAYER
    (engine.decoder_backward / encoder_backward fire ``on_group_done`` in exactly this order): the head, every Up
    block from the last (its second conv before its first), the time MLP, every encoder level from the deepest.

    Each entry is (owner, local_name, parameter) with owner in {"dec", "enc"}.
    """
    dec, enc = net.flow_decoder, net.encoder
    dnamed = dict(dec.named_parameters())
    enamed = dict(enc.named_parameters())
    groups: List[List[Tuple[str, str, torch.nn.Parameter]]] = []

    def layer(owner, named, prefix):        # the two layers of a DoubleConv: (conv 3, bn 4) finishes before (conv 0, bn 1)
        for idx in (("3.", "4."), ("0.", "1.")):
            groups.append([(owner, n, p) for n, p in named.items()
                           if any(n.startswith(prefix + i) for i in idx)])

    groups.append([("dec", n, p) for n, p in dnamed.items() if n.startswith("outc.")])
    for i in range(len(dec.ups) - 1, -1, -1):
        layer("dec", dnamed, f"ups.{i}.conv.double_conv.")
    groups.append([("dec", n, p) for n, p in dnamed.items() if n.startswith("time_")])
    for i in range(len(enc.downs) - 1, -1, -1):
        layer("enc", enamed, f"downs.{i}.maxpool_conv.1.double_conv.")
    layer("enc", enamed, "inc.double_conv.")
    groups = [g for g in groups if g] if getattr(dec, "time_mlp", None) is None else groups
    seen = sum(len(g) for g in groups)
    if seen != len(dnamed) + len(enamed) or any(not g for g in groups):
        raise RuntimeError("parameter grouping does not cover the network")
    return groups


class FusedAdamHandle(torch.optim.Optimizer):
    """A ``torch.optim.Optimizer`` face for the trainer's fused Adam, so that the reference's schedulers
    (``ReduceLROnPlateau`` in configs/model/*.yaml:12-16, driven by Lightning on ``val/loss``) and anything else that
    edits ``optimizer.param_groups[0]["lr"]`` work unchanged: the trainer reads its hyper-parameters from this
    param group at every step.  ``step()`` runs the trainer's optimiser step (join the all-reduce, fused Adam,
    repack)."""

    def __init__(self, trainer: "CFMTrainer", lr, betas, eps, weight_decay):
        self._trainer = trainer
        super().__init__([trainer.fp.p], dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self._trainer.optimizer_step()
        return loss

    def zero_grad(self, set_to_none: bool = False) -> None:      # every backward overwrites the flat gradient buffer
        pass

    # The handle's own parameter list is the one flat buffer, which carries no per-parameter state: a checkpoint
    # written from the inherited state_dict() would silently drop exp_avg / exp_avg_sq / step.  Lightning and user
    # code checkpoint optimisers through these two methods, so they speak torch.optim.Adam's layout over
    # net.parameters() (what the reference's checkpoint["optimizer_states"][0] holds).
    def state_dict(self):
        return self._trainer.optimizer_state_dict()

    def load_state_dict(self, state_dict) -> None:
        self._trainer.load_optimizer_state_dict(state_dict)


class CFMTrainer:
    def __init__(self, net: FlowUNet, lr: float = 1e-4, weight_decay: float = 1e-5,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, sigma: float = 0.0,
                 bucket_mb: float = 4.0, process_group=None, sync_loss: bool = True, max_bucket_mb: float = 16.0,
                 sharded_optimizer: bool = False, sync_batchnorm: bool = False, graph: bool = False,
                 ema_decay: Optional[float] = None, ema_buffers: bool = True):
        """``graph``: ``step()`` replays ONE captured hipGraph per optimisation step (sample -> forward -> loss -> backward
        -> [gradient exchange] -> Adam -> repack: ~210 kernel launches) instead of issuing them from Python
        (fused_step.CapturedStep: eager warm-up, capture, bit-equal replays).
        ``sharded_optimizer``: exchange gradients by reduce-scatter, run the fused Adam on this rank's 1/world of every
        bucket and all-gather the updated parameters (ddp.GradBucketer, mode "reduce_scatter") instead of all-reduce +
        a full Adam pass on every rank.  Same results, same wire volume, 1/world of the optimiser's HBM traffic.
        ``sync_batchnorm``: BatchNorm statistics over the global batch (Lightning's ``sync_batchnorm: True``,
        configs/trainer/ddp.yaml:9; the stain experiments leave it off): two 2C-float all-reduces per layer and step.
        ``ema_decay``: keep an exponential moving average of the weights (None: off), the numbers of
        torch.optim.swa_utils.AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(ema_decay), use_buffers=ema_buffers)
        updated after every step (stain2stain_amd.ema).  The parameters' average is updated inside the fused Adam pass,
        the BatchNorm buffers' by one more launch; both are part of a captured step.  ``ema_model()`` is the averaged
        network.  With it off nothing of the step changes."""
        dev = next(net.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("stain2stain_amd: CFMTrainer needs the network on a GPU (HIP-only implementation)")
        self.net = net
        self.sigma = sigma
        self.pg = process_group
        self.sync_loss = sync_loss
        groups = [[(f"{owner}.{name}", p) for owner, name, p in g] for g in _param_groups(net)]
        self.fp = FlatParams(groups, bucket_mb, process_group, max_bucket_mb, sharded_optimizer)
        self.grads_enc = {k[len("enc."):]: v for k, v in self.fp.grads.items() if k.startswith("enc.")}
        self.grads_dec = {k[len("dec."):]: v for k, v in self.fp.grads.items() if k.startswith("dec.")}
        # net.parameters() order -> flat-buffer name: the torch.optim.Adam layout of optimizer_state_dict
        names = {id(p): name for g in groups for name, p in g}
        self._names = [names[id(p)] for p in net.parameters()]
        self.optimizer = FusedAdamHandle(self, lr, betas, eps, weight_decay)
        self.n_params = sum(p.numel() for g in groups for _, p in g)
        self._group = 0
        self._sync_bn = engine.SyncBNExchange(process_group) if sync_batchnorm and self.bucketer.enabled else None
        broadcast_from_rank0(list(net.buffers()), process_group)
        self._dtype = net.encoder.compute_dtype
        self.packer = engine.Conv3x3Packer(list(net.encoder._blocks) + list(net.flow_decoder.up_blocks), self._dtype)
        # weight gradients overlap the bandwidth-bound backward passes on a second HIP stream (engine.run_on_side);
        # S2S_WGRAD_STREAM=0 keeps everything on one stream
        self._side = ops.side_stream_for(dev)
        self.overlap_wgrad = True       # bench.py clears it on the steps whose kernels it brackets with HIP events
        # the last BatchNorm + ReLU, the head, the loss and their backward straight from the last conv output
        # (engine.decoder_tail_loss): neither the last activation nor its gradient is stored, the results are the
        # chain's bit for bit.  False keeps the chain
        # bn_relu_apply -> head_loss_fused -> bn_relu_bwd, as does a forward_backward that is asked for the velocity
        # (want_v: the inspecting call, which leaves every layer's activation in its context)
        self.fuse_tail = True
        # the activations that only an up-sampling reads (the bottleneck, the second conv of every Up block but the
        # last) are not stored: the up-sampling applies BatchNorm + ReLU to its loads (engine.LazyAct), same bits.  False,
        # or the inspecting call (want_v), keeps them
        self.lazy_up = True
        self.graph = graph
        self._graph_step = CapturedStep()
        self._ema = None
        if ema_decay is not None:
            self.fp.enable_ema(ema_decay)
            self._ema = TrainerEMA(self.fp, [net], ema_buffers)
        # evaluate()'s workspaces: never the ones a captured training step has baked into its graph (released by close())
        self._eval_owner = object()
        self._generation = evaluation.GenerationEval()      # evaluate_generation()'s velocities and captured steps

    step_count = property(lambda self: self.fp.step_count)
    bucketer = property(lambda self: self.fp.bucketer)
    flat_p = property(lambda self: self.fp.p)           # all parameters / gradients, in _param_groups order
    flat_g = property(lambda self: self.fp.g)
    _captured = property(lambda self: self._graph_step.graph)      # of the current batch shape (None: not captured)

    # hyper-parameters live in the optimiser handle's param group (schedulers edit them there)
    @property
    def _hp(self):
        return self.optimizer.param_groups[0]

    lr = property(lambda self: self._hp["lr"], lambda self, v: self._hp.__setitem__("lr", v))
    wd = property(lambda self: self._hp["weight_decay"], lambda self, v: self._hp.__setitem__("weight_decay", v))
    betas = property(lambda self: self._hp["betas"], lambda self, v: self._hp.__setitem__("betas", tuple(v)))
    eps = property(lambda self: self._hp["eps"], lambda self, v: self._hp.__setitem__("eps", v))

    # ------------------------------------------------------------------------------------------
    def forward_backward(self, x0: torch.Tensor, x1: torch.Tensor, t: Optional[torch.Tensor] = None,
                         want_v: bool = True):
        """Gradients of the local batch into the flat buffer (+ async all-reduce).  Returns (loss, v); the
        velocity field is only materialised when ``want_v`` (tests) -- the training step does not need it."""
        net = self.net
        enc, dec = net.encoder, net.flow_decoder
        dt = enc.compute_dtype
        B = x0.shape[0]
        x0, x1 = x0.float().contiguous(), x1.float().contiguous()       # NCHW fp32, the reference's boundary layout
        if t is None:
            t = torch.rand(B, device=x0.device, dtype=torch.float32)
        t = t.float().contiguous()
        eps_noise = torch.randn_like(x0) if self.sigma != 0.0 else None
        xt, ut = ops.cfm_sample(x0, x1, t, self.sigma, eps_noise)
        with engine.sync_batchnorm(self._sync_bn):
            lazy = self.lazy_up and not want_v
            ectx = engine.encoder_forward(enc._blocks, xt, dt, True, lazy_up=lazy)
            temb = ops.time_embedding(t, net.time_embedding.dim)
            feats = ectx.feats
            dctx = engine.decoder_forward(dec, feats[-1], feats[:-1][::-1], temb, dt, True, with_head=False,
                                          fuse_tail=self.fuse_tail and not want_v, lazy_up=lazy)
        if dctx.lows[-1] is None:       # fused tail: the loss and the head's gradients straight from the last conv output
            g_head = None
            loss, v = engine.decoder_tail_loss(dec, dctx, ut, self.grads_dec, want_v=want_v)
        else:
            # head conv + loss + their backward in one sweep over the last activation
            loss, g_head, v = ops.head_loss_fused(dctx.lows[-1], dec.outc.weight.detach(),
                                                  dec.outc.bias.detach() if dec.outc.bias is not None else None, ut,
                                                  self.grads_dec["outc.weight"], self.grads_dec.get("outc.bias"),
                                                  want_v=want_v)
            dctx.v = v
        self.bucketer.start_step()
        self._group = 0
        # (the scope's exit joins the side stream: whatever reads the gradients next -- Adam, a test -- is on the compute
        # stream)
        with engine.side_scope(self._side if self.overlap_wgrad else None):
            dbott, dskips, _ = engine.decoder_backward(dec, dctx, None, self.grads_dec, g_head=g_head,
                                                       on_group_done=self._group_done)
            L = len(feats) - 1
            dfeats = [dskips[L - 1 - l] for l in range(L)] + [dbott]
            engine.encoder_backward(enc._blocks, ectx, dfeats, self.grads_enc, on_group_done=self._group_done)
        return loss, dctx.v

    def _group_done(self) -> None:
        """The next parameter group (layer, in _param_groups order) has its gradients enqueued: BatchNorm / bias / linear
        gradients on the compute stream, the conv weight gradient on the side stream.  A bucket that closes here is
        exchanged behind BOTH streams (GradBucketer.mark_ready_ordered): the head and the time-MLP groups have no
        side-stream fork after their compute-stream kernels, so ordering behind the side stream alone is not enough."""
        self.bucketer.mark_ready_ordered(self._group, self._side if self.overlap_wgrad else None)
        self._group += 1

    def optimizer_step(self) -> None:
        self._enqueue_optimizer(None)
        self._after_step()

    def _after_step(self) -> None:
        engine.mutation_epoch[0] += 1
        if self._ema is not None:
            self._ema.after_step()

    def _enqueue_optimizer(self, hyper_dev: Optional[torch.Tensor]) -> None:
        """Join the exchange, Adam, [parameter all-gather], repack.  ``hyper_dev``: the Adam scalars in device memory
        (captured step) instead of kernel arguments."""
        engine.join_side(self._side)        # the weight gradients
        self.fp.adam(self.lr, self.betas, self.eps, self.wd, hyper_dev)
        if self._ema is not None:
            self._ema.update_buffers()
        self._repack()

    def _repack(self) -> None:
        self.packer.repack()        # master weights changed behind torch's version counter

    # ------------------------------------------------------------------------------------------
    # optimiser state in torch.optim.Adam's own layout, so a run can move between this trainer and the
    # reference's Lightning loop (checkpoint["optimizer_states"][0], parameters in net.parameters() order)
    def optimizer_state_dict(self) -> Dict:
        """With ``sharded_optimizer`` a rank's Adam moments are current only on its own 1/world of every bucket: they are
        all-gathered first, so the dump is the full state on every rank (a COLLECTIVE in that mode: every rank calls it,
        as Lightning's checkpoint hook does)."""
        sd = self.fp.state_dict()
        state = {}
        if self.step_count > 0:
            for i, name in enumerate(self._names):
                state[i] = {"step": torch.tensor(float(self.step_count)),
                            "exp_avg": sd["exp_avg"][name], "exp_avg_sq": sd["exp_avg_sq"][name]}
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.wd,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False,
                 "fused": None, "params": list(range(len(self._names)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd: Dict) -> None:
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._names):
            raise ValueError("optimizer state does not match this network (one group over net.parameters() expected)")
        if groups[0].get("amsgrad", False) or groups[0].get("maximize", False):
            raise ValueError("amsgrad / maximize Adam states are not supported")
        g = groups[0]
        self.lr, self.betas, self.eps, self.wd = g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]
        steps = set()
        fp = self.fp
        fp.m.zero_()
        fp.v.zero_()
        for i, (p, name) in enumerate(zip(self.net.parameters(), self._names)):
            st = sd["state"].get(i, sd["state"].get(str(i)))
            if st is None:
                continue
            o, n = fp.slot[name]
            if tuple(st["exp_avg"].shape) != tuple(p.shape):
                raise ValueError(f"optimizer state {i}: shape {tuple(st['exp_avg'].shape)} != {tuple(p.shape)}")
            fp.m[o:o + n].copy_(st["exp_avg"].reshape(-1))
            fp.v[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError("per-parameter step counts differ; the flat Adam kernel keeps one")
        fp.step_count = steps.pop() if steps else 0

    def step(self, x0: torch.Tensor, x1: torch.Tensor, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One training step on this rank's shard of the global batch; returns the (rank-mean) loss."""
        with ops.workspace_owner(self):          # split-K / weight-gradient slabs belong to this trainer (ops._workspace)
            if self.graph and ops._PROFILE is None:
                if t is None:
                    t = torch.rand(x0.shape[0], device=x0.device, dtype=torch.float32)
                if self.sigma != 0.0:
                    raise NotImplementedError("graph=True with sigma != 0: the path noise is drawn inside forward_backward")
                loss = self._graph_step.run((tuple(x0.shape), x0.device, self.overlap_wgrad), (x0, x1, t),
                                            self._step_body, [self.fp], (self.lr, self.betas, self.eps, self.wd))
            else:
                loss = self._step_body(x0, x1, t, None)
            self._after_step()
            return loss

    def _step_body(self, x0, x1, t, hyper_dev) -> torch.Tensor:
        loss, _ = self.forward_backward(x0, x1, t, want_v=False)
        work = all_reduce_mean_scalar(loss, self.pg) if self.sync_loss else None
        self._enqueue_optimizer(hyper_dev)
        if work is not None:
            work.wait()
            loss = loss / dist.get_world_size(self.pg)
        return loss

    # ------------------------------------------------------------------------------------------
    # exponential moving average of the weights (ema_decay=)
    def _ema_on(self) -> TrainerEMA:
        if self._ema is None:
            raise RuntimeError("stain2stain_amd: this trainer keeps no EMA (construct it with ema_decay=...)")
        return self._ema

    def ema_model(self) -> FlowUNet:
        """The averaged network: a persistent eval-mode FlowUNet whose parameters are views of the flat EMA buffer and
        whose buffers hold the averaged BatchNorm statistics.  The same object throughout; it follows every later step
        (its packed operands, folded BatchNorm constants and any sampler graph are refreshed at first use after a step).
        With ``sharded_optimizer`` a COLLECTIVE (the EMA shards are all-gathered)."""
        return self._ema_on().modules()[0]

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """AveragedModel's layout: ``n_averaged`` + ``module.<FlowUNet keys>`` (loads into AveragedModel and back)."""
        return self._ema_on().state_dict(self.ema_model().state_dict())

    def load_ema_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        ema = self._ema_on()
        ema.load_state_dict(sd, ema.copies[0])

    def evaluate(self, x0: torch.Tensor, x1: torch.Tensor, t: Optional[torch.Tensor] = None,
                 accumulator: Optional[evaluation.EvalAccumulator] = None,
                 use_ema: bool = False) -> Dict[str, torch.Tensor]:
        """The validation loss of one batch, {"loss": device scalar} (conditional_flow_matching.py:88-97): path sample,
        eval-mode forward (BatchNorm from the running statistics), forward-only head + MSE.  Touches no training state
        (parameters, running statistics, gradients, Adam moments, step count, packed weights), never waits for the device,
        runs no collective (``accumulator.compute()`` does that once per epoch) and runs eagerly beside a captured step,
        on workspaces of its own.  ``accumulator``: the batch is added to it with weight ``x0.shape[0]``.
        ``use_ema``: score the averaged network (``ema_model()``; a collective with ``sharded_optimizer``)."""
        net = self.ema_model() if use_ema else self.net
        with ops.workspace_owner(self._eval_owner), evaluation.eval_grad_mode():
            x0, x1 = x0.float().contiguous(), x1.float().contiguous()
            if t is None:
                t = torch.rand(x0.shape[0], device=x0.device, dtype=torch.float32)
            t = t.float().contiguous()
            eps_noise = torch.randn_like(x0) if self.sigma != 0.0 else None
            xt, ut = ops.cfm_sample(x0, x1, t, self.sigma, eps_noise)
            loss = evaluation.flow_loss(net.encoder, net.flow_decoder, net.time_embedding.dim, xt, t, ut)
        out = {"loss": loss}
        if accumulator is not None:
            accumulator.add(out, x0.shape[0])
        return out

    def evaluate_generation(self, x0: torch.Tensor, x1: torch.Tensor, num_steps: int = 50, method: str = "euler",
                            graph: bool = False, use_ema: bool = False,
                            accumulator: Optional[evaluation.EvalAccumulator] = None,
                            quantize: bool = True, stain: Optional[dict] = None) -> Dict[str, torch.Tensor]:
        """Image quality of one generated batch: ``x0`` is carried to t = 1 by ``samplers.solve`` (``method`` one of
        ``samplers.SOLVER_METHODS``, ``num_steps`` for the fixed-step ones; ``graph``: a captured step, kept until the
        next optimiser step) on the eval-mode network and scored against the paired ``x1``.  Returns the per-sample
        {"psnr", "ssim", "mae", "mse"} of ``image_metrics.image_quality`` (fp32 [B] device tensors; ``quantize`` as
        there).  Like ``evaluate`` it touches no training state -- parameters, running statistics, module modes,
        gradients, Adam moments, step count, packed weights, a captured training step -- never waits for the device
        (eagerly; a capture does) and uses workspaces of its own.  ``accumulator``: the batch means are added with weight
        ``x0.shape[0]``.  ``use_ema``: sample from the averaged network.  ``method="dopri5"`` runs the per-sample
        controller at the default tolerances (a sample's score then does not depend on its batch mates; ``generate``'s
        default is the batch-wide one) and ignores ``num_steps``.  ``stain``: a dict of ``stain_quant.stain_agreement``'s
        keyword arguments adds "stain/burden_abs_err", "stain/dice" and "stain/iou" (how well the generated stain agrees
        with the real one on what is positive); ``None``: nothing changes."""
        net = self.ema_model() if use_ema else self.net
        with ops.workspace_owner(self._eval_owner), evaluation.eval_grad_mode():
            return evaluation.generation_values(self._generation, bool(use_ema), net.encoder, net.flow_decoder,
                                                net.time_embedding.dim, x0, x1, num_steps, method, graph, quantize,
                                                accumulator, stain)

    def close(self) -> None:
        """Drop the captured graph, its static buffers and the pinned Adam-scalar ring while torch and the HIP runtime are
        fully alive (a captured step sits in a reference cycle with its trainer; left to the cyclic collector it may be
        destroyed during another capture or at interpreter exit, in an order the runtime does not define)."""
        self._generation.close()
        self._graph_step.close()
        ops.release_workspaces(self)
        ops.release_workspaces(self._eval_owner)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
