"""Exponential moving average (EMA) of the weights, computed by the HIP kernels of optim.hip.

The numbers are those of ``torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay),
use_buffers=True)`` with ``update_parameters(model)`` called after every optimiser step:

  * the first update copies (``n_averaged`` 0 -> 1), every later one is ``ema = lerp(ema, x, 1 - decay)`` over every
    floating-point parameter AND buffer (BatchNorm running_mean / running_var).  Both are one lerp kernel: weight 1.0
    gives ``x`` exactly under torch's two-branch lerp;
  * integer buffers (``num_batches_tracked``) are COPIED from the live network.  This is the one deviation:
    AveragedModel lerps them through a float and truncates into int64, which only ever lags the live count;
  * the state-dict layout is AveragedModel's: ``n_averaged`` + ``module.<the network's own keys>``; states move both
    ways between this module and AveragedModel.

Two users:

  * ``TrainerEMA``  the fused trainers (``ema_decay=``).  The parameters' EMA lives in ``FlatParams.ema`` and is updated
                    inside the fused Adam pass; this object owns the averaged network -- a persistent copy whose
                    parameters are views of that buffer -- and one ``ema_multi`` launch per step for its buffers.
  * ``FusedEMA``    the drop-in path: AveragedModel's surface, each update ONE ``ema_multi`` launch over parameters and
                    buffers.
"""
from __future__ import annotations

import copy
from collections import OrderedDict
from typing import Dict, List, Sequence, Tuple

import torch

from . import engine, ops

PREFIX = "module."


# ------------------------------------------------------------------------------------------------
# state-dict layout (host only: no GPU needed)
# ------------------------------------------------------------------------------------------------
def averaged_state_dict(module_state: Dict[str, torch.Tensor], n_averaged: int) -> "OrderedDict[str, torch.Tensor]":
    """AveragedModel's layout: ``n_averaged`` (0-d int64) first, then the network's keys under ``module.``; every tensor
    is a detached copy that keeps its dtype (integer buffers stay integer)."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    out["n_averaged"] = torch.tensor(int(n_averaged), dtype=torch.long)
    for k, v in module_state.items():
        out[PREFIX + k] = v.detach().clone()
    return out


def split_averaged_state_dict(sd: Dict[str, torch.Tensor], expected_keys: Sequence[str]) -> Tuple[int, Dict]:
    """(n_averaged, the network's own state dict) of an AveragedModel-layout state; raises ValueError when the keys are
    not exactly ``n_averaged`` + ``module.<expected_keys>``."""
    want = {"n_averaged"} | {PREFIX + k for k in expected_keys}
    have = set(sd)
    if have != want:
        missing, unexpected = sorted(want - have), sorted(have - want)
        raise ValueError(f"EMA state does not match this network: missing {missing[:5]}, unexpected {unexpected[:5]}")
    n = sd["n_averaged"]
    n = int(n.item()) if isinstance(n, torch.Tensor) else int(n)
    if n < 0:
        raise ValueError(f"EMA state: n_averaged = {n} < 0")
    return n, {k[len(PREFIX):]: v for k, v in sd.items() if k != "n_averaged"}


def _ema_pairs(ema_module: torch.nn.Module, live_module: torch.nn.Module, buffers_only: bool
               ) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """(averaged, live) tensor pairs in AveragedModel's order: parameters, then buffers."""
    pairs = []
    if not buffers_only:
        ep, lp = list(ema_module.parameters()), list(live_module.parameters())
        if len(ep) != len(lp):
            raise ValueError("EMA: the live network does not have the averaged network's parameters")
        pairs += [(e.detach(), p.detach()) for e, p in zip(ep, lp)]
    eb, lb = list(ema_module.buffers()), list(live_module.buffers())
    if len(eb) != len(lb):
        raise ValueError("EMA: the live network does not have the averaged network's buffers")
    pairs += list(zip(eb, lb))
    for e, p in pairs:
        if e.shape != p.shape or e.dtype != p.dtype:
            raise ValueError(f"EMA: averaged {tuple(e.shape)} {e.dtype} vs live {tuple(p.shape)} {p.dtype}")
    return pairs


def _touch(tensors: Sequence[torch.Tensor]) -> None:
    """The EMA kernels write through raw pointers, behind torch's version counters.  The averaged network's packed MFMA
    operands are cached by (pointer, version) of their master weight (engine.ConvBN.packed; the forward refreshes stale
    ones in one batched launch, engine.repack_stale) and a sampler's captured graph by the parameter versions
    (samplers.GraphedVelocity): bumping the versions here is what makes both see the new average.  The folded
    BatchNorm constants are keyed on engine.mutation_epoch, which the caller bumps."""
    with torch.no_grad():
        torch.autograd.graph.increment_version(list(tensors))


# ------------------------------------------------------------------------------------------------
# the fused trainers' averaged network
# ------------------------------------------------------------------------------------------------
class TrainerEMA:
    """The averaged network of a fused trainer.  ``live``: the trainer's modules (their parameters already views of
    ``fp.p``); the copies' parameters become views of ``fp.ema`` at the same offsets, their buffers stay their own and
    are averaged by ``update_buffers`` (one ``ema_multi`` launch, weight from ``fp.ema_w``) when ``ema_buffers``;
    otherwise the same launch copies them from the live network (AveragedModel with ``use_buffers=False``)."""

    def __init__(self, fp, live: Sequence[torch.nn.Module], ema_buffers: bool = True):
        self.fp = fp
        self.live = list(live)
        self.copies: List[torch.nn.Module] = list(copy.deepcopy(tuple(self.live)))
        base, n_all = fp.p.data_ptr(), fp.p.numel()
        with torch.no_grad():
            for src, dst in zip(self.live, self.copies):
                for p, e in zip(src.parameters(), dst.parameters()):
                    o = (p.data_ptr() - base) // p.element_size()
                    if p.data_ptr() < base or o + p.numel() > n_all:
                        raise RuntimeError("TrainerEMA: a parameter is not a view of the flat parameter buffer")
                    e.data = fp.ema[o:o + p.numel()].view(p.shape)
                    e.requires_grad_(False)
                dst.eval()
        self.ema_buffers = ema_buffers
        pairs = [pr for src, dst in zip(self.live, self.copies) for pr in _ema_pairs(dst, src, buffers_only=True)]
        self.table = ops.EmaTable(pairs, [not ema_buffers] * len(pairs)) if pairs else None
        self._tensors = [t for m in self.copies for t in list(m.parameters()) + list(m.buffers())]

    def update_buffers(self) -> None:
        """Enqueue the buffer EMA of this step (after the step's Adam: its weight is already in ``fp.ema_w``)."""
        if self.table is not None:
            ops.ema_multi_(self.table, self.fp.ema_w.dev)

    def after_step(self) -> None:
        _touch(self._tensors)

    def modules(self) -> List[torch.nn.Module]:
        """The averaged networks, in eval mode, complete on every rank (sharded optimiser: a COLLECTIVE)."""
        self.fp.gather_ema()
        for m in self.copies:
            m.eval()
        return self.copies

    def state_dict(self, module_state: Dict[str, torch.Tensor]) -> "OrderedDict[str, torch.Tensor]":
        return averaged_state_dict(module_state, self.fp.n_averaged)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], target: torch.nn.Module) -> None:
        """``target``: the module whose keys the state carries (the averaged FlowUNet, or a ModuleDict of the three)."""
        n, inner = split_averaged_state_dict(sd, list(target.state_dict().keys()))
        with torch.no_grad():
            target.load_state_dict(inner, strict=True)     # parameters: copied into fp.ema through their views
        self.fp.n_averaged = n
        _touch(self._tensors)
        engine.mutation_epoch[0] += 1


# ------------------------------------------------------------------------------------------------
# the drop-in path
# ------------------------------------------------------------------------------------------------
class FusedEMA(torch.nn.Module):
    """``torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True)`` on the
    GPU: ``.module`` (a deep copy of ``model``), ``update_parameters(model)`` after every optimiser step, ``n_averaged``,
    ``state_dict`` / ``load_state_dict`` in AveragedModel's layout (the two interchange) and ``forward`` delegating to
    ``.module``.  Each update is ONE ``s2s_ema_multi`` launch over every parameter and buffer (integer buffers copied,
    see the module docstring); its descriptor table is cached by the pointer signature of the (averaged, live) pairs.
    ``use_buffers=False``: the parameters are averaged and the buffers copied from ``model``, as AveragedModel does
    (in the same launch).  GPU only: CPU modules raise."""

    def __init__(self, model: torch.nn.Module, decay: float = 0.999, use_buffers: bool = True):
        super().__init__()
        self.decay = ops.check_ema_decay(decay)
        tensors = list(model.parameters()) + list(model.buffers())
        if not tensors or any(not t.is_cuda for t in tensors):
            raise RuntimeError("stain2stain_amd.FusedEMA: the model must live on the GPU (HIP-only implementation)")
        self.module = copy.deepcopy(model)
        self.register_buffer("n_averaged", torch.tensor(0, dtype=torch.long, device=tensors[0].device))
        self.use_buffers = use_buffers
        self._n = 0                     # host copy of n_averaged: picks the lerp weight without a device read
        self._w = ops.EmaWeightSlot(tensors[0].device)
        self._table = None

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    @torch.no_grad()
    def update_parameters(self, model: torch.nn.Module) -> None:
        pairs = _ema_pairs(self.module, model, buffers_only=False)
        n_par = len(list(self.module.parameters()))
        copy_flags = [False] * n_par + [not self.use_buffers] * (len(pairs) - n_par)
        if any(not (e.is_cuda and p.is_cuda) for e, p in pairs):
            raise RuntimeError("stain2stain_amd.FusedEMA: the model must live on the GPU (HIP-only implementation)")
        # contiguous operands for the kernel: a non-contiguous live tensor is staged (rare; module tensors are contiguous)
        pairs = [(e, p if p.is_contiguous() else p.contiguous()) for e, p in pairs]
        if any(not e.is_contiguous() for e, _ in pairs):
            raise RuntimeError("stain2stain_amd.FusedEMA: averaged tensors must be contiguous")
        if self._table is None or self._table.signature != ops.EmaTable.signature_of(pairs):
            self._table = ops.EmaTable(pairs, copy_flags)
        self._w.push(ops.ema_weight(self._n, self.decay))
        ops.ema_multi_(self._table, self._w.dev)
        self.n_averaged += 1
        self._n += 1
        _touch([e for e, _ in pairs])
        engine.mutation_epoch[0] += 1

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self._n = int(self.n_averaged.item())
        _touch(list(self.module.parameters()) + list(self.module.buffers()))
        engine.mutation_epoch[0] += 1
        return out
