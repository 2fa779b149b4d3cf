"""Teacher-forced references for the bf16 training step (a helper module of the suite, not a conftest).

Two parts:

  * plain torch references of every layer the engine runs, on the CPU: fp32 convolutions of bf16-exact operands and fp64
    for every reduction.  Where a kernel rounds an operand or evaluates a decision in a particular way, the reference
    mirrors the kernel (cited per function), so that fed with the tensors a real step recorded, each layer can be held
    to the per-op tolerances: ReLU masks and pool winners come from the step's own tensors and the backward is linear.
    tests/test_stepwise_ref_cpu.py checks these against torch autograd of nn.Conv2d / nn.BatchNorm2d / F.max_pool2d /
    F.interpolate in fp64.
  * ``Recorder``: a context manager that wraps the engine's layer functions and the ops the training / sampling steps
    call, and keeps clones (taken on the current stream, at call time) of what each launch received and produced.

All activations are NHWC, as the engine keeps them."""
from __future__ import annotations

import contextlib
import os
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

BF = torch.bfloat16

# Conv3x3Family (conv3x3_mfma.hip) as s2s_conv3x3_family returns it
FAMILY_NAMES = ("kStageResident", "kStageStream", "kPersCarry", "kPers", "kTap", "kSplitF32")


def cpu_threads() -> int:
    """The GPU box reports more cores than its share of 16."""
    return min(16, os.cpu_count() or 8)


def bf(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (round to nearest even, as the kernels' conversions do) and return fp32."""
    return t.to(BF).float()


def to_nchw(x: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    return x.detach().cpu().to(dtype).permute(0, 3, 1, 2).contiguous()


def to_nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# convolutions (fp32 on bf16-exact operands; torch's CPU convolution accumulates in fp32)
# ---------------------------------------------------------------------------------------------------------------------
def cat_input(x0: torch.Tensor, x1: Optional[torch.Tensor]) -> torch.Tensor:
    """NCHW fp32 of cat(x0, x1) along channels; x0 / x1 NHWC."""
    x = to_nchw(x0)
    return x if x1 is None else torch.cat([x, to_nchw(x1)], 1)


def conv3x3(x_nchw: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    return F.conv2d(x_nchw.float(), w.float().cpu(), None if bias is None else bias.float().cpu(), padding=1)


def conv3x3_dgrad(dy_nchw: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    return F.conv_transpose2d(dy_nchw.float(), w.float().cpu(), None, padding=1)


def conv3x3_wgrad(x_nchw: torch.Tensor, dy_nchw: torch.Tensor) -> torch.Tensor:
    cout, cin = dy_nchw.shape[1], x_nchw.shape[1]
    return torch.nn.grad.conv2d_weight(x_nchw.float(), (cout, cin, 3, 3), dy_nchw.float(), padding=1)


def stem_image(x_nchw: torch.Tensor) -> torch.Tensor:
    """The fp32 image as the bf16 stem paths see it: the 8-channel NHWC pack (p2p_pack_kernel) and the stem weight
    gradient (stem_wgrad_kernel, split_store with one image) both convert it to bf16."""
    return bf(x_nchw.detach().cpu().float())


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm2d (train) statistics, running statistics, apply
# ---------------------------------------------------------------------------------------------------------------------
def bn_stats(raw: torch.Tensor, eps: float = 1e-5) -> Dict[str, torch.Tensor]:
    """fp64 per-channel statistics of the STORED conv output (NHWC): mean, biased var, invstd, element count."""
    r = raw.detach().cpu().double().reshape(-1, raw.shape[-1])
    n = r.shape[0]
    mean = r.sum(0) / n
    var = ((r - mean) ** 2).sum(0) / n
    return {"mean": mean, "var": var, "invstd": 1.0 / torch.sqrt(var + eps), "count": n}


def bn_affine(st: Dict[str, torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor):
    """(scale, shift) of the folded train-mode normalisation."""
    scale = gamma.detach().cpu().double() * st["invstd"]
    return scale, beta.detach().cpu().double() - st["mean"] * scale


def bn_running(rm: torch.Tensor, rv: torch.Tensor, st: Dict[str, torch.Tensor], momentum: float = 0.1,
               conv_bias: Optional[torch.Tensor] = None):
    """nn.BatchNorm2d's running-statistic update behind nn.Conv2d(bias=True): the statistics were taken without the
    bias (it cancels in the normalised output), the running mean is that of conv + bias, the variance is unbiased."""
    n = st["count"]
    mean = st["mean"] + (0.0 if conv_bias is None else conv_bias.detach().cpu().double())
    unbiased = st["var"] * (n / (n - 1.0))
    rm, rv = rm.detach().cpu().double(), rv.detach().cpu().double()
    return (1.0 - momentum) * rm + momentum * mean, (1.0 - momentum) * rv + momentum * unbiased


def fma_f32(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """fp32 fmaf(x, scale, shift) per channel (last dim): the product of two fp32 values is exact in fp64, so one
    fp64 add and the rounding to fp32 reproduce fmaf except where the fp64 sum itself rounds onto an fp32 tie."""
    return (x.detach().cpu().double() * scale.detach().cpu().float().double()
            + shift.detach().cpu().float().double()).float()


def bn_relu_apply(raw: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor):
    """bn_relu_apply_kernel: y = fmaxf(fmaf(raw, scale, shift), 0) in fp32, stored in bf16.  Returns (fp32 y, stored y)."""
    y = fma_f32(raw, scale, shift).clamp_min(0.0)
    return y, bf(y)


def pool_winner(y: torch.Tensor) -> torch.Tensor:
    """Index 0..3 of the winner of every 2x2 window of ``y`` (NHWC, the stored values): the FIRST maximum in the order
    (0,0), (0,1), (1,0), (1,1) (WindowGrad::eval in norm_act.hip: strict ``>`` while scanning)."""
    B, H, W, C = y.shape
    q = y.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4, C)
    best = torch.zeros((B, H // 2, W // 2, C), dtype=torch.long)
    bv = q[:, :, :, 0]
    for k in range(1, 4):
        better = q[:, :, :, k] > bv
        best = torch.where(better, torch.full_like(best, k), best)
        bv = torch.where(better, q[:, :, :, k], bv)
    return best


def maxpool2(y: torch.Tensor) -> torch.Tensor:
    B, H, W, C = y.shape
    return y.reshape(B, H // 2, 2, W // 2, 2, C).amax((2, 4))


def pool_scatter(gp: torch.Tensor, winner: torch.Tensor) -> torch.Tensor:
    """The pooled gradient ``gp`` [B, H/2, W/2, C] placed on each window's winner: [B, H, W, C]."""
    B, Hp, Wp, C = gp.shape
    out = torch.zeros((B, Hp, Wp, 4, C), dtype=gp.dtype)
    out.scatter_(3, winner.unsqueeze(3), gp.unsqueeze(3))
    return out.reshape(B, Hp, Wp, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * Hp, 2 * Wp, C)


def bn_relu_bwd(g1: Optional[torch.Tensor], gp: Optional[torch.Tensor], raw: torch.Tensor, stats: torch.Tensor,
                gamma: torch.Tensor):
    """Backward of BN(train) -> ReLU (-> 2x2 max-pool) as the kernels recompute it from the saved conv output ``raw``
    and the forward's ``stats`` rows (mean, invstd, scale, shift): the ReLU mask is fmaf(raw, scale, shift) > 0, the
    pool winner the first maximum of the stored (bf16) ReLU output, dz = g1 + scatter(gp) in fp32, xhat = (raw - mean)
    * invstd in fp32; sums in fp64.  Returns (draw fp64, dgamma, dbeta), dgamma = sum dz xhat, dbeta = sum dz."""
    stats = stats.detach().cpu().float()
    raw = raw.detach().cpu().float()
    z = fma_f32(raw, stats[2], stats[3])
    dz = torch.zeros_like(raw) if g1 is None else g1.detach().cpu().float().clone()
    if gp is not None:
        dz = dz + pool_scatter(gp.detach().cpu().float(), pool_winner(bf(z.clamp_min(0.0))))
    dz = torch.where(z > 0, dz, torch.zeros_like(dz)).double()
    xh = ((raw - stats[0]) * stats[1]).double()
    C = raw.shape[-1]
    n = raw.numel() // C
    dbeta = dz.reshape(-1, C).sum(0)
    dgamma = (dz * xh).reshape(-1, C).sum(0)
    draw = (gamma.detach().cpu().double() * stats[1].double()) * (dz - dbeta / n - xh * (dgamma / n))
    return draw, dgamma, dbeta


# ---------------------------------------------------------------------------------------------------------------------
# up-sampling, time path, head + loss, glue
# ---------------------------------------------------------------------------------------------------------------------
def _ac_matrix(n_in: int, n_out: int) -> torch.Tensor:
    """[n_out, n_in] bilinear weights of align_corners=True (src = dst * (n_in-1)/(n_out-1))."""
    m = torch.zeros((n_out, n_in), dtype=torch.float64)
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    for d in range(n_out):
        s = d * scale
        i0 = min(int(s), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        w1 = s - i0
        m[d, i0] += 1.0 - w1
        m[d, i1] += w1
    return m


def upsample2x(x: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 bilinear x2 (align_corners) of NHWC ``x`` (+ the per-(sample, channel) bias added to its input first)."""
    x = x.detach().cpu().double()
    if bias is not None:
        x = x + bias.detach().cpu().double()[:, None, None, :]
    _, H, W, _ = x.shape
    return torch.einsum("ph,qw,bhwc->bpqc", _ac_matrix(H, 2 * H), _ac_matrix(W, 2 * W), x)


def upsample2x_bwd(dy: torch.Tensor, hin: int, win: int) -> torch.Tensor:
    dy = dy.detach().cpu().double()
    _, Ho, Wo, _ = dy.shape
    return torch.einsum("ph,qw,bpqc->bhwc", _ac_matrix(hin, Ho), _ac_matrix(win, Wo), dy)


def pixel_sum(x: torch.Tensor) -> torch.Tensor:
    return x.detach().cpu().double().sum((1, 2))


def time_embedding(t: torch.Tensor, dim: int) -> torch.Tensor:
    """fp64 sinusoidal embedding [sin(t f_k) | cos(t f_k)], f_k = exp(-k log(1e4) / (dim/2 - 1))."""
    half = dim // 2
    f = torch.exp(torch.arange(half, dtype=torch.float64) * -(torch.log(torch.tensor(1e4, dtype=torch.float64)) / (half - 1)))
    a = t.detach().cpu().double()[:, None] * f[None]
    return torch.cat([a.sin(), a.cos()], 1)


def time_path(temb: torch.Tensor, dec, dtb: Optional[torch.Tensor] = None):
    """FlowMatchingDecoder's time MLP + projection in fp64: returns (tbias, {parameter name: gradient} given the gradient
    ``dtb`` [B, Cb] reaching the bias, else {})."""
    P = {n: p.detach().cpu().double().requires_grad_(dtb is not None) for n, p in dec.named_parameters()
         if n.startswith(("time_mlp.", "time_proj."))}
    x = temb.detach().cpu().double()
    with torch.enable_grad():
        h = F.linear(x, P["time_mlp.0.weight"], P["time_mlp.0.bias"])
        h = F.linear(F.silu(h), P["time_mlp.2.weight"], P["time_mlp.2.bias"])
        tb = F.linear(h, P["time_proj.weight"], P["time_proj.bias"])
        if dtb is None:
            return tb.detach(), {}
        tb.backward(dtb.detach().cpu().double())
    return tb.detach(), {n: p.grad for n, p in P.items()}


def head_loss(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], u_nchw: torch.Tensor):
    """1x1 head + mean squared error and their backward in fp64 (head_loss_lanes_kernel reads the fp32 weight as is).
    x NHWC; returns (loss, v NCHW, dx NHWC, dw [Cout, C, 1, 1], db)."""
    x = x.detach().cpu().double()
    cout = w.shape[0]
    wm = w.detach().cpu().double().reshape(cout, -1)
    v = x @ wm.t()
    if b is not None:
        v = v + b.detach().cpu().double()
    u = u_nchw.detach().cpu().double().permute(0, 2, 3, 1)
    d = v - u
    loss = (d * d).mean()
    dv = d * (2.0 / d.numel())
    dw = torch.einsum("bhwo,bhwc->oc", dv, x).reshape(w.shape)
    return loss, v.permute(0, 3, 1, 2), dv @ wm, dw, dv.sum((0, 1, 2))


def head_fwd(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor]) -> torch.Tensor:
    cout = w.shape[0]
    v = x.detach().cpu().double() @ w.detach().cpu().double().reshape(cout, -1).t()
    if b is not None:
        v = v + b.detach().cpu().double()
    return v.permute(0, 3, 1, 2)


def cfm_sample(x0: torch.Tensor, x1: torch.Tensor, t: torch.Tensor):
    """xt = t x1 + (1 - t) x0, ut = x1 - x0 (sigma = 0), fp64."""
    x0, x1, t = (a.detach().cpu().double() for a in (x0, x1, t))
    tt = t.reshape(-1, 1, 1, 1)
    return tt * x1 + (1.0 - tt) * x0, x1 - x0


def eval_affine(bn) -> tuple:
    """Eval-mode BatchNorm folded to (scale, shift) from the running statistics, fp64."""
    sc = bn.weight.detach().cpu().double() / torch.sqrt(bn.running_var.detach().cpu().double() + bn.eps)
    return sc, bn.bias.detach().cpu().double() - bn.running_mean.detach().cpu().double() * sc


# ---------------------------------------------------------------------------------------------------------------------
# error measures
# ---------------------------------------------------------------------------------------------------------------------
def rel_max(a: torch.Tensor, r: torch.Tensor) -> float:
    a, r = a.detach().cpu().double(), r.detach().cpu().double()
    return float((a - r).abs().max() / max(float(r.abs().max()), 1e-30))


def rel_l2(a: torch.Tensor, r: torch.Tensor) -> float:
    a, r = a.detach().cpu().double(), r.detach().cpu().double()
    return float((a - r).norm() / max(float(r.norm()), 1e-30))


def bf16_ulps(a: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """|a - r| in units of the bf16 spacing at |r| (8 significant bits)."""
    a, r = a.detach().cpu().double(), r.detach().cpu().double()
    mag = r.abs().clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    return (a - r).abs() / ulp


# ---------------------------------------------------------------------------------------------------------------------
# recorder
# ---------------------------------------------------------------------------------------------------------------------
def _clone(v):
    if isinstance(v, torch.Tensor):
        return v.detach().clone()
    if isinstance(v, (tuple, list)):
        return type(v)(_clone(x) for x in v)
    return v


def conv3x3_family(x0, x1, w_packed, bias, cout, want_stats=False, scale=None, out=None, **_) -> int:
    """The Conv3x3Family an ops.conv3x3 call with these arguments launches (the plan s2s_conv3x3_nhwc_s dispatches)."""
    from stain2stain_amd import ops
    L = ops._L()
    dt = ops._dt(x0)
    B, H, W, c0 = x0.shape
    _, ld0 = ops._nhwc(x0)
    ld1, c1 = 8, 0
    if x1 is not None:
        ld1, c1 = ops._nhwc(x1)[1], x1.shape[3]
    ldy = ops._nhwc(out)[1] if out is not None else cout
    has_bias = int(bias is not None)
    rows = L.s2s_conv3x3_stat_rows(dt, B, H, W, cout, c0, c1, ld0, ld1, has_bias) if want_stats else 0
    kwork = int(not want_stats and L.s2s_conv3x3_ksplit(dt, B, H, W, cout, c0 + c1) > 1)
    return L.s2s_conv3x3_family(dt, B, H, W, cout, c0, c1, ld0, ld1, ldy, has_bias, int(scale is not None),
                                int(want_stats), rows, kwork)


class Recorder:
    """Wraps ``engine._conv_bn_relu`` / ``engine._conv_bn_relu_bwd`` and the ops the CFM / multitask training steps and
    the sampler call; every wrapped call appends a dict of clones to ``calls[name]``:

      * ``fwd``  (engine._conv_bn_relu): name (``cb.prefix`` + conv index), cb, training, stem, x0, x1, raw, act, stats,
        pooled, rm0/rv0/nbt0 and rm1/rv1/nbt1 (running statistics around the call), ss (the folded eval-mode affine),
        families (one per ops.conv3x3 launch inside), raw_ptr (links the backward record)
      * ``bwd``  (engine._conv_bn_relu_bwd): name, cb, stem, accumulate, need_dx, g1, gp, draw, dx, families, raw_ptr
      * every other op: ``{"args": clones of the arguments before the call, "out": clones of the result,
        "after": clones of the tensor arguments after the call}`` (the latter for ops that write into an argument).

    Clones are taken on the current stream at call time; every attribute is restored on exit."""

    OPS = ("bn_relu_bwd", "head_loss_fused", "head_fwd", "upsample2x_fwd", "upsample2x_bwd", "cfm_sample",
           "time_embedding", "linear_fwd", "linear_bwd", "silu_fwd", "silu_bwd", "pixel_sum", "axpy_")
    IN_PLACE = ("upsample2x_fwd", "axpy_")

    def __init__(self):
        self.calls: Dict[str, List[dict]] = {k: [] for k in ("fwd", "bwd") + self.OPS}
        self._layer: Optional[dict] = None
        self._saved = []

    def _patch(self, mod, name, fn):
        self._saved.append((mod, name, getattr(mod, name)))
        setattr(mod, name, fn)

    def __enter__(self):
        from stain2stain_amd import engine, ops
        try:
            orig_fwd, orig_bwd, orig_conv = engine._conv_bn_relu, engine._conv_bn_relu_bwd, ops.conv3x3

            def conv3x3(*a, **k):
                if self._layer is not None:
                    self._layer["families"].append(conv3x3_family(*a, **k))
                return orig_conv(*a, **k)

            def fwd(cb, x0, x1, dtype, training, want_pool=False, stem=False):
                bn = cb.bn
                rec = {"name": f"{cb.prefix}.{cb.idx[0]}", "cb": cb, "training": training, "stem": stem,
                       "x0": _clone(x0), "x1": _clone(x1), "families": [],
                       "rm0": _clone(bn.running_mean), "rv0": _clone(bn.running_var),
                       "nbt0": _clone(bn.num_batches_tracked)}
                prev, self._layer = self._layer, rec
                try:
                    lc, act, pooled = orig_fwd(cb, x0, x1, dtype, training, want_pool, stem)
                finally:
                    self._layer = prev
                rec.update(act=_clone(act), pooled=_clone(pooled), rm1=_clone(bn.running_mean),
                           rv1=_clone(bn.running_var), nbt1=_clone(bn.num_batches_tracked))
                if lc is not None:
                    rec.update(raw=_clone(lc.raw), stats=_clone(lc.stats), raw_ptr=lc.raw.data_ptr())
                else:
                    rec["ss"] = _clone(cb._eval_ss)
                self.calls["fwd"].append(rec)
                return lc, act, pooled

            def bwd(cb, lc, g1, gp, grads, accumulate, need_dx, stem=False):
                rec = {"name": f"{cb.prefix}.{cb.idx[0]}", "cb": cb, "stem": stem, "accumulate": accumulate,
                       "need_dx": need_dx, "g1": _clone(g1), "gp": _clone(gp), "families": [],
                       "raw_ptr": lc.raw.data_ptr()}
                prev, self._layer = self._layer, rec
                try:
                    dx = orig_bwd(cb, lc, g1, gp, grads, accumulate, need_dx, stem)
                finally:
                    self._layer = prev
                rec["dx"] = _clone(dx)
                self.calls["bwd"].append(rec)
                return dx

            self._patch(ops, "conv3x3", conv3x3)
            self._patch(engine, "_conv_bn_relu", fwd)
            self._patch(engine, "_conv_bn_relu_bwd", bwd)
            for name in self.OPS:
                self._patch(ops, name, self._wrap(name, getattr(ops, name)))
        except BaseException:
            self._restore()
            raise
        return self

    def _wrap(self, name, orig):
        def fn(*a, **k):
            rec = {"args": _clone(a), "kwargs": _clone(k)}
            out = orig(*a, **k)
            rec["out"] = _clone(out)
            if name in self.IN_PLACE:
                rec["after"] = _clone(a)
            if name == "bn_relu_bwd" and self._layer is not None:
                self._layer["draw"] = rec["out"]
            self.calls[name].append(rec)
            return out
        return fn

    def _restore(self):
        while self._saved:
            mod, name, fn = self._saved.pop()
            setattr(mod, name, fn)

    def __exit__(self, *exc):
        self._restore()
        return False

    # ---- lookups -----------------------------------------------------------------------------------------------------
    def fwd(self, name: str, k: int = 0) -> dict:
        return [r for r in self.calls["fwd"] if r["name"] == name][k]

    def bwd(self, name: str, k: int = 0) -> dict:
        return [r for r in self.calls["bwd"] if r["name"] == name][k]

    def fwd_of(self, brec: dict) -> dict:
        """The forward record whose saved conv output the backward record ``brec`` used."""
        hits = [r for r in self.calls["fwd"] if r.get("raw_ptr") == brec["raw_ptr"] and r["name"] == brec["name"]]
        assert len(hits) == 1, (brec["name"], len(hits))
        return hits[0]

    def families(self) -> Dict[str, set]:
        """{family name: set of layer names that launched it} over the forward and backward records."""
        out: Dict[str, set] = {}
        for kind in ("fwd", "bwd"):
            for r in self.calls[kind]:
                for f in r["families"]:
                    out.setdefault(FAMILY_NAMES[f] if 0 <= f < len(FAMILY_NAMES) else str(f), set()).add(
                        f"{kind}:{r['name']}")
        return out


@contextlib.contextmanager
def cpu_thread_share():
    n = torch.get_num_threads()
    torch.set_num_threads(cpu_threads())
    try:
        yield
    finally:
        torch.set_num_threads(n)
