"""Case tables and the float64 host models of the kernels that end a training step or a validation pass, form by form (a
helper module of the suite, not a conftest; no HIP calls in here):

  s2s_head_loss_fused                      head_loss_lanes_kernel<T, PCB> / head_loss_fused_kernel<T>   (conv_edge.hip)
  s2s_tail_fwd_loss / s2s_tail_bwd_apply   tail_fwd_loss_kernel / tail_bwd_apply_kernel<T, PCB, MO>      (conv_edge.hip)
                                           bn_relu_bwd_reduce_tail_kernel<T> + bn_bwd_finalize_kernel    (norm_act.hip)
  s2s_head_mse_eval                        head_mse_eval_kernel<T, GL, MO, 4>                             (eval_metrics.hip)

Tables: ``name: (shape (B, H, W, C), options, expected family)``.  The family is what s2s_head_loss_family /
s2s_tail_family / s2s_head_mse_family answer; the pixel counts were chosen from the block queries and each row names the
walk it was written for (``walk`` below mirrors the kernels' grid-stride loops; tests/test_head_tail_forms_cpu.py holds it
to the library's block counts and asserts by enumeration that every form is in the tables).

Models (plain torch on the CPU, from the operands as the kernels read them; ``cd`` = float64 for the reference, float32
for the yardstick: what torch's fp32 arithmetic on the CPU costs for the same quantity):

  * ``head_model``: v = W x + b, loss = mean (v - u)^2, g = coef (v - u), dx = W^T g rounded to T on store, dW = g^T x,
    db = sum g.  The one-thread-per-pixel kernel stages the activation in LDS as bf16 for dW ("bf16 is enough for dW",
    head_loss_fused_kernel): with ``staged`` the model takes dW from the bf16-rounded activation, as that kernel does.
  * ``tail_model``: the chain of tests/test_tail_fused_gpu.py::_reference (z = fmaf(raw, scale, shift) in fp32: the ReLU
    DECISION is the kernel's; a = relu(z) rounded to T; the head; da = W^T g rounded to T; dz = da where z > 0; the
    BatchNorm sums, c1 = sum dz / n, c2 = sum dz xhat / n, d raw = gamma invstd (dz - c1 - xhat c2)).  ``da_seen``: the da
    a kernel stored (head_loss_fused's dx on the same operands).  Where the float64 da lies within the fp32 evaluation's
    error bound of a rounding boundary of T, the direction of that rounding is a decision as well, and the model takes
    the stored neighbour; everywhere else it rounds its own value.  ``means``: adds ``draw_forced_pre``, d raw evaluated
    with the kernel's fp32 c1 and c2 (from ``work``) as tests/bn_forms_ref.py does for BatchNorm's dx; c1 and c2
    themselves are held to the model.
  * ``eval_model``: the scalar mean (W a + b - u)^2.

Operand tiers.  ``exact``: small integers, hand-made statistics rows and a power-of-two coef, so that every fp32
operation of the kernels is exact whatever the order of the sums (``exact_preconditions`` checks that on the CPU).
``real``: normal / uniform operands as tests/test_tail_fused_gpu.py draws them, rounded to bf16 so that both storage types
read the same values.  Cases and references are cached and shared; treat them as read-only."""
from __future__ import annotations

import functools
from typing import Dict, Optional, Tuple

import torch

import stepwise_ref as SR

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
YARD_FLOOR = 1e-7
PIXEL = 100                      # s2s_head_loss_family's code of the one-thread-per-pixel kernel
ERR_SHAPE = -1
LOSS_BLOCK_CAP, MSE_BLOCK_CAP, MSE_UNROLL = 1024, 2048, 4

# cout, head bias, want_v, accumulate (onto random values; otherwise the kernels overwrite NaN), grad_scale class.  Four
# consecutive rows cover the four output counts; the exact tier turns the class into coef = 1 or 1/4 (a power of two).
OPTIONS = [(3, True, True, False, 1.0), (1, False, False, True, 0.25), (4, True, False, True, 1.0),
           (2, False, True, False, 0.25), (3, False, False, False, 0.25), (1, True, True, True, 1.0),
           (4, False, True, False, 0.25), (2, True, False, True, 1.0)]

# lanes per pixel -> [(B, H, W), what the walk of head_loss_lanes_kernel / tail_*_kernel looks like]; PPB = 256 / lanes
# pixels a workgroup round, nb = min(ceil(npix / 256), 1024) workgroups, rounds = ceil(npix / (nb PPB)).  Below the
# workgroup cap rounds <= lanes: one or two lanes per pixel reach a third round only past 262 144 pixels.
LANE_PIXELS = {
    1: [((1, 5, 7), "fewer"), ((1, 16, 16), "one"), ((3, 33, 18), "blocks-ragged"), ((5, 481, 109), "cap-2-last1"),
        ((3, 419, 418), "cap-3-ragged"), ((1, 1, 786433), "cap-4-last1")],
    2: [((1, 5, 7), "fewer"), ((2, 8, 8), "one"), ((1, 3, 43), "2-last1"), ((2, 10, 10), "2-ragged"),
        ((5, 481, 109), "cap-3-last1"), ((1, 1, 393217), "cap-4-last1")],
    4: [((1, 5, 7), "fewer"), ((1, 8, 8), "one"), ((2, 8, 12), "3-full"), ((1, 1, 193), "4-last1"), ((2, 5, 15), "3-ragged"),
        ((3, 33, 18), "blocks-4-ragged")],
    8: [((1, 3, 7), "fewer"), ((1, 4, 8), "one"), ((2, 6, 8), "3-full"), ((1, 1, 97), "4-last1"), ((3, 10, 20), "blocks-7-ragged"),
        ((37, 1, 1), "2-ragged")],
    16: [((1, 3, 5), "fewer"), ((1, 4, 4), "one"), ((3, 4, 4), "3-full"), ((1, 7, 7), "4-last1"), ((2, 5, 7), "5-ragged"),
         ((2, 16, 16), "blocks-16-full")],
    32: [((1, 1, 5), "fewer"), ((1, 2, 4), "one"), ((1, 3, 8), "3-full"), ((1, 5, 5), "4-last1"), ((2, 11, 13), "blocks-18-ragged"),
         ((37, 1, 1), "5-ragged")],
    64: [((1, 1, 3), "fewer"), ((1, 2, 2), "one"), ((1, 3, 4), "3-full"), ((1, 1, 13), "4-last1"), ((2, 3, 5), "8-ragged"),
         ((3, 10, 10), "blocks-38-full")],
}
# one-thread-per-pixel head (C / 8 = 3, 5, 9, 12; 96 channels sit just under the 60 KB of its LDS tile)
PIXEL_ROWS = [((1, 5, 7, 24), "fewer"), ((2, 19, 23, 40), "blocks-ragged"), ((1, 16, 16, 72), "one"), ((3, 10, 10, 96), "blocks-ragged"),
              ((2, 9, 7, 96), "fewer")]


def _name(shape, cout) -> str:
    return "x".join(map(str, shape)) + f"-o{cout}"


def _lane_rows(with_pixel: bool) -> Dict[str, tuple]:
    rows = {}
    for li, (lanes, pix) in enumerate(LANE_PIXELS.items()):
        for i, (bhw, walk) in enumerate(pix):
            opt = OPTIONS[(i + 3 * li) % len(OPTIONS)]
            rows[_name(bhw + (8 * lanes,), opt[0])] = (bhw + (8 * lanes,), opt + (walk,), lanes)
    if with_pixel:
        for i, (shape, walk) in enumerate(PIXEL_ROWS):
            opt = OPTIONS[(i + 2) % len(OPTIONS)]
            rows[_name(shape, opt[0])] = (shape, opt + (walk,), PIXEL)
    return rows


HEAD: Dict[str, tuple] = _lane_rows(True)                                   # family: lanes per pixel or PIXEL
TAIL: Dict[str, tuple] = {k: (s, o, (f, 3 if o[0] <= 3 else 4)) for k, (s, o, f) in _lane_rows(False).items()}   # (PCB, MO)
TAIL_TWO_GROUPS = 512            # bn_relu_bwd_reduce_tail_kernel takes 32 pieces a channel group: grid.x = 2 at C = 512

# eval loss: (B, H, W, C), (cout, bias), (GL, MO); PER = 256 / GL * 4 pixels an unrolled workgroup round
EVAL: Dict[str, tuple] = {}
for _shape, _cout, _bias, _fam in [
        ((1, 31, 33, 8), 3, True, (1, 3)), ((1, 32, 32, 8), 1, False, (1, 4)), ((5, 5, 41, 8), 5, True, (1, 8)),
        ((1, 7, 73, 16), 3, False, (2, 3)), ((2, 16, 16, 16), 2, True, (2, 4)), ((1, 19, 27, 24), 8, False, (2, 8)),
        ((1, 15, 17, 32), 3, True, (4, 3)), ((1, 16, 16, 40), 4, False, (4, 4)), ((1, 1, 257, 56), 6, True, (4, 8)),
        ((1, 1, 127, 64), 3, False, (8, 3)), ((2, 8, 8, 72), 1, True, (8, 4)), ((3, 43, 1, 128), 7, False, (8, 8)),
        ((37, 1, 1, 64), 4, True, (8, 4)), ((2, 9, 11, 1920), 2, False, (8, 4)), ((3, 33, 18, 72), 5, True, (8, 8)),
        ((5, 481, 109, 64), 3, True, (8, 3))]:
    EVAL[_name(_shape, _cout)] = (_shape, (_cout, _bias), _fam)
EVAL_CAPPED = "5x481x109x64-o3"
EVAL_MAX_C = 1920

# (entry, (B, H, W, C, cout)): launches that are refused with S2S_ERR_SHAPE
REFUSED = [("head", (1, 4, 4, 64, 5)), ("head", (1, 4, 4, 104, 3)), ("head", (1, 4, 4, 12, 3)),
           ("tail", (1, 4, 4, 64, 5)), ("tail", (1, 4, 4, 24, 3)), ("tail", (1, 4, 4, 12, 3)), ("tail", (1, 4, 4, 1024, 3)),
           ("eval", (1, 4, 4, 64, 9)), ("eval", (1, 4, 4, 12, 3)), ("eval", (1, 4, 4, 1928, 3))]


# ---------------------------------------------------------------------------------------------------------------------
# walk mirrors (labels only: the block counts come from the library)
# ---------------------------------------------------------------------------------------------------------------------
def walk(npix: int, ppb: int, nb: int) -> dict:
    """A grid-stride loop of ``nb`` workgroups over ``ppb`` pixels each: rounds, pixels of the last round."""
    stride = nb * ppb
    rounds = -(-npix // stride)
    last = npix - (rounds - 1) * stride
    return {"nb": nb, "rounds": rounds, "last": last, "ragged": last % ppb != 0, "full": last == stride}


def walk_label(npix: int, ppb: int, nb: int, cap: int) -> str:
    w = walk(npix, ppb, nb)
    if w["rounds"] == 1 and nb == 1:
        return "fewer" if npix < ppb else "one"
    pre = "cap-" if nb == cap else "blocks-" if nb > 1 else ""
    if w["rounds"] == 1:
        return pre + ("ragged" if w["ragged"] else "full")
    return pre + f"{w['rounds']}-" + ("last1" if w["last"] == 1 else "ragged" if w["ragged"] else "full")


# ---------------------------------------------------------------------------------------------------------------------
# error measures
# ---------------------------------------------------------------------------------------------------------------------
def round_to(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Values as a kernel stores them in T (round to nearest even), in the dtype they came in; float64 = no rounding."""
    if dtype == F64:
        return t
    return t.float().to(dtype).to(t.dtype)


def ulp(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    bits = 7 if dtype == BF else 23
    return torch.exp2(torch.floor(torch.log2(ref.abs().double().clamp_min(2.0 ** -126))) - bits)


def deviation(a: torch.Tensor, ref: torch.Tensor) -> Tuple[float, float]:
    return SR.rel_max(a, ref), SR.rel_l2(a, ref)


def ratios(err, yard) -> Tuple[float, float]:
    return err[0] / max(yard[0], YARD_FLOOR), err[1] / max(yard[1], YARD_FLOOR)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit equality of fp32 values (NaN equal to the same NaN, -0 different from +0)."""
    a, b = a.detach().cpu().float().contiguous(), b.detach().cpu().float().contiguous()
    return a.shape == b.shape and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
def coef_of(grad_scale: float, count: int) -> float:
    """(float)(2.0 * (double)grad_scale / count), the entry points' expression (grad_scale arrives as a C float)."""
    gs = float(torch.tensor(grad_scale, dtype=F32))
    return float(torch.tensor(2.0 * gs / count, dtype=F64).float())


def _flat_u(u: torch.Tensor, cd) -> torch.Tensor:
    return u.to(cd).permute(0, 2, 3, 1).reshape(-1, u.shape[1])


def _nchw(t: torch.Tensor, B, H, W) -> torch.Tensor:
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def head_model(x, w, b, u, coef: float, dtype, cd=F64, staged: bool = False) -> dict:
    B, H, W, C = x.shape
    cout = w.shape[0]
    xx, wm = x.to(cd).reshape(-1, C), w.to(cd).reshape(cout, C)
    v = xx @ wm.t()
    if b is not None:
        v = v + b.to(cd)
    d = v - _flat_u(u, cd)
    g = d * coef
    dx = g @ wm
    xw = SR.bf(x.float()).to(cd).reshape(-1, C) if staged else xx
    out = dict(v=_nchw(v, B, H, W), loss=(d * d).mean(), g=_nchw(g, B, H, W), dx_pre=dx.reshape(B, H, W, C),
               dx=round_to(dx, dtype).reshape(B, H, W, C), dw=g.t() @ xw)
    if b is not None:
        out["db"] = g.sum(0)
    return out


def tail_model(raw, stats, gamma, w, b, u, coef: float, dtype, cd=F64, da_seen=None, means=None) -> dict:
    """``stats``: rows mean, invstd, scale, shift (fp32 as the kernels read them; float64 with dtype float64)."""
    B, H, W, C = raw.shape
    cout = w.shape[0]
    n = B * H * W
    mean, invstd, scale, shift = (stats[i].to(cd) for i in range(4))
    if dtype == F64:
        z = raw.to(cd) * scale + shift
    else:
        z = SR.fma_f32(raw.float(), stats[2], stats[3])                # the decision, always in fp32
    act = round_to(z.clamp_min(0.0).to(cd), dtype)
    h = head_model(act, w, b, u, coef, dtype, cd)
    da, da_pre = h["dx"], h["dx_pre"]
    forced = 0
    if da_seen is not None and dtype == BF:
        # error bound of the kernels' fp32 chain of cout fmaf: cout roundings of at most 2^-24 sum |g_o w_o| each
        g = _flat_u(h["g"], F64).abs()
        band = (cout * 2.0 ** -24) * (g @ w.double().reshape(cout, C).abs()).reshape(B, H, W, C)
        tie = (da_pre.double() - da.double()).abs() >= 0.5 * ulp(da, dtype) - band
        seen = da_seen.to(cd)
        take = tie & ((seen - da_pre).abs().double() <= 0.5 * ulp(da, dtype) + band) & (seen != da)
        forced = int(take.sum())
        da = torch.where(take, seen, da)
    dz = torch.where(z.to(cd) > 0, da, torch.zeros_like(da))
    xh = (raw.to(cd) - mean) * invstd
    dbeta = dz.reshape(-1, C).sum(0)
    dgamma = (dz * xh).reshape(-1, C).sum(0)
    c1, c2 = dbeta / n, dgamma / n
    gak = gamma.to(cd) * invstd
    draw = gak * (dz - c1 - xh * c2)
    out = dict(h)
    del out["dx"], out["dx_pre"]
    out.update(act=act, da=da, dgamma=dgamma, dbeta=dbeta, c1=c1, c2=c2, draw_pre=draw, draw=round_to(draw, dtype),
               forced=forced, dbias=torch.zeros(C, dtype=cd))
    if means is not None:
        out["draw_forced_pre"] = gak * (dz - means[0].to(cd) - xh * means[1].to(cd))
    return out


def eval_model(x, w, b, u, cd=F64) -> torch.Tensor:
    B, H, W, C = x.shape
    v = x.to(cd).reshape(-1, C) @ w.to(cd).reshape(w.shape[0], C).t()
    if b is not None:
        v = v + b.to(cd)
    d = v - _flat_u(u, cd)
    return (d * d).mean()


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def _ints(gen, shape, lo, hi) -> torch.Tensor:
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _choice(gen, values, n) -> torch.Tensor:
    return torch.tensor(values, dtype=F32)[torch.randint(0, len(values), (n,), generator=gen)]


def _nonzero_residual(gen, shape, big: bool) -> torch.Tensor:
    """Integer v - u in {-2, -1, 1, 2} ({-1, 1} at the large pixel counts): never 0, so every d^2 is an integer >= 1."""
    r = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    return r if big else r * torch.randint(1, 3, shape, generator=gen).float()


def _seed(name: str, tier: str, salt: int) -> int:
    return (sum((i + 1) * ord(ch) for i, ch in enumerate(name + tier)) * 7919 + salt) % (2 ** 31)


@functools.lru_cache(maxsize=4)
def head_case(name: str, tier: str) -> dict:
    """Operands of a HEAD row as fp32 CPU tensors (bf16-exact where a kernel reads T).  ``grad_scale`` is what the entry
    point is given; in the exact tier it makes coef 1 or 1/4."""
    (B, H, W, C), (cout, bias, _v, acc, gs, _walk), _fam = HEAD[name]
    gen = torch.Generator().manual_seed(_seed(name, tier, 1))
    count = B * H * W * cout
    if tier == "exact":
        big = B * H * W > 2 ** 14
        x = _ints(gen, (B, H, W, C), -2, 3)
        w = _ints(gen, (cout, C), -1, 1) if big else _ints(gen, (cout, C), -2, 2)
        b = _ints(gen, (cout,), -3, 3) if bias else None
        v = head_model(x, w, b, torch.zeros(B, cout, H, W), 1.0, F32)["v"]
        u = (v - _nonzero_residual(gen, (B, cout, H, W), big)).float()
        grad_scale = gs * count / 2.0
        base = lambda *s: _ints(gen, s, -8, 8)                         # noqa: E731
    else:
        x = SR.bf(torch.randn(B, H, W, C, generator=gen) * (0.5 + torch.rand(C, generator=gen)) + torch.randn(C, generator=gen))
        w = (torch.rand(cout, C, generator=gen) * 2 - 1) * 0.3
        b = (torch.rand(cout, generator=gen) * 2 - 1) * 0.1 if bias else None
        u = torch.rand(B, cout, H, W, generator=gen) * 2 - 1
        grad_scale = gs
        base = lambda *s: torch.rand(*s, generator=gen) - 0.5          # noqa: E731
    out = dict(x=x, w=w, b=b, u=u, grad_scale=float(grad_scale), coef=coef_of(grad_scale, count), acc=acc,
               base=dict(dw=base(cout, C), db=base(cout)) if acc else None)
    return out


@functools.lru_cache(maxsize=4)
def tail_case(name: str, tier: str) -> dict:
    """Operands of a TAIL row.  Exact tier: hand-made statistics rows (scale +-1 / +-2, integer shift and mean,
    power-of-two invstd and gamma; every eighth channel entirely off, every eighth entirely on); real tier: the rows
    bn_finalize's formulas give for the tensor in float64, stored as fp32, with per-channel offsets that leave channels
    3 (mod 8) entirely off and 5 (mod 8) entirely on."""
    (B, H, W, C), (cout, bias, _v, acc, gs, _walk), _fam = TAIL[name]
    gen = torch.Generator().manual_seed(_seed(name, tier, 2))
    n = B * H * W
    count = n * cout
    ch = torch.arange(C)
    if tier == "exact":
        big = n > 2 ** 14
        raw = _ints(gen, (B, H, W, C), -2, 2) if big else _ints(gen, (B, H, W, C), -4, 4)
        scale = _choice(gen, [1.0, -1.0] if big else [1.0, -1.0, 2.0, -2.0], C)
        shift = _ints(gen, (C,), -1, 1) if big else _ints(gen, (C,), -3, 3)
        shift = torch.where(ch % 8 == 3, torch.full_like(shift, -20.0), shift)
        shift = torch.where(ch % 8 == 5, torch.full_like(shift, 4.0 if big else 20.0), shift)
        mean = _ints(gen, (C,), -1, 1) if big else _ints(gen, (C,), -2, 2)
        invstd = torch.ones(C) if big else _choice(gen, [0.5, 1.0, 2.0], C)
        gamma = _choice(gen, [0.5, 1.0, 2.0, -1.0], C)
        stats = torch.stack([mean, invstd, scale, shift])
        w = _ints(gen, (cout, C), -1, 1) if big else _ints(gen, (cout, C), -2, 2)
        b = _ints(gen, (cout,), -3, 3) if bias else None
        v = tail_model(raw, stats, gamma, w, b, torch.zeros(B, cout, H, W), 1.0, F32)["v"]
        u = (v - _nonzero_residual(gen, (B, cout, H, W), big)).float()
        grad_scale = gs * count / 2.0
        base = lambda *s: _ints(gen, s, -8, 8)                         # noqa: E731
    else:
        off = torch.randn(C, generator=gen)
        off = torch.where(ch % 8 == 3, torch.full_like(off, -30.0), off)
        off = torch.where(ch % 8 == 5, torch.full_like(off, 30.0), off)
        raw = SR.bf(torch.randn(B, H, W, C, generator=gen) * (0.5 + torch.rand(C, generator=gen)) + off)
        gamma = torch.rand(C, generator=gen) + 0.5
        beta = torch.rand(C, generator=gen) - 0.5
        beta = torch.where(ch % 8 == 3, beta - 8.0, torch.where(ch % 8 == 5, beta + 8.0, beta))
        r64 = raw.double().reshape(-1, C)
        mean = r64.mean(0)
        var = ((r64 - mean) ** 2).mean(0)
        invstd = (var + 1e-5).rsqrt()
        scale = gamma.double() * invstd
        stats = torch.stack([mean, invstd, scale, beta.double() - mean * scale]).float()
        w = (torch.rand(cout, C, generator=gen) * 2 - 1) * 0.3
        b = (torch.rand(cout, generator=gen) * 2 - 1) * 0.1 if bias else None
        u = torch.rand(B, cout, H, W, generator=gen) * 2 - 1
        grad_scale = gs
        base = lambda *s: torch.rand(*s, generator=gen) - 0.5          # noqa: E731
    return dict(raw=raw, stats=stats, gamma=gamma, w=w, b=b, u=u, grad_scale=float(grad_scale),
                coef=coef_of(grad_scale, count), acc=acc,
                base=dict(dw=base(cout, C), db=base(cout), dgamma=base(C), dbeta=base(C), dbias=base(C)) if acc else None)


@functools.lru_cache(maxsize=4)
def eval_case(name: str, tier: str) -> dict:
    (B, H, W, C), (cout, bias), _fam = EVAL[name]
    gen = torch.Generator().manual_seed(_seed(name, tier, 3))
    if tier == "exact":
        # few non-zero weights a row, so that v stays a small integer at 1920 channels too
        x = _ints(gen, (B, H, W, C), -2, 3)
        w = _ints(gen, (cout, C), -1, 1)
        b = _ints(gen, (cout,), -3, 3) if bias else None
        v = head_model(x, w, b, torch.zeros(B, cout, H, W), 1.0, F32)["v"]
        u = (v - _nonzero_residual(gen, (B, cout, H, W), False)).float()
    else:
        x = SR.bf(torch.randn(B, H, W, C, generator=gen))
        w = (torch.rand(cout, C, generator=gen) * 2 - 1) * (2.4 / C ** 0.5)
        b = (torch.rand(cout, generator=gen) * 2 - 1) * 0.1 if bias else None
        u = torch.rand(B, cout, H, W, generator=gen) * 2 - 1
    return dict(x=x, w=w, b=b, u=u)


def with_base(ref: dict, base: Optional[dict]) -> dict:
    """The gradients after an accumulating launch: base + the model's value, in the model's dtype."""
    if base is None:
        return ref
    out = dict(ref)
    for k, t in base.items():
        if k in out:
            out[k] = out[k] + t.to(out[k].dtype).reshape(out[k].shape)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the exact tier's preconditions
# ---------------------------------------------------------------------------------------------------------------------
def _fits(t: torch.Tensor, dtype) -> bool:
    return bool(torch.equal(round_to(t.double(), dtype), t.double()))


def _sum_ok(terms: torch.Tensor, quantum: float, extra: float = 0.0) -> bool:
    """Every term a multiple of ``quantum`` and, per column, sum |terms| (+ extra) < 2^24 quanta: any partial sum in any
    order is an fp32 value."""
    q = terms.double() / quantum
    return bool(torch.equal(q, q.round())) and float(q.abs().sum(0).max()) + extra / quantum < 2.0 ** 24


def exact_preconditions(kind: str, name: str) -> list:
    """The conditions under which the exact tier's claims hold, evaluated in float64; returns the ones that fail."""
    bad = []
    if kind == "eval":
        c = eval_case(name, "exact")
        x, w = c["x"], c["w"]
        d = _flat_u(head_model(x, w, c["b"], c["u"], 1.0, F32)["g"], F64)
        prods = x.double().reshape(-1, x.shape[-1]).abs() @ w.double().abs().t()
        ok = _fits(x, BF) and float(prods.max()) + 3 < 2 ** 24 and bool((d.abs() >= 1).all()) and bool(torch.equal(d, d.round()))
        return [] if ok and d.numel() < 2 ** 23 else ["eval operands"]
    c = (head_case if kind == "head" else tail_case)(name, "exact")
    coef = c["coef"]
    if coef not in (1.0, 0.25):
        bad.append(f"coef {coef}")
    q = coef / 4.0                        # invstd 1/2 and gamma 1/2 each halve the quantum of what they scale
    if kind == "head":
        m = head_model(c["x"], c["w"], c["b"], c["u"], coef, F64)
        act, da = c["x"].double(), m["dx"]
    else:
        m = tail_model(c["raw"], c["stats"], c["gamma"], c["w"], c["b"], c["u"], coef, F64)
        act, da = m["act"].double(), m["da"]
        if not _fits(c["raw"], BF):
            bad.append("raw not bf16")
    C = act.shape[-1]
    g = _flat_u(m["g"], F64)
    d = g / coef
    if not (bool(torch.equal(d, d.round())) and bool((d.abs() >= 1).all())):
        bad.append("v - u not a non-zero integer")
    if d.numel() >= 2 ** 23:
        bad.append("count")
    if not (_fits(act, BF) and _fits(da, BF)):
        bad.append("a T-stored value is not bf16-exact")
    vterms = act.reshape(-1, C).abs() @ c["w"].double().abs().t()
    if float(vterms.max()) + 3 + 2 >= 2 ** 24:
        bad.append("v")
    base = c["base"] or {}
    big = lambda k: float(base[k].abs().max()) if k in base else 0.0   # noqa: E731
    dw_abs = g.abs().t() @ act.reshape(-1, C).abs()                     # per (output, channel): sum over pixels of |g a|
    if not _sum_ok(g, q, big("db")) or float(dw_abs.max()) / q + big("dw") / q >= 2 ** 24:
        bad.append("dW / db")
    if kind == "tail":
        mean, invstd = c["stats"][0].double(), c["stats"][1].double()
        xh = (c["raw"].double() - mean) * invstd
        dz = torch.where(m["act"] > 0, da, torch.zeros_like(da))
        for k, t in (("dbeta", dz), ("dgamma", dz * xh)):
            t2 = t.reshape(-1, C)
            qq = t2 / q
            if not bool(torch.equal(qq, qq.round())) or float(qq.abs().sum(0).max()) + big(k) / q >= 2 ** 24:
                bad.append(k)
        n = xh.numel() // C
        if n & (n - 1) == 0:
            # c1, c2 and every intermediate of gamma invstd (dz - c1 - xhat c2) are fp32 values
            f = lambda t: bool(torch.equal(t.float().double(), t))     # noqa: E731
            t1, t2 = dz - m["c1"], xh * m["c2"]
            if not (f(m["c1"]) and f(m["c2"]) and f(xh) and f(t1) and f(t2) and f(t1 - t2) and f(m["draw_pre"])):
                bad.append("d raw")
    return bad
