"""Row tables, launch-arithmetic predicates and float64 host models of the segmentation and ROI loss kernels, form by
form (a helper module of the suite, not a conftest; CPU only, no HIP calls in here):

  seg_loss.hip        s2s_seg_loss (seg_loss_reduce / _finalize / _bwd), s2s_seg_loss_multiclass (mc_reduce<C> /
                      mc_finalize / mc_bwd<C>, C = 2 ... 8)
  eval_metrics.hip    s2s_seg_eval_binary, s2s_seg_eval_multiclass (the two segmentation passes)
  loss_variants.hip   s2s_weighted_mse (lv_reduce<0>, lv_finalize, wmse_bwd), s2s_charbonnier_roi (lv_reduce<1>),
                      s2s_class_embed_add, s2s_class_embed_bwd

Models.  Every ``*_model(..., cd)`` evaluates the operation from the fp32 operands the kernel receives, written from the
formulas of the kernels' header comments, with ``cd = float64`` for the reference and ``cd = float32`` for the yardstick:
what torch's fp32 arithmetic on the CPU costs for the same quantity (deviations as relative max and
relative L2, floored at 1e-7).  Scalars that reach an entry point as a C ``float`` are rounded to fp32 first (``f32``).
tests/test_loss_forms_cpu.py holds the float64 models to torch's own float64 evaluation and autograd.

Launch arithmetic.  The constants of the launches are mirrored once, below; ``form`` names the form of a grid-stride loop
from glue_forms_ref.walk, and ``work_extent`` is the highest element of ``work`` a launcher writes.

A case holds the operands, the float64 reference and the yardstick's deviations (numbers, not tensors).  Cases are cached
and shared; treat them as read-only."""
from __future__ import annotations

import functools
import itertools

import torch

from glue_forms_ref import F32, F64, YARD_FLOOR, _gen, deviation, f32, ratios, same_bits, walk  # noqa: F401

# ---------------------------------------------------------------------------------------------------------------------
# launch constants (seg_loss.hip, eval_metrics.hip, loss_variants.hip) and the work sizes of include/stain2stain_hip.h
# ---------------------------------------------------------------------------------------------------------------------
THREADS = 256
PART_ROWS = 512                # SEG_BLOCKS, EV_BLOCKS, LV_BLOCKS: rows of per-workgroup partials
BWD_CAP = 4096                 # blocks of seg_loss_bwd_kernel, mc_bwd_kernel, wmse_bwd_kernel
MC_SUMS, MC_CNTS, MC_MAX = 26, 32, 8
WORK = {                       # doubles
    "seg_loss": 512 * 4 + 4,
    "seg_loss_multiclass": 513 * 26,
    "seg_eval_binary": 512 * 8,
    "seg_eval_multiclass": 512 * 58,
    "weighted_mse": 512 * 2 + 2,
    "charbonnier_roi": 512 * 2 + 2,
}
PART_WIDTH = {"seg_loss": 4, "seg_loss_multiclass": MC_SUMS, "seg_eval_binary": 4, "seg_eval_multiclass": MC_SUMS,
              "weighted_mse": 2, "charbonnier_roi": 2}
# what follows the PART_ROWS rows of partials: a block of sums, or (eval) one row of 64-bit counts per workgroup
SUMS_BLOCK = {"seg_loss": 4, "seg_loss_multiclass": MC_SUMS, "weighted_mse": 2, "charbonnier_roi": 2}
COUNT_WIDTH = {"seg_eval_binary": 4, "seg_eval_multiclass": MC_CNTS}


def work_extent(kind: str, items: int) -> int:
    """One past the highest double of ``work`` the launcher of ``kind`` writes for ``items`` elements / pixels: nb rows of
    partials from 0, then, from the fixed offset PART_ROWS * width, the sums block or nb rows of counts."""
    nb = walk(items, PART_ROWS)["grid"]
    k = PART_WIDTH[kind]
    assert nb * k <= PART_ROWS * k
    tail = SUMS_BLOCK[kind] if kind in SUMS_BLOCK else nb * COUNT_WIDTH[kind]
    return PART_ROWS * k + tail


def form(total: int, cap: int) -> str:
    """The form a grid-stride loop of ``cap`` blocks x 256 threads takes over ``total`` items."""
    w = walk(total, cap)
    if w["strides"]:
        return "stride-partial" if w["partial_last"] else "stride-whole"
    if w["grid"] == 1:
        return "one-ragged" if w["ragged"] else "one-full"
    return "blocks-ragged" if w["ragged"] else "blocks-full"


def reduce_form(items: int) -> str:
    return form(items, PART_ROWS)


def bwd_form(items: int) -> str:
    return form(items, BWD_CAP)


def _yard(fn) -> dict:
    """(float64 reference, {quantity: (rel max, rel L2)} of the fp32 evaluation against it); "out-each" holds the
    deviations of the elements of ``out`` one by one, so that seg, dice and bce / ce are each held alone."""
    ref, y = fn(F64), fn(F32)
    yard = {k: deviation(y[k], ref[k]) for k in ref if torch.is_tensor(ref[k])}
    yard["out-each"] = [deviation(y["out"][i:i + 1], ref["out"][i:i + 1]) for i in range(ref["out"].numel())] if "out" in ref else []
    return ref, yard


# ---------------------------------------------------------------------------------------------------------------------
# binary Dice + BCE (loss and eval)
# ---------------------------------------------------------------------------------------------------------------------
BIN_REDUCE_EDGE = PART_ROWS * THREADS                  # 131 072: 512 blocks, no stride
BIN_STRIDING = BWD_CAP * THREADS + 777                 # 1 049 353: the backward strides, ragged last round
BIN_N = [1, 255, 256, 257, BIN_REDUCE_EDGE, BIN_REDUCE_EDGE + 1, BIN_STRIDING]
BIN_SPECIALS = [0.0, 1e-30, -1e-30, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0]
KNIFE = [0.0, -1e-8, 1e-8, 6e-8, 1.2e-7, 1e-6]
KNIFE_N = 300
# An fp32 result below 2^-126 may be flushed to zero.  In seg_loss_bwd_kernel that can happen to exp(-|z|), to the smaller
# of p and 1 - p, to their product, to (p - g) / n and to the products with dice_w, 1 - dice_w and scale: fewer than eight
# places, and what multiplies a flushed value on its way to dz is a product of p <= 1, dice_w <= 1, scale <= 1, 1 / n <= 1
# and |g a - b| <= a + b with a = 2 / (P + G + s) and b = (2 I + s) / (P + G + s)^2, both below 1 on the specials row
# (G = 9).  So 8 x 2 x 2^-126 bounds it, as 2^-119 does for SiLU in glue_forms_ref.
BIN_UNDERFLOW = 2.0 ** -122


def _bin(name, n, mask="random", dw=0.3, smooth=1.0, gs=1.0, logits="normal"):
    return name, dict(n=n, mask=mask, dw=dw, smooth=smooth, gs=gs, logits=logits)


BIN_ROWS = dict(
    [_bin(f"n{n}", n) for n in BIN_N]
    + [_bin(f"n{n}-dw{dw:g}", n, dw=dw) for n in (257, BIN_STRIDING) for dw in (1.0, 0.0)]
    + [_bin(f"n{n}-smooth1e-6", n, smooth=1e-6) for n in (257, BIN_STRIDING)]
    + [_bin(f"n{n}-gs0.25", n, gs=0.25) for n in (1, 257, BIN_STRIDING)]
    + [_bin(f"n{n}-mask-{m}", n, mask=m) for n in (257, BIN_REDUCE_EDGE + 1) for m in ("zeros", "ones")]
    + [_bin("n257-mask-zeros-smooth1e-6-dw1", 257, mask="zeros", smooth=1e-6, dw=1.0)]
    + [_bin(f"specials-dw{dw:g}", 2 * len(BIN_SPECIALS), mask="specials", dw=dw, logits="specials") for dw in (1.0, 0.0, 0.3)]
    + [_bin("knife-edge", KNIFE_N, logits="knife")]
)
BIN_OPS_ROWS = ["n257", f"n{BIN_STRIDING}-gs0.25"]            # the wrappers against the direct call: small, striding


def away(z: torch.Tensor) -> torch.Tensor:
    """Logits with |z| < 1e-3 moved away from the threshold of sigmoid(z) > 0.5 (tests/test_eval_metrics_gpu._logits)."""
    z = z.clone()
    z[z.abs() < 1e-3] = 0.5
    return z


def bin_model(z, g, smooth, dw, gs, cd=F64) -> dict:
    """seg = dw (1 - (2 I + s) / (P + G + s)) + (1 - dw) mean(max(z, 0) - z g + log(1 + exp(-|z|))) and
    dz = gs (dw d dice + (1 - dw) (p - g) / n), d dice = -[2 g (P + G + s) - (2 I + s)] / (P + G + s)^2 p (1 - p)."""
    s, dw, gs = f32(smooth), f32(dw), f32(gs)
    z, g = z.to(cd), g.to(cd)
    p = torch.sigmoid(z)
    I, P, G = (p * g).sum(), p.sum(), g.sum()
    den = P + G + s
    dice = 1.0 - (2.0 * I + s) / den
    bce = (z.clamp_min(0.0) - z * g + torch.log1p(torch.exp(-z.abs()))).mean()
    q = torch.sigmoid(-z)                                   # 1 - p without the cancellation
    ddice = -(2.0 * g * den - (2.0 * I + s)) / (den * den) * p * q
    p_minus_g = torch.where(z >= 0, (1.0 - g) - q, p - g)
    dbce = p_minus_g / z.numel()
    return dict(out=torch.stack([dw * dice + (1.0 - dw) * bce, dice, bce]), dz=gs * (dw * ddice + (1.0 - dw) * dbce),
                a=float(2.0 / den), b=float((2.0 * I + s) / (den * den)))


def bin_counts(z, g, lo: bool) -> list:
    """{I, P, G, U} of pred = z >= 1e-6 (``lo``) or pred = z > 0: the band sigmoid(z) > 0.5 in fp32 lies in."""
    pred = (z >= 1e-6) if lo else (z > 0)
    m = g != 0
    return [int((pred & m).sum()), int(pred.sum()), int(m.sum()), int((pred | m).sum())]


def metric_model(I, PG, U) -> tuple:
    """dice_coef = (2 I + 1e-7) / (P + G + 1e-7), iou = (I + 1e-7) / (U + 1e-7) in float64."""
    return (2.0 * I + 1e-7) / (PG + 1e-7), (I + 1e-7) / (U + 1e-7)


@functools.lru_cache(maxsize=None)
def bin_case(name: str) -> dict:
    r = BIN_ROWS[name]
    n, gen = r["n"], _gen("bin", name)
    if r["logits"] == "specials":
        z = torch.tensor(BIN_SPECIALS + BIN_SPECIALS, dtype=F32)
        g = torch.cat([torch.zeros(len(BIN_SPECIALS)), torch.ones(len(BIN_SPECIALS))])
    else:
        if r["logits"] == "knife":
            z = torch.tensor(KNIFE, dtype=F32).repeat(n // len(KNIFE))
        else:
            z = away(torch.randn(n, generator=gen) * 3.0)
        g = {"random": (torch.rand(n, generator=gen) < 0.4).float(), "zeros": torch.zeros(n), "ones": torch.ones(n)}[r["mask"]]
    ref, yard = _yard(lambda cd: bin_model(z, g, r["smooth"], r["dw"], r["gs"], cd))
    return dict(r, z=z, g=g, ref=ref, yard=yard, counts_lo=bin_counts(z, g, True), counts_hi=bin_counts(z, g, False))


# ---------------------------------------------------------------------------------------------------------------------
# multiclass softmax Dice + cross entropy (loss and eval)
# ---------------------------------------------------------------------------------------------------------------------
MC_C = [2, 3, 4, 5, 6, 7, 8]
MC_SHAPES = [(5, 1), (3, 85), (1, 256), (2, 257), (3, 43_699)]
MC_STRIDING = (3, 349_537)                             # 1 048 611 pixels: the backward strides; C = 2 and 8 only
MC_STRIDING_C = [2, 8]
MC_VARIANT_SHAPE = (2, 257)
MC_VARIANT_C = [2, 5, 8]
MC_VARIANTS = {
    "ignore-100": dict(ignore="none"), "ignore0": dict(ignore="first"), "ignore-last": dict(ignore="last"),
    "absent": dict(absent=True), "x4": dict(scale=4.0), "x40": dict(scale=40.0), "dw1": dict(dw=1.0), "dw0": dict(dw=0.0),
    "smooth1e-6": dict(smooth=1e-6), "gs0.25": dict(gs=0.25), "all-ignored": dict(ignore="last", all_ignored=True),
}
_MC_IGNORE = ("none", "first", "last")


def _mc(name, B, HW, C, ignore="none", absent=False, scale=1.0, dw=0.3, smooth=1.0, gs=1.0, all_ignored=False):
    return name, dict(B=B, HW=HW, C=C, ignore={"none": -100, "first": 0, "last": C - 1}[ignore], absent=absent, scale=scale,
                      dw=dw, smooth=smooth, gs=gs, all_ignored=all_ignored)


MC_ROWS = dict(
    [_mc(f"{B}x{HW}-C{C}", B, HW, C, ignore=_MC_IGNORE[(i + C) % 3]) for i, (B, HW) in enumerate(MC_SHAPES) for C in MC_C]
    + [_mc(f"{MC_STRIDING[0]}x{MC_STRIDING[1]}-C{C}", *MC_STRIDING, C, ignore="last", gs=0.25) for C in MC_STRIDING_C]
    + [_mc(f"{v}-C{C}", *MC_VARIANT_SHAPE, C, **kw) for v, kw in MC_VARIANTS.items() for C in MC_VARIANT_C]
)
MC_OPS_ROWS = ["3x85-C5", f"{MC_STRIDING[0]}x{MC_STRIDING[1]}-C8"]


def mc_model(z, t, ignore: int, smooth, dw, gs, cd=F64) -> dict:
    """z [B, C, HW], t [B, HW] in [0, C).  Dice over the pixels with t != ignore (every pixel when ignore < 0), mean over
    the classes; cross entropy as the mean over the pixels with t != ignore (0 / 0 = NaN when there are none, with a zero
    gradient); dz = gs (dw d dice + (1 - dw) d ce)."""
    s, dw, gs = f32(smooth), f32(dw), f32(gs)
    B, C, HW = z.shape
    z = z.to(cd)
    m = z.max(1, keepdim=True).values
    e = torch.exp(z - m)
    se = e.sum(1, keepdim=True)
    p = e / se
    lse = (m + torch.log(se))[:, 0]
    oh = (t[:, None, :] == torch.arange(C)[None, :, None]).to(cd)
    keep = (t != ignore)
    vd = (keep if ignore >= 0 else torch.ones_like(keep)).to(cd)[:, None, :]
    I, P, G = (p * oh * vd).sum((0, 2)), (p * vd).sum((0, 2)), (oh * vd).sum((0, 2))
    den = P + G + s
    dice = 1.0 - ((2.0 * I + s) / den).mean()
    nv = keep.sum()
    zt = (z * oh).sum(1)
    ce = ((lse - zt) * keep.to(cd)).sum() / nv.to(cd)
    a = -((2.0 / den)[None, :, None] * oh - ((2.0 * I + s) / (den * den))[None, :, None]) / C * vd
    ddice = p * (a - (a * p).sum(1, keepdim=True))
    dce = torch.where(keep[:, None, :], (p - oh) / nv.clamp_min(1).to(cd), torch.zeros((), dtype=cd))
    return dict(out=torch.stack([dw * dice + (1.0 - dw) * ce, dice, ce]), dz=gs * (dw * ddice + (1.0 - dw) * dce))


def first_argmax(z: torch.Tensor) -> torch.Tensor:
    """The first maximal class index of z [B, C, HW], written out (no reliance on an argmax's tie rule)."""
    C = z.shape[1]
    idx = torch.arange(C)[None, :, None].expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, idx, torch.full_like(idx, C)).min(1).values


def mc_counts(z, t, C: int) -> torch.Tensor:
    """int64 [4, C]: I_c, P_c, G_c, U_c of pred = first argmax (P counts every pixel, ignored targets included)."""
    pred = first_argmax(z)
    rows = []
    for c in range(C):
        pc, gc = pred == c, t == c
        rows.append([int((pc & gc).sum()), int(pc.sum()), int(gc.sum()), int((pc | gc).sum())])
    return torch.tensor(rows, dtype=torch.int64).T.contiguous()


def mc_metric_model(counts: torch.Tensor, ignore: int) -> tuple:
    """Mean over c != ignore of the float64 dice_coef and iou of the counts."""
    d, i = [], []
    for c in range(counts.shape[1]):
        if c == ignore:
            continue
        I, P, G, U = (float(x) for x in counts[:, c])
        dc, io = metric_model(I, P + G, U)
        d.append(dc)
        i.append(io)
    return sum(d) / len(d), sum(i) / len(i)


@functools.lru_cache(maxsize=None)
def mc_case(name: str) -> dict:
    r = MC_ROWS[name]
    B, HW, C, gen = r["B"], r["HW"], r["C"], _gen("mc", name)
    z = torch.randn(B, C, HW, generator=gen) * 3.0 * r["scale"]
    z[:, 1, ::3] = z[:, 0, ::3]                            # exact ties between two classes on every third pixel
    t = torch.randint(0, C, (B, HW), generator=gen)
    absent = None
    if r["absent"]:
        absent = C // 2
        t[t == absent] = (absent + 1) % C
    if r["all_ignored"]:
        t = torch.full((B, HW), r["ignore"], dtype=torch.int64)
    ref, yard = _yard(lambda cd: mc_model(z, t, r["ignore"], r["smooth"], r["dw"], r["gs"], cd))
    return dict(r, z=z, t=t, absent=absent, ref=ref, yard=yard, counts=mc_counts(z, t, C))


# ---------------------------------------------------------------------------------------------------------------------
# ROI-weighted MSE and ROI Charbonnier
# ---------------------------------------------------------------------------------------------------------------------
LV_SHAPES = [(1, 1, 1, 1), (1, 1, 5, 7), (3, 4, 5, 17), (2, 3, 16, 16), (2, 3, 257, 255), (2, 3, 257, 256), (3, 3, 600, 583)]
LV_SMALL, LV_STRIDING = (2, 3, 16, 16), (3, 3, 600, 583)


def _sid(s) -> str:
    return "x".join(map(str, s))


def _wm(name, shape, lam=10.0, mask="random", gs=1.0):
    return name, dict(shape=shape, lam=lam, mask=mask, gs=gs)


WMSE_ROWS = dict(
    [_wm(_sid(s), s) for s in LV_SHAPES]
    + [_wm(f"{_sid(s)}-{v}", s, **kw) for s in (LV_SMALL, LV_STRIDING)
       for v, kw in (("lam0", dict(lam=0.0)), ("empty", dict(mask="empty")), ("full", dict(mask="full")), ("gs0.25", dict(gs=0.25)),
                     ("lam0-gs0.25-full", dict(lam=0.0, gs=0.25, mask="full")))]
)
WMSE_OPS_ROWS = [_sid(LV_SMALL), f"{_sid(LV_STRIDING)}-gs0.25"]


def _cb(name, shape, eps_charb=1e-3, eps_area=1e-8, mask="random", same=False):
    return name, dict(shape=shape, eps_charb=eps_charb, eps_area=eps_area, mask=mask, same=same)


CHARB_ROWS = dict(
    [_cb(_sid(s), s) for s in LV_SHAPES]
    + [_cb(f"{_sid(LV_SMALL)}-{v}", LV_SMALL, **kw)
       for v, kw in (("charb1e-6", dict(eps_charb=1e-6)), ("same", dict(same=True)),
                     ("same-charb1e-6-area1", dict(same=True, eps_charb=1e-6, eps_area=1.0)), ("area1", dict(eps_area=1.0)), ("empty", dict(mask="empty")), ("empty-area1", dict(mask="empty", eps_area=1.0)),
                     ("full", dict(mask="full")))]
    + [_cb(f"{_sid(LV_STRIDING)}-full-area1", LV_STRIDING, mask="full", eps_area=1.0)]
)
CHARB_OPS_ROWS = [_sid(LV_SMALL), _sid(LV_STRIDING)]


def _lv_operands(kind, name, shape, mask):
    B, C, H, W = shape
    gen = _gen(kind, name)
    a, b = torch.rand(B, C, H * W, generator=gen), torch.rand(B, C, H * W, generator=gen) * 2 - 1
    m = {"random": (torch.rand(B, H * W, generator=gen) < 0.4).float(), "empty": torch.zeros(B, H * W), "full": torch.ones(B, H * W)}[mask]
    return a, b, m


def wmse_model(v, u, m, lam, gs, cd=F64) -> dict:
    """w = 1 + lam m over the channels; loss = sum(w (v - u)^2) / (sum(w) + 1e-8); dv = gs 2 w (v - u) / (sum(w) + 1e-8)."""
    lam, gs = f32(lam), f32(gs)
    v, u = v.to(cd), u.to(cd)
    w = (1.0 + lam * m.to(cd))[:, None, :].expand_as(v)
    d = v - u
    den = w.sum() + 1e-8
    return dict(out=((w * d * d).sum() / den).reshape(1), dv=gs * 2.0 * w * d / den)


def mse_model(v, u, gs) -> dict:
    """The plain float64 MSE the lam = 0 rows are also held to (the model of s2s_mse_loss)."""
    d = v.double() - u.double()
    return dict(out=(d * d).mean().reshape(1), dv=f32(gs) * 2.0 * d / d.numel())


def charb_model(a, b, m, eps_charb, eps_area, cd=F64) -> torch.Tensor:
    """sum(sqrt((a - b)^2 + eps_charb^2) m) / (sum(m) C + eps_area), m over the channels."""
    ec, ea = f32(eps_charb), f32(eps_area)
    a, b, m = a.to(cd), b.to(cd), m.to(cd)
    d = a - b
    num = (torch.sqrt(d * d + ec * ec) * m[:, None, :]).sum()
    return dict(out=(num / (m.sum() * a.shape[1] + ea)).reshape(1))


@functools.lru_cache(maxsize=None)
def wmse_case(name: str) -> dict:
    r = WMSE_ROWS[name]
    v, u, m = _lv_operands("wmse", name, r["shape"], r["mask"])
    ref, yard = _yard(lambda cd: wmse_model(v, u, m, r["lam"], r["gs"], cd))
    return dict(r, v=v, u=u, m=m, ref=ref, yard=yard)


@functools.lru_cache(maxsize=None)
def charb_case(name: str) -> dict:
    r = CHARB_ROWS[name]
    a, b, m = _lv_operands("charb", name, r["shape"], r["mask"])
    if r["same"]:
        b = a.clone()
    ref, yard = _yard(lambda cd: charb_model(a, b, m, r["eps_charb"], r["eps_area"], cd))
    return dict(r, a=a, b=b, m=m, ref=ref, yard=yard)


# ---------------------------------------------------------------------------------------------------------------------
# class embedding
# ---------------------------------------------------------------------------------------------------------------------
# (B, dim, classes): the issue's five rows, and one whose table takes two blocks with a ragged last one (classes * dim =
# 300; the five have 4, 96, 768 = 3 x 256, 10 240 = 40 x 256 and 252 elements)
EMBED = [(1, 4, 1), (3, 32, 3), (16, 256, 3), (5, 1024, 10), (600, 36, 7), (4, 100, 3)]
EMBED_LABELS = ("one", "absent", "every")
EMBED_ROWS = {f"{B}x{d}x{k}-{lab}": dict(B=B, dim=d, classes=k, labels=lab) for (B, d, k), lab in itertools.product(EMBED, EMBED_LABELS)}
EMBED_OPS_ROWS = ["3x32x3-every", "600x36x7-absent"]


def embed_labels(B: int, classes: int, kind: str, gen) -> torch.Tensor:
    """all one class | the last class absent (where there are two) | every class that B samples can hold, in turn."""
    if kind == "one" or classes == 1:
        return torch.full((B,), classes // 2, dtype=torch.int64)
    if kind == "absent":
        return torch.randint(0, classes - 1, (B,), generator=gen)
    return torch.arange(B, dtype=torch.int64) % classes


def embed_add_model(temb, table, y, cd=F64) -> torch.Tensor:
    return temb.to(cd) + table.to(cd)[y]


def embed_bwd_sequential(dout, y, classes: int) -> torch.Tensor:
    """dtable as class_embed_bwd_kernel states it: per element an fp32 sum over the batch in index order from +0."""
    s = torch.zeros(classes, dout.shape[1], dtype=F32)
    for b in range(dout.shape[0]):
        s[int(y[b])] += dout[b]
    return s


def embed_bwd_model(dout, y, classes: int, cd=F64) -> dict:
    return dict(dtable=torch.zeros(classes, dout.shape[1], dtype=cd).index_add_(0, y, dout.to(cd)))


@functools.lru_cache(maxsize=None)
def embed_case(name: str) -> dict:
    r = EMBED_ROWS[name]
    B, dim, k, gen = r["B"], r["dim"], r["classes"], _gen("embed", name)
    temb, table = torch.randn(B, dim, generator=gen), torch.randn(k, dim, generator=gen) * 0.5
    dout, base = torch.randn(B, dim, generator=gen), torch.randn(k, dim, generator=gen)
    y = embed_labels(B, k, r["labels"], gen)
    ref, yard = _yard(lambda cd: embed_bwd_model(dout, y, k, cd))
    present = torch.zeros(k, dtype=torch.bool)
    present[y] = True
    return dict(r, temb=temb, table=table, dout=dout, base=base, y=y, ref=ref, yard=yard, present=present,
                seq=embed_bwd_sequential(dout, y, k))
