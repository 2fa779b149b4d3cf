"""Every form of the kernels that end a training step or a validation pass against float64:
s2s_head_loss_fused, s2s_tail_fwd_loss + s2s_tail_bwd_apply (with the tail's BatchNorm sums) and s2s_head_mse_eval, row by
row of tests/head_tail_forms_ref.py, in bf16 and fp32, on poisoned memory, dense and as a channel slice of a NaN-filled
wider buffer (the two launches have to give the same bits, the slice's surroundings stay NaN, the inputs stay as they were).

Exact tier (integer operands, hand-made statistics rows, coef a power of two: every fp32 operation is exact, see
head_tail_forms_ref.exact_preconditions): v, g, dx, dW, db, dgamma, dbeta equal the float64 result bit for bit whatever
the order of the sums, the conv-bias gradient is exactly zero, every scalar loss is within 1 fp32 ulp of the float64 loss
(all d^2 are integers >= 1 and count < 2^23: a pixel counted twice or not at all moves it by at least 1 / count), and on
power-of-two pixel counts c1, c2 and d raw equal the rounded exact values.  On other counts those three are held as in
the real tier.

Real tier (normal / uniform operands): hard bounds, the project's own -- fp32 outputs 1e-4 in the max norm and in L2;
T-stored dx / d raw 4e-3 and, from 500 elements on, 2.2e-3 in L2 -- and, on top, K x the yardstick (the deviation of torch's
fp32 evaluation of the same quantity on the CPU from float64; relative max and L2 deviations, floored at 1e-7).  T-stored
tensors element by element: (1/2 + 1/64) ulp of T + K x the yardstick's largest absolute deviation before the store.  d raw
is evaluated with the means the kernel wrote into ``work``; c1 and c2 themselves are held to the model.  Scalar losses:
1e-6 relative to float64 for both storage types (both read the same bf16-exact values).

K = 4 x the largest ratio measured on the MI355X, rounded up to a power of two, per quantity and storage type (the row
that gave the largest ratio in brackets):

  head v      bf16  K 16  ratio 3.19  [3x10x10x96-o1]
  head v      fp32  K 16  ratio 3.19  [3x10x10x96-o1]
  head dw     bf16  K 8   ratio 1.78  [2x10x10x16-o4]
  head dw     fp32  K 8   ratio 1.78  [2x10x10x16-o4]
  head db     bf16  K 8   ratio 1.65  [1x8x8x32-o2]
  head db     fp32  K 8   ratio 1.65  [1x8x8x32-o2]
  head dx     bf16  K 2   ratio 0.31  [5x481x109x16-o2]
  head dx     fp32  K 16  ratio 3.16  [3x10x10x96-o1]
  tail v      bf16  K 8   ratio 1.10  [5x481x109x8-o2]
  tail v      fp32  K 8   ratio 1.29  [5x481x109x8-o2]
  tail g      bf16  K 8   ratio 1.41  [1x1x786433x8-o1]
  tail g      fp32  K 8   ratio 1.39  [2x5x7x128-o3]
  tail dw     bf16  K 16  ratio 2.92  [1x1x13x512-o1]
  tail dw     fp32  K 8   ratio 1.53  [2x8x12x32-o3]
  tail db     bf16  K 16  ratio 6.61  [1x1x13x512-o1]
  tail db     fp32  K 8   ratio 1.66  [1x5x7x8-o3]
  tail dgamma bf16  K 8   ratio 1.69  [2x10x10x16-o4]
  tail dgamma fp32  K 4   ratio 1.00  [37x1x1x64-o4]
  tail dbeta  bf16  K 4   ratio 0.60  [3x33x18x8-o4]
  tail dbeta  fp32  K 4   ratio 0.88  [1x2x4x256-o3]
  tail c1     bf16  K 4   ratio 0.52  [1x1x97x64-o3]
  tail c1     fp32  K 4   ratio 0.88  [1x2x4x256-o3]
  tail c2     bf16  K 16  ratio 2.41  [1x16x16x8-o1]
  tail c2     fp32  K 8   ratio 1.05  [3x4x4x128-o4]
  tail draw   bf16  K 8   ratio 1.20  [1x1x786433x8-o1]
  tail draw   fp32  K 8   ratio 1.07  [2x6x8x64-o2]

(tail db in bf16: 4 x 6.61 asks for 32.  A K above 16 is not adopted: the row has 13 pixels and one output, so db is ONE
number, the sum of 13 values of either sign, each carrying the rounding of a 512-term fp32 dot product, against a yardstick
of a single fp32 ulp, 1.19e-7; the error itself is 7.9e-7 of db.  It is held to K = 16.)

Chain equality: for every tail row, tail_fwd_loss + tail_bwd_apply equal bn_relu_apply -> head_loss_fused -> bn_relu_bwd
bit for bit (tests/test_tail_fused_gpu.py asserts that at three widths; since head_loss_fused takes every width the tail
takes it holds at all seven).  Refused shapes raise and leave their NaN-filled outputs untouched."""
import pytest
import torch

import head_tail_forms_ref as R
from test_wgrad_forms_gpu import _guards_intact, _slice_of_wide, poison  # noqa: F401  (poison: autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = R.BF, R.F32, R.F64
DTYPES = [BF, F32]
DT_IDS = ["bf16", "fp32"]
TIERS = ["exact", "real"]
NAN = float("nan")
TOL_F32 = (1e-4, 1e-4)
TOL_BF16 = (4e-3, 2.2e-3)
HALF = 0.5 + 1.0 / 64
LOSS_TOL = 1e-6

# (entry, quantity, storage type) -> K; the measurements are in the docstring
K = {
    ("head", "v", BF): 16,
    ("head", "v", F32): 16,
    ("head", "dw", BF): 8,
    ("head", "dw", F32): 8,
    ("head", "db", BF): 8,
    ("head", "db", F32): 8,
    ("head", "dx", BF): 2,
    ("head", "dx", F32): 16,
    ("tail", "v", BF): 8,
    ("tail", "v", F32): 8,
    ("tail", "g", BF): 8,
    ("tail", "g", F32): 8,
    ("tail", "dw", BF): 16,
    ("tail", "dw", F32): 8,
    ("tail", "db", BF): 16,
    ("tail", "db", F32): 8,
    ("tail", "dgamma", BF): 8,
    ("tail", "dgamma", F32): 4,
    ("tail", "dbeta", BF): 4,
    ("tail", "dbeta", F32): 4,
    ("tail", "c1", BF): 4,
    ("tail", "c1", F32): 4,
    ("tail", "c2", BF): 16,
    ("tail", "c2", F32): 8,
    ("tail", "draw", BF): 8,
    ("tail", "draw", F32): 8,
}


def _dn(dtype):
    return "bf16" if dtype == BF else "fp32"


def _hold(entry, row, q, got, ref, yard_val, dtype):
    """An fp32 output against the float64 model: the hard bound, then K x the yardstick."""
    err = R.deviation(got, ref)
    yard = R.deviation(yard_val, ref)
    rat = R.ratios(err, yard)
    k = K[(entry, q, dtype)]
    line = (f"RATIO {entry} {row} {_dn(dtype)} {q} {max(rat):.3f} | max {err[0]:.2e} l2 {err[1]:.2e} yardstick {yard[0]:.2e} "
            f"{yard[1]:.2e} K {k}")
    print(line)
    assert bool(torch.isfinite(got).all()), line
    assert err[0] < TOL_F32[0] and err[1] < TOL_F32[1], f"{line}: over the hard bound"
    assert max(rat) <= k, f"{line}: over K x yardstick"


def _hold_stored(entry, row, q, got, ref_pre, yard_pre, dtype):
    """A T-stored tensor against the unrounded float64 value: the norms, then element by element."""
    r = ref_pre.double()
    g = got.detach().cpu().double().reshape(r.shape)
    err = R.deviation(g, r)
    yard_abs = max(float((yard_pre.double() - r).abs().max()), R.YARD_FLOOR * float(r.abs().max()))
    over = ((g - r).abs() - HALF * R.ulp(r, dtype)).clamp_min(0.0)
    rat = float(over.max()) / max(yard_abs, 1e-300)
    k = K[(entry, q, dtype)]
    line = (f"RATIO {entry} {row} {_dn(dtype)} {q} {rat:.3f} | max {err[0]:.2e} l2 {err[1]:.2e} yardstick abs {yard_abs:.2e} "
            f"K {k} ({r.numel()} elements)")
    print(line)
    assert bool(torch.isfinite(g).all()), line
    tol = TOL_BF16 if dtype == BF else TOL_F32
    assert err[0] < tol[0], line
    assert (dtype == BF and r.numel() < 500) or err[1] < tol[1], line
    assert rat <= k, f"{line}: an element over (1/2 + 1/64) ulp + K x yardstick"


def _hold_loss(what, got, ref, exact):
    got, ref = float(got), float(ref)
    tol = float(R.ulp(torch.tensor(ref, dtype=F64), F32)) if exact else LOSS_TOL * abs(ref)
    print(f"{what}: loss {got!r} float64 {ref!r} off {abs(got - ref):.3e} bound {tol:.3e}")
    assert abs(got - ref) <= tol, what


def _bits(what, got, ref_f64):
    """Equality with the float64 result (which the exact tier makes an fp32 value): the same bits, but for the sign of a
    zero (a lone product g * 0 is -0 for g < 0 in the model's matrix product and +0 after the kernels' fmaf onto 0.f)."""
    ref = ref_f64.double()
    assert bool(torch.equal(ref.float().double(), ref)), f"{what}: the reference is not an fp32 value"
    g = got.detach().cpu().float().reshape(ref.shape)
    n = int((g.double() != ref).sum())
    assert n == 0, f"{what}: {n} of {ref.numel()} elements differ, largest {float((g.double() - ref).abs().max()):.3e}"


def _dev(t, dtype=F32):
    return None if t is None else t.to(dtype).to(DEV)


def _grads(base, keys_shapes, has_bias):
    out = {}
    for k, shape in keys_shapes.items():
        if k == "db" and not has_bias:
            out[k] = None
        elif base is not None:
            out[k] = base[k].reshape(shape).clone().to(DEV)
        else:
            out[k] = torch.full(shape, NAN, device=DEV)
    return out


def _layouts(t):
    """The tensor dense, and as channels [8, 8 + C) of a NaN-filled buffer 24 channels wider."""
    yield "dense", t, None
    view, wide = _slice_of_wide(t, 8, 16)
    yield "slice", view, wide


def _same_as_dense(what, outs, dense):
    for k, t in outs.items():
        if t is not None:
            assert R.same_bits(t, dense[k]), f"{what}: {k} of the channel slice differs from the dense launch"


# ---------------------------------------------------------------------------------------------------------------------
# fused head + loss
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", list(R.HEAD))
def test_head_loss_form(name, tier, dtype):
    from stain2stain_amd import ops
    (B, H, W, C), (cout, bias, want_v, acc, _gs, _walk), fam = R.HEAD[name]
    assert ops.head_loss_family(dtype, B, H, W, C, cout) == fam
    c = R.head_case(name, tier)
    w, b, u = _dev(c["w"]).reshape(cout, C, 1, 1), _dev(c["b"]), _dev(c["u"])
    keep = [t.clone() for t in (w, u)]
    dense = None
    for layout, x, wide in _layouts(_dev(c["x"], dtype)):
        x0 = x.clone()
        gr = _grads(c["base"], {"dw": (cout, C, 1, 1), "db": (cout,)}, bias)
        loss, dx, v = ops.head_loss_fused(x, w, b, u, gr["dw"], gr["db"], want_v=want_v, grad_scale=c["grad_scale"],
                                          accumulate=acc)
        torch.cuda.synchronize()
        assert (v is not None) == want_v and dx.dtype == dtype and dx.shape == x.shape
        assert R.same_bits(x.float(), x0.float()) and torch.equal(w, keep[0]) and torch.equal(u, keep[1])
        assert wide is None or _guards_intact(wide, 8, C)
        outs = dict(loss=loss, dx=dx.float(), v=v, dw=gr["dw"], db=gr["db"])
        if dense is None:
            dense = outs
        else:
            _same_as_dense(f"{name} {layout}", outs, dense)
    what = f"head {name} {_dn(dtype)} {tier}"
    ref = R.with_base(R.head_model(c["x"], c["w"], c["b"], c["u"], c["coef"], dtype, F64, staged=fam == R.PIXEL), c["base"])
    o = dense
    _hold_loss(what, o["loss"], ref["loss"], tier == "exact")
    if tier == "exact":
        for q in ("v", "dx", "dw", "db"):
            if o[q] is not None:
                _bits(f"{what} {q}", o[q], ref[q])
        return
    yard = R.with_base(R.head_model(c["x"], c["w"], c["b"], c["u"], c["coef"], dtype, F32, staged=fam == R.PIXEL), c["base"])
    for q in ("v", "dw", "db"):
        if o[q] is not None:
            _hold("head", name, q, o[q].detach().cpu().reshape(ref[q].shape), ref[q], yard[q], dtype)
    _hold_stored("head", name, "dx", o["dx"], ref["dx_pre"], yard["dx_pre"], dtype)


# ---------------------------------------------------------------------------------------------------------------------
# fused tail
# ---------------------------------------------------------------------------------------------------------------------
def _tail_once(ops, c, raw, dtype, shape, opt):
    (B, H, W, C), (cout, bias, want_v, acc, _gs, _walk) = shape, opt
    stats, gamma = _dev(c["stats"]), _dev(c["gamma"])
    w, b, u = _dev(c["w"]).reshape(cout, C, 1, 1), _dev(c["b"]), _dev(c["u"])
    shapes = {"dw": (cout, C, 1, 1), "db": (cout,), "dgamma": (C,), "dbeta": (C,), "dbias": (C,)}
    old, new = _grads(c["base"], shapes, bias), _grads(c["base"], shapes, bias)
    keep = [t.clone() for t in (stats, gamma, w, u)]
    # the chain
    act, _ = ops.bn_relu_apply(raw, stats[2], stats[3])
    loss_o, dact, v_o = ops.head_loss_fused(act, w, b, u, old["dw"], old["db"], want_v=True, grad_scale=c["grad_scale"],
                                            accumulate=acc)
    draw_o = ops.bn_relu_bwd(dact, None, raw, stats, gamma, old["dgamma"], old["dbeta"], old["dbias"], accumulate=acc)
    # the fused pair
    loss_n, g_n, v_n, work = ops.tail_fwd_loss(raw, stats, w, b, u, new["dw"], new["db"], new["dgamma"], new["dbeta"],
                                               new["dbias"], want_v=want_v, grad_scale=c["grad_scale"], accumulate=acc)
    draw_n = ops.tail_bwd_apply(raw, stats, w, g_n, gamma, work)
    torch.cuda.synchronize()
    assert (v_n is not None) == want_v and draw_n.shape == raw.shape and draw_n.dtype == dtype and g_n.shape == u.shape
    for t, t0 in zip((stats, gamma, w, u), keep):
        assert torch.equal(t, t0)
    from stain2stain_amd import _native
    nbn = _native.lib().s2s_bn_bwd_blocks(B, H, W, C)
    means = work[2 * C * nbn:].reshape(2, C)
    chain = dict(loss=loss_o, v=v_o if want_v else None, draw=draw_o.float(), **old)
    fused = dict(loss=loss_n, v=v_n, draw=draw_n.float(), **new)
    differ = [k for k, t in fused.items() if t is not None and not R.same_bits(t, chain[k])]
    assert not differ, f"fused tail differs from the chain in {differ}"
    fused.update(g=g_n, c1=means[0].clone(), c2=means[1].clone(), dact=dact.float())
    return fused


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", list(R.TAIL))
def test_tail_form(name, tier, dtype):
    from stain2stain_amd import ops
    shape, opt, fam = R.TAIL[name]
    (B, H, W, C), (cout, bias, want_v, acc, _gs, _walk) = shape, opt
    assert ops.tail_family(dtype, B, H, W, C, cout) == fam and ops.head_loss_family(dtype, B, H, W, C, cout) == fam[0]
    c = R.tail_case(name, tier)
    dense = None
    for layout, raw, wide in _layouts(_dev(c["raw"], dtype)):
        raw0 = raw.clone()
        outs = _tail_once(ops, c, raw, dtype, shape, opt)
        assert R.same_bits(raw.float(), raw0.float())
        assert wide is None or _guards_intact(wide, 8, C)
        if dense is None:
            dense = outs
        else:
            _same_as_dense(f"{name} {layout}", outs, dense)
    what = f"tail {name} {_dn(dtype)} {tier}"
    o = dense
    means = (o["c1"].cpu(), o["c2"].cpu())
    seen = o["dact"].cpu() if tier == "real" else None
    args = (c["raw"], c["stats"], c["gamma"], c["w"], c["b"], c["u"], c["coef"], dtype)
    ref = R.with_base(R.tail_model(*args, F64, da_seen=seen, means=means), c["base"])
    print(f"{what}: {ref['forced']} roundings of da taken from the kernel")
    assert ref["forced"] <= max(2, ref["da"].numel() // 1000)
    _hold_loss(what, o["loss"], ref["loss"], tier == "exact")
    # the conv-bias gradient: exactly zero, so an accumulating launch leaves the buffer as it was
    assert bool((o["dbias"] == 0).all()) if not acc else R.same_bits(o["dbias"], c["base"]["dbias"])
    pow2 = (B * H * W) & (B * H * W - 1) == 0
    if tier == "exact":
        for q in ("v", "g", "dw", "db", "dgamma", "dbeta"):
            if o[q] is not None:
                _bits(f"{what} {q}", o[q], ref[q])
        if pow2:
            _bits(f"{what} c1", o["c1"], ref["c1"])
            _bits(f"{what} c2", o["c2"], ref["c2"])
            _bits(f"{what} d raw", o["draw"], ref["draw"])
            return
    yard = R.with_base(R.tail_model(*args, F32, da_seen=seen, means=means), c["base"])
    qs = ("c1", "c2") if tier == "exact" else ("v", "g", "dw", "db", "dgamma", "dbeta", "c1", "c2")
    for q in qs:
        if o[q] is not None:
            _hold("tail", name, q, o[q].detach().cpu().reshape(ref[q].shape), ref[q], yard[q], dtype)
    _hold_stored("tail", name, "draw", o["draw"], ref["draw_forced_pre"], yard["draw_forced_pre"], dtype)


# ---------------------------------------------------------------------------------------------------------------------
# eval loss
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", list(R.EVAL))
def test_head_mse_eval_form(name, tier, dtype):
    from stain2stain_amd import ops
    (B, H, W, C), (cout, _bias), fam = R.EVAL[name]
    assert ops.head_mse_family(dtype, B, H, W, C, cout) == fam
    c = R.eval_case(name, tier)
    w, b, u = _dev(c["w"]), _dev(c["b"]), _dev(c["u"])
    keep = [t.clone() for t in (w, u)]
    ref = R.eval_model(c["x"], c["w"], c["b"], c["u"])
    first = None
    for layout, x, wide in _layouts(_dev(c["x"], dtype)):
        x0 = x.clone()
        loss = ops.head_mse_eval(x, w, b, u)
        torch.cuda.synchronize()
        assert R.same_bits(x.float(), x0.float()) and torch.equal(w, keep[0]) and torch.equal(u, keep[1])
        assert wide is None or _guards_intact(wide, 8, C)
        _hold_loss(f"eval {name} {_dn(dtype)} {tier} {layout}", loss, ref, tier == "exact")
        first = loss if first is None else first
        assert R.same_bits(loss, first)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_refused_shapes_raise_and_write_nothing(dtype):
    from stain2stain_amd import _native, ops
    L = _native.lib()
    for entry, (B, H, W, C, cout) in R.REFUSED:
        x = torch.ones(B, H, W, C, dtype=dtype, device=DEV)
        w = torch.ones(cout, C, 1, 1, device=DEV)
        u = torch.zeros(B, cout, H, W, device=DEV)
        outs = {k: torch.full(s, NAN, device=DEV) for k, s in
                (("dw", (cout, C, 1, 1)), ("db", (cout,)), ("dgamma", (C,)), ("dbeta", (C,)), ("dbias", (C,)))}
        stats = torch.ones(4, C, device=DEV)
        with pytest.raises(RuntimeError):
            if entry == "head":
                ops.head_loss_fused(x, w, outs["db"] * 0 + 1, u, outs["dw"], outs["db"], want_v=True)
            elif entry == "tail":
                ops.tail_fwd_loss(x, stats, w, None, u, outs["dw"], outs["db"], outs["dgamma"], outs["dbeta"], outs["dbias"])
            else:
                ops.head_mse_eval(x, w, None, u)
        if entry == "tail":
            # below ops.tail_fusable: the entry points themselves answer the family's status and launch nothing
            g = torch.full((B, cout, H, W), NAN, device=DEV)
            dx = torch.full((B, H, W, C), NAN, dtype=dtype, device=DEV)
            scratch = torch.full((4096,), NAN, device=DEV)
            lpart = torch.full((8,), NAN, dtype=F64, device=DEV)
            p = lambda t: t.data_ptr()                                              # noqa: E731
            rc = L.s2s_tail_fwd_loss(0 if dtype == BF else 1, p(x), C, p(stats[2]), p(stats[3]), p(stats[0]), p(stats[1]),
                                     p(w), None, p(u), None, p(g), 1.0, p(scratch), p(lpart), p(scratch), p(outs["dw"]),
                                     p(outs["db"]), p(scratch), p(outs["dgamma"]), p(outs["dbeta"]), p(outs["dbias"]), 0, B,
                                     H, W, C, cout, None)
            assert rc == L.s2s_tail_family(0 if dtype == BF else 1, B, H, W, C, cout) == R.ERR_SHAPE
            rc = L.s2s_tail_bwd_apply(0 if dtype == BF else 1, p(x), C, p(g), p(w), p(stats[2]), p(stats[3]), p(stats[0]),
                                      p(stats[1]), p(stats[0]), p(scratch), p(dx), C, B, H, W, C, cout, None)
            assert rc == R.ERR_SHAPE
            torch.cuda.synchronize()
            assert all(bool(torch.isnan(t).all()) for t in (g, dx, scratch, lpart))
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in outs.values()), (entry, C, cout)
