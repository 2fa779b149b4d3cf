"""Every form of the optimiser, packing, layout and flow-glue kernels against float64, row by row of
tests/glue_forms_ref.py: the Adam family, s2s_pack_conv3x3 / _batched, the two layout conversions, s2s_pixel_sum, the time
path (embedding, linear, SiLU), s2s_cfm_sample, s2s_mse_loss, s2s_ode_error_norm, s2s_axpy, s2s_euler_tick, s2s_fill_f32.

Every output starts as NaN (torch.empty through the ``poison`` fixture, or a NaN-filled buffer of the test's own);
in-place operands and buffers a launch accumulates onto sit between sentinel guard elements that must be intact
afterwards; operands with a pixel stride run dense and as a channel slice of a wider NaN-filled buffer (the same bits, the
surroundings still NaN).

Exact claims: the forms of Adam agree bit for bit (adam_step = adam_step_dev = adam_multi = the p, m, v of adam_ema_step
and adam_ema_step_dev; with g = m = v = 0 and no weight decay p keeps its bits); packing and layout conversion equal the
permutation of torch's round-to-nearest-even values, padded lanes +0; accumulate equals torch's single fp32 add; the exact
tiers (small integers) of pixel_sum, linear and mse equal float64; ut = torch's fp32 x1 - x0; t = 0 / 1 give x0 / x1.

Bounded claims: the project's hard bounds (Adam 1e-6 of the largest value, pixel_sum 1e-4, linear 1e-6 forward and 1e-5
backward, time embedding / SiLU / cfm / mse / error norm 1e-6) and, on top, K x the yardstick: the deviation of torch's
fp32 evaluation of the same quantity on the CPU from float64 (relative max and L2, floored at 1e-7).  Adam's p element by
element: (1/2 + 1/64) fp32 ulp of the reference + K x the yardstick's largest absolute deviation of the update.

K = 4 x the largest ratio measured on the MI355X over the table, rounded up to a power of two (the row in brackets):

  adam m       K 4  ratio 1.000  [n1 step1000 v-positive]
  adam v       K 4  ratio 1.000  [n1 step2-wd-gs v-zeros]
  adam ema     K 4  ratio 0.996  [n2098179 step1e6 v-positive]
  adam p       K 4  ratio 0.977  [n257 step1e6 v-zeros]
  pixsum bf16  K 8  ratio 1.027  [B3 HW1000 C64 acc1]
  pixsum fp32  K 8  ratio 1.027  [B3 HW1000 C64 acc1]   (both types read the same bf16-exact values)
  temb         K 4  ratio 0.918  [dim1024 B600]
  lin y        K 8  ratio 1.013  [2x40x56 bias1]
  lin dx       K 4  ratio 0.839  [5x32x48 db1 dx1 acc0]
  lin dw       K 4  ratio 1.000  [5x32x48 db1 dx1 acc0]
  lin db       K 4  ratio 0.885  [7x256x1024 db1 dx1 acc1]
  silu a       K 4  ratio 0.923  [n5120]
  silu dh      K 4  ratio 1.000  [n255]
  cfm xt       K 4  ratio 0.792  [3x1398400 sigma0.1 t0]
  mse dv       K 4  ratio 0.597  [count1049776 gs1.0]
  err norm     K 4  ratio 0.915  [n1 atol0 rtol0.001]

No quantity asks for more than 16: these kernels perform the roundings of torch's fp32 evaluation, most of them in the
same order (a ratio of 1.000 is the same error to three digits).

Refused launches (C % 8, ld % 8, per_sample % 4, a misaligned view) raise and leave their NaN-filled outputs untouched."""
import pytest
import torch

import glue_forms_ref as R
from test_wgrad_forms_gpu import _guards_intact, _slice_of_wide, poison  # noqa: F401  (poison: autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, F64 = R.BF, R.F32, R.F64
DTYPES = [BF, F32]
DT_IDS = ["bf16", "fp32"]
TIERS = ["exact", "real"]
NAN = float("nan")
HALF = 0.5 + 1.0 / 64
G = 8                                  # guard elements on either side (32 bytes of fp32: 16-byte alignment is kept)
SENT = -1216.0                         # a bf16 value too

# quantity -> K; the measurements are in the docstring
K = {
    "adam m": 4, "adam v": 4, "adam ema": 4, "adam p": 4,
    "pixsum bf16": 8, "pixsum fp32": 8,
    "temb": 4, "lin y": 8, "lin dx": 4, "lin dw": 4, "lin db": 4, "silu a": 4, "silu dh": 4,
    "cfm xt": 4, "mse dv": 4, "err norm": 4,
}


def _dn(dtype):
    return "bf16" if dtype == BF else "fp32"


def _code(dtype):
    return 0 if dtype == BF else 1


def _hold(q, row, got, ref, yard_val, hard):
    """An fp32 output against the float64 model: finite, the hard bound, then K x the yardstick."""
    got = got.detach().cpu().reshape(ref.shape)
    err = R.deviation(got, ref)
    yard = R.deviation(yard_val, ref)
    rat = R.ratios(err, yard)
    line = (f"RATIO {q} | {row} | {max(rat):.3f} | max {err[0]:.2e} l2 {err[1]:.2e} yardstick {yard[0]:.2e} {yard[1]:.2e} "
            f"K {K[q]}")
    print(line)
    assert bool(torch.isfinite(got).all()), line
    assert err[0] < hard and err[1] < hard, f"{line}: over the hard bound {hard}"
    assert max(rat) <= K[q], f"{line}: over K x yardstick"


def _guarded(t, dtype=None):
    """A CPU tensor as the middle of a GPU buffer with G sentinel elements on either side: (view, buffer)."""
    n = t.numel()
    buf = torch.full((n + 2 * G,), SENT, dtype=dtype or t.dtype, device=DEV)
    buf[G:G + n] = t.reshape(-1).to(DEV)
    return buf[G:G + n].view(t.shape), buf


def _nan_guarded(shape, dtype=F32):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * G,), SENT, dtype=dtype, device=DEV)
    buf[G:G + n] = NAN
    return buf[G:G + n].view(shape), buf


def _intact(*bufs):
    return all(bool((b[:G] == SENT).all()) and bool((b[-G:] == SENT).all()) for b in bufs)


def _same_stored(got, ref_f32, dtype):
    """Bit equality of a T-stored tensor with the reference's T-rounded values (kept in fp32)."""
    ref = ref_f32.to(got.device).to(dtype).reshape(-1)
    it = torch.int16 if dtype == BF else torch.int32
    return got.numel() == ref.numel() and bool(torch.equal(got.contiguous().reshape(-1).view(it), ref.view(it)))


def _equal_values(what, got, ref_f64):
    """Equality with the float64 result (which the exact tier makes an fp32 value) but for the sign of a zero: a lone
    product x * 0 is -0 in a matrix product and +0 after the kernels' fmaf onto 0.f."""
    ref = ref_f64.double()
    assert bool(torch.equal(ref.float().double(), ref)), f"{what}: the reference is not an fp32 value"
    g = got.detach().cpu().double().reshape(ref.shape)
    n = int((g != ref).sum())
    assert n == 0, f"{what}: {n} of {ref.numel()} elements differ"


def _layouts(t):
    """An NHWC tensor dense, and as channels [8, 8 + C) of a NaN-filled buffer 24 channels wider."""
    yield "dense", t, None
    view, wide = _slice_of_wide(t, 8, 16)
    yield "slice", view, wide


# ---------------------------------------------------------------------------------------------------------------------
# Adam family
# ---------------------------------------------------------------------------------------------------------------------
ADAM_KINDS = ("step", "dev", "multi", "ema", "ema_dev")


def _adam_kw(sc):
    return {k: sc[k] for k in ("step", "lr", "beta1", "beta2", "eps", "weight_decay", "grad_scale")}


def _adam_multi(ops, tensors, sc):
    """One launch of s2s_adam_multi over [(p, g, m, v)]."""
    L = ops._L()
    rows, start = [], 0
    for p, g, m, v in tensors:
        rows.append([p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), start])
        start += L.s2s_adam_multi_blocks(p.numel())
    desc = torch.tensor(rows, dtype=torch.int64).to(DEV)
    rc = L.s2s_adam_multi(desc.data_ptr(), len(rows), start, sc["step"], sc["lr"], sc["beta1"], sc["beta2"], sc["eps"],
                          sc["weight_decay"], sc["grad_scale"], ops._stream())
    assert rc == 0
    torch.cuda.synchronize()


def _adam_run(ops, kind, c, sc):
    views, bufs = {}, []
    for k in ("p", "g", "m", "v", "ema"):
        views[k], b = _guarded(c[k])
        bufs.append(b)
    p, g, m, v, e = (views[k] for k in ("p", "g", "m", "v", "ema"))
    kw = _adam_kw(sc)
    hyper = lambda: torch.tensor(ops.adam_hyper(*kw.values()), dtype=F32, device=DEV)      # noqa: E731
    if kind == "step":
        ops.adam_step_(p, g, m, v, **kw)
    elif kind == "dev":
        ops.adam_step_dev_(p, g, m, v, hyper())
    elif kind == "multi":
        _adam_multi(ops, [(p, g, m, v)], sc)
    elif kind == "ema":
        ops.adam_ema_step_(p, g, m, v, e, **kw, ema_weight=sc["ema_weight"])
    else:
        ops.adam_ema_step_dev_(p, g, m, v, e, hyper(), torch.tensor([sc["ema_weight"]], dtype=F32, device=DEV))
    torch.cuda.synchronize()
    assert _intact(*bufs), f"{kind}: a guard element was written"
    assert R.same_bits(g, c["g"]), f"{kind}: the gradient changed"
    if kind in ("step", "dev", "multi"):
        assert R.same_bits(e, c["ema"])
    return {k: t.cpu() for k, t in views.items()}


def _hold_p(row, got, ref, yard):
    """p element by element: one rounding of the subtraction + K x what the update itself costs in fp32."""
    r, g = ref["p"], got.double()
    err = R.deviation(g, r)
    yard_abs = max(float((yard["upd"].double() - ref["upd"]).abs().max()), R.YARD_FLOOR * float(ref["upd"].abs().max()))
    over = ((g - r).abs() - HALF * R.ulp(r, F32)).clamp_min(0.0)
    rat = float(over.max()) / max(yard_abs, 1e-300)
    line = f"RATIO adam p | {row} | {rat:.3f} | max {err[0]:.2e} l2 {err[1]:.2e} yardstick abs {yard_abs:.2e} K {K['adam p']}"
    print(line)
    assert bool(torch.isfinite(g).all()) and err[0] < 1e-6, line
    assert rat <= K["adam p"], f"{line}: an element over (1/2 + 1/64) ulp + K x yardstick"


@pytest.mark.parametrize("name", list(R.ADAM_SCALARS))
@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_adam_forms(n, name):
    from stain2stain_amd import ops
    sc = R.ADAM_SCALARS[name]
    for vs in R.ADAM_V_STARTS:
        c = R.adam_case(n, vs)
        row = f"n{n} {name} v-{vs}"
        out = {kind: _adam_run(ops, kind, c, sc) for kind in ADAM_KINDS}
        for kind in ADAM_KINDS[1:]:
            differ = [q for q in ("p", "m", "v") if not R.same_bits(out[kind][q], out["step"][q])]
            assert not differ, f"{row}: adam {kind} differs from adam_step in {differ}"
        assert R.same_bits(out["ema"]["ema"], out["ema_dev"]["ema"]), row
        ref, yard = R.adam_model(c, sc, F64), R.adam_model(c, sc, F32)
        for q in ("m", "v"):
            _hold(f"adam {q}", row, out["step"][q], ref[q], yard[q], 1e-6)
        _hold("adam ema", row, out["ema"]["ema"], ref["ema"], yard["ema"], 1e-6)
        _hold_p(row, out["step"]["p"], ref, yard)
        z0, z1 = R.adam_zero_block(n)
        if sc["weight_decay"] == 0.0 and z1 > z0:
            assert R.same_bits(out["step"]["p"][z0:z1], c["p"][z0:z1]), f"{row}: p moved where g = m = v = 0"
            assert float(out["step"]["m"][z0:z1].abs().max()) == 0.0 and float(out["step"]["v"][z0:z1].abs().max()) == 0.0


@pytest.mark.parametrize("table", list(R.ADAM_MULTI))
def test_adam_multi_equals_adam_step_tensor_by_tensor(table):
    from stain2stain_amd import ops
    sc = R.ADAM_SCALARS["step2-wd-gs"]
    cases = [R.adam_case(n, "positive", salt=i) for i, n in enumerate(R.ADAM_MULTI[table])]
    tensors, bufs = [], []
    for c in cases:
        vb = [_guarded(c[k]) for k in ("p", "g", "m", "v")]
        tensors.append(tuple(v for v, _ in vb))
        bufs += [b for _, b in vb]
    _adam_multi(ops, tensors, sc)
    assert _intact(*bufs)
    for i, (c, (p, g, m, v)) in enumerate(zip(cases, tensors)):
        want = _adam_run(ops, "step", c, sc)
        differ = [q for q, t in (("p", p), ("m", m), ("v", v)) if not R.same_bits(t, want[q])]
        assert not differ, f"{table}: tensor {i} (n = {p.numel()}) differs from adam_step in {differ}"
        assert R.same_bits(g, c["g"])


# ---------------------------------------------------------------------------------------------------------------------
# weight packing
# ---------------------------------------------------------------------------------------------------------------------
def _pack_outputs(cout, cin, dtype, want_d=True):
    nf, nd = R.pack_elems(cout, cin)
    wf, bf_ = _nan_guarded((nf,), dtype)
    wd, bd = _nan_guarded((nd,), dtype) if want_d else (None, None)
    return wf, wd, [b for b in (bf_, bd) if b is not None]


def _pack_single(ops, shape, dtype, want_d=True):
    w = R.pack_case(*shape).to(DEV)
    wf, wd, bufs = _pack_outputs(*shape, dtype, want_d)
    ops.pack_conv3x3(w, dtype, want_d, out=(wf, wd))
    torch.cuda.synchronize()
    assert _intact(*bufs) and R.same_bits(w, R.pack_case(*shape))
    return wf, wd


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("want_d", R.PACK_WANT_DGRAD, ids=["dgrad", "fwd-only"])
@pytest.mark.parametrize("shape", R.PACK, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_conv3x3_form(shape, want_d, dtype):
    from stain2stain_amd import ops
    wf, wd = _pack_single(ops, shape, dtype, want_d)
    rf, rd = R.pack_ref(R.pack_case(*shape), dtype)
    assert _same_stored(wf, rf, dtype), "Wf differs from the permutation of the rounded weights"
    assert wd is None or _same_stored(wd, rd, dtype), "Wd differs from the flipped, transposed permutation"


def _pack_batched(ops, order, dtype, null_wd=(), misaligned=False):
    rows, outs, bufs, keep, start = [], [], [], [], 0
    for pos, li in enumerate(order):
        cout, cin = R.PACK[li]
        w0 = R.pack_case(cout, cin)
        if misaligned:
            wb = torch.full((w0.numel() + 8,), NAN, device=DEV)
            w = wb[1:1 + w0.numel()]
            w.copy_(w0.reshape(-1).to(DEV))
            assert w.data_ptr() % 16 == 4
        else:
            w = w0.to(DEV)
            assert w.data_ptr() % 16 == 0
        keep.append(w)
        wf, wd, b = _pack_outputs(cout, cin, dtype, pos not in null_wd)
        outs.append((li, wf, wd))
        bufs += b
        rows.append([w.data_ptr(), wf.data_ptr(), 0 if wd is None else wd.data_ptr(), cout, cin, start])
        start += R.pack_form(cout, cin)["tiles"]
    desc = torch.tensor(rows, dtype=torch.int64).to(DEV)
    ops.pack_conv3x3_batched(desc, start, dtype)
    torch.cuda.synchronize()
    assert _intact(*bufs)
    return outs


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("variant", ["order0", "order1", "null-wd", "misaligned"])
def test_pack_conv3x3_batched_form(variant, dtype):
    from stain2stain_amd import ops
    order = R.PACK_ORDERS[1 if variant == "order1" else 0]
    outs = _pack_batched(ops, order, dtype, null_wd=(R.PACK_NULL_WD,) if variant == "null-wd" else (),
                         misaligned=variant == "misaligned")
    for pos, (li, wf, wd) in enumerate(outs):
        shape = R.PACK[li]
        sf, sd = _pack_single(ops, shape, dtype)
        rf, rd = R.pack_ref(R.pack_case(*shape), dtype)
        assert _same_stored(wf, rf, dtype) and _same_stored(wf, sf.float(), dtype), f"{variant}: Wf of layer {shape}"
        if variant == "null-wd" and pos == R.PACK_NULL_WD:
            assert wd is None
        else:
            assert _same_stored(wd, rd, dtype) and _same_stored(wd, sd.float(), dtype), f"{variant}: Wd of layer {shape}"


# ---------------------------------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------------------------------
def _shape_id(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", R.LAYOUT, ids=_shape_id)
def test_nchw_to_nhwc_form(shape, dtype):
    from stain2stain_amd import ops
    B, C, H, W = shape
    c = R.layout_case(shape)
    x = c["x"].to(DEV)
    ref = R.nchw_to_nhwc_ref(c["x"], dtype)
    for sl in R.LAYOUT_SLICES:
        if sl is None:
            wide, out = None, torch.full((B, H, W, C), NAN, dtype=dtype, device=DEV)
        else:
            wide = torch.full((B, H, W, sl[0] + C + sl[1]), NAN, dtype=dtype, device=DEV)
            out = wide[..., sl[0]:sl[0] + C]
        ops.nchw_to_nhwc(x, dtype, out=out)
        torch.cuda.synchronize()
        assert _same_stored(out, ref, dtype), f"{sl}: not the permutation of the rounded values"
        assert wide is None or _guards_intact(wide, sl[0], C), f"{sl}: the slice's surroundings were written"
        del wide, out
    assert R.same_bits(x[:, :, :, : min(W, 64)], c["x"][:, :, :, : min(W, 64)])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", R.LAYOUT, ids=_shape_id)
def test_nhwc_to_nchw_form(shape, dtype):
    from stain2stain_amd import ops
    B, C, H, W = shape
    c = R.layout_case(shape)
    stored = R.nchw_to_nhwc_ref(c["x"], dtype)                   # NHWC, T-rounded values in fp32
    back = R.nhwc_to_nchw_ref(stored)
    xd = stored.to(DEV, dtype)
    for acc in R.LAYOUT_ACCUMULATE:
        want = (c["base"] + back) if acc else back               # torch's single fp32 add
        for sl in R.LAYOUT_SLICES:
            x, wide = (xd, None) if sl is None else _slice_of_wide(xd, *sl)
            out, ob = _guarded(c["base"]) if acc else _nan_guarded(shape)
            ops.nhwc_to_nchw(x, out=out, accumulate=acc)
            torch.cuda.synchronize()
            assert bool(torch.equal(out.view(torch.int32), want.to(DEV).view(torch.int32))), f"acc {acc} {sl}"
            assert _intact(ob) and (wide is None or _guards_intact(wide, sl[0], C))
            del wide, x, out, ob


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_layout_refused_shapes_raise_and_write_nothing(dtype):
    from stain2stain_amd import ops
    for _what, (B, C, H, W), ld in R.LAYOUT_REFUSED:
        wide = torch.full((B, H, W, ld), NAN, dtype=dtype, device=DEV)
        nchw = torch.full((B, C, H, W), NAN, device=DEV)
        with pytest.raises(RuntimeError):
            ops.nchw_to_nhwc(torch.ones(B, C, H, W, device=DEV), dtype, out=wide[..., :C])
        with pytest.raises(RuntimeError):
            ops.nhwc_to_nchw(torch.ones(B, H, W, ld, dtype=dtype, device=DEV)[..., :C], out=nchw)
        torch.cuda.synchronize()
        assert bool(torch.isnan(wide).all()) and bool(torch.isnan(nchw).all())


# ---------------------------------------------------------------------------------------------------------------------
# pixel sum
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", R.PIXSUM_C)
@pytest.mark.parametrize("HW", R.PIXSUM_HW)
def test_pixel_sum_form(HW, C, dtype):
    from stain2stain_amd import _native, ops
    L = ops._L()
    for B in R.PIXSUM_B:
        for tier in TIERS:
            c = R.pixsum_case(B, HW, C, tier)
            xd = c["x"].to(DEV, dtype)
            for acc in R.PIXSUM_ACCUMULATE:
                base = c["base"] if acc else None
                first = None
                for layout, x, wide in _layouts(xd):
                    assert layout in R.PIXSUM_LAYOUTS
                    out, ob = _guarded(c["base"]) if acc else _nan_guarded((B, C))
                    px, ldx = ops._nhwc(x)
                    _native.check(L.s2s_pixel_sum(_code(dtype), px, ldx, out.data_ptr(), B, HW, C, int(acc), ops._stream()),
                                  "pixel_sum")
                    torch.cuda.synchronize()
                    assert _intact(ob) and (wide is None or _guards_intact(wide, 8, C))
                    first = out if first is None else first
                    assert R.same_bits(out, first), f"{layout}: differs from the dense launch"
                row = f"B{B} HW{HW} C{C} acc{int(acc)}"
                ref = R.pixel_sum_ref(c["x"], base, F64)
                if tier == "exact":
                    assert R.same_bits(first, ref.float()), f"{row}: not the exact sum"
                else:
                    _hold(f"pixsum {_dn(dtype)}", row, first, ref, R.pixel_sum_ref(c["x"], base, F32), 1e-4)
    if HW == R.PIXSUM_HW[0] and C == R.PIXSUM_C[0]:
        x = torch.ones(1, 1, 4, 8, dtype=dtype, device=DEV)
        assert R.same_bits(ops.pixel_sum(x), torch.full((1, 8), 4.0))            # the wrapper: accumulate off


# ---------------------------------------------------------------------------------------------------------------------
# time path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", R.TIME_B)
@pytest.mark.parametrize("dim", R.TIME_DIMS)
def test_time_embedding_form(dim, B):
    from stain2stain_amd import ops
    t = R.time_case(B)
    td, tb = _guarded(t)
    out = ops.time_embedding(td, dim)
    torch.cuda.synchronize()
    assert out.shape == (B, dim) and _intact(tb) and R.same_bits(td, t)
    _hold("temb", f"dim{dim} B{B}", out, R.time_embedding_ref(t, dim, F64), R.time_embedding_ref(t, dim, F32), 1e-6)
    o = out.cpu()
    assert float(o[0, : dim // 2].abs().max()) == 0.0 and bool((o[0, dim // 2:] == 1.0).all())      # t = 0 exactly


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("shape", R.LINEAR, ids=_shape_id)
def test_linear_form(shape, tier):
    from stain2stain_amd import ops
    B, Kd, N = shape
    c = R.linear_case(B, Kd, N, tier)
    x, w, b, dy = (c[k].to(DEV) for k in ("x", "w", "b", "dy"))
    row = f"{B}x{Kd}x{N}"
    for bias in R.LINEAR_BIAS:
        y = ops.linear_fwd(x, w, b if bias else None)
        torch.cuda.synchronize()
        ref = R.linear_fwd_ref(c["x"], c["w"], c["b"] if bias else None, F64)
        if tier == "exact":
            _equal_values(f"{row} y bias {bias}", y, ref)
        else:
            _hold("lin y", f"{row} bias{int(bias)}", y, ref, R.linear_fwd_ref(c["x"], c["w"], c["b"] if bias else None, F32), 1e-6)
    ref, yard = R.linear_bwd_ref(c["dy"], c["x"], c["w"], F64), R.linear_bwd_ref(c["dy"], c["x"], c["w"], F32)
    for want_db, need_dx, acc in R.LINEAR_BWD_OPTS:
        dw, dwb = _guarded(c["dw0"]) if acc else _nan_guarded((N, Kd))
        db, dbb = (_guarded(c["db0"]) if acc else _nan_guarded((N,))) if want_db else (None, None)
        dx = ops.linear_bwd(dy, x, w, dw, db, need_dx=need_dx, accumulate=acc)
        torch.cuda.synchronize()
        assert (dx is not None) == need_dx and _intact(dwb) and (dbb is None or _intact(dbb))
        opt = f"{row} db{int(want_db)} dx{int(need_dx)} acc{int(acc)}"
        got = dict(dx=dx, dw=dw, db=db)
        for q in ("dx", "dw", "db"):
            if got[q] is None:
                continue
            base = c[q + "0"] if acc and q != "dx" else None
            r = ref[q] if base is None else ref[q] + base.double()
            if tier == "exact":
                _equal_values(f"{opt} {q}", got[q], r)
            else:
                _hold(f"lin {q}", opt, got[q], r, yard[q] if base is None else yard[q] + base, 1e-5)
    for t, k in ((x, "x"), (w, "w"), (dy, "dy")):
        assert R.same_bits(t, c[k])


@pytest.mark.parametrize("n", R.SILU_N)
def test_silu_form(n):
    from stain2stain_amd import ops
    c = R.silu_case(n)
    h, da = c["h"].to(DEV), c["da"].to(DEV)
    a, dh = ops.silu_fwd(h), ops.silu_bwd(h, da)
    torch.cuda.synchronize()
    a, dh = a.cpu(), dh.cpu()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(dh).all()), "NaN or inf where expf overflows"
    ra, rd = R.silu_fwd_ref(c["h"], F64), R.silu_bwd_ref(c["h"], c["da"], F64)
    k = c["specials"]
    # the specials element by element (|h| up to 104 would hide everything else in a norm)
    for got, ref in ((a[:k], ra[:k]), (dh[:k], rd[:k])):
        assert bool(((got.double() - ref).abs() <= 1e-6 * ref.abs() + R.SILU_UNDERFLOW).all()), (got, ref)
    if n > k:
        _hold("silu a", f"n{n}", a[k:], ra[k:], R.silu_fwd_ref(c["h"], F32)[k:], 1e-6)
        _hold("silu dh", f"n{n}", dh[k:], rd[k:], R.silu_bwd_ref(c["h"], c["da"], F32)[k:], 1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# probability path and loss
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(R.CFM_CASES))
@pytest.mark.parametrize("shape", R.CFM, ids=_shape_id)
def test_cfm_sample_form(shape, case):
    from stain2stain_amd import ops
    B, ps = shape
    sigma, eps_kind = R.CFM_CASES[case]
    c = R.cfm_case(B, ps)
    x0, x1 = c["x0"].to(DEV), c["x1"].to(DEV)
    eps = None if eps_kind is None else torch.full((B, ps), NAN, device=DEV) if eps_kind == "nan" else c["eps"].to(DEV)
    for tv in R.cfm_times(B):
        t = torch.tensor(tv, dtype=F32)
        xt, ut = ops.cfm_sample(x0, x1, t.to(DEV), sigma, eps)
        torch.cuda.synchronize()
        assert R.same_bits(ut, c["x1"] - c["x0"]), "ut is not torch's fp32 x1 - x0"
        rx, _ = R.cfm_ref(c["x0"], c["x1"], t, c["eps"], sigma, F64)
        yx, _ = R.cfm_ref(c["x0"], c["x1"], t, c["eps"], sigma, F32)
        _hold("cfm xt", f"{B}x{ps} {case} t{tv[0]:g}", xt, rx, yx, 1e-6)
        if sigma == 0.0:
            for i, ti in enumerate(tv):
                if ti == 0.0:
                    assert R.same_bits(xt[i], c["x0"][i]), "t = 0 does not return x0"
                if ti == 1.0:
                    assert R.same_bits(xt[i], c["x1"][i]), "t = 1 does not return x1"
    assert R.same_bits(x0, c["x0"]) and R.same_bits(x1, c["x1"])


def test_cfm_refused_launches_raise_and_write_nothing():
    from stain2stain_amd import _native, ops
    L = ops._L()
    for _what, (B, ps), off in R.CFM_REFUSED:
        n = B * ps
        src = torch.ones(2 * n + 8, device=DEV)
        x0, x1 = src[off:off + n], src[n + 4:2 * n + 4]
        xt, ut = torch.full((n,), NAN, device=DEV), torch.full((n,), NAN, device=DEV)
        t = torch.zeros(B, device=DEV)
        with pytest.raises(RuntimeError):
            _native.check(L.s2s_cfm_sample(x0.data_ptr(), x1.data_ptr(), t.data_ptr(), None, 0.0, xt.data_ptr(), ut.data_ptr(),
                                           B, ps, ops._stream()), "cfm_sample")
        with pytest.raises(RuntimeError):
            ops.cfm_sample(x0.view(B, ps), x1.view(B, ps), t)
        torch.cuda.synchronize()
        assert bool(torch.isnan(xt).all()) and bool(torch.isnan(ut).all())


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("count", R.MSE_COUNTS)
def test_mse_loss_form(count, tier):
    from stain2stain_amd import ops
    c = R.mse_case(count, tier)
    v, u = c["v"].to(DEV), c["u"].to(DEV)
    for gs in R.MSE_GRAD_SCALES:
        ref, yard = R.mse_ref(c["v"], c["u"], gs, F64), R.mse_ref(c["v"], c["u"], gs, F32)
        losses = []
        for want_dv in R.MSE_WANT_DV:
            loss, dv = ops.mse_loss(v, u, want_grad=want_dv, grad_scale=gs)
            torch.cuda.synchronize()
            assert (dv is not None) == want_dv
            losses.append(loss)
            got, want = float(loss), float(ref["loss"])
            tol = float(R.ulp(ref["loss"], F32)) if tier == "exact" else 1e-6 * abs(want)
            print(f"mse count {count} {tier} gs {gs}: loss {got!r} float64 {want!r} off {abs(got - want):.3e} bound {tol:.3e}")
            assert abs(got - want) <= tol
            if dv is None:
                continue
            if tier == "exact":
                # one fp32 multiply of an integer by the fp32 coef: the correctly rounded product, whatever the count
                assert R.same_bits(dv, ref["dv"].float()), "dv is not the rounded product"
            else:
                _hold("mse dv", f"count{count} gs{gs}", dv, ref["dv"], yard["dv"], 1e-6)
        assert R.same_bits(losses[0], losses[1]), "the loss depends on whether dv is written"
    assert R.same_bits(v, c["v"]) and R.same_bits(u, c["u"])


# ---------------------------------------------------------------------------------------------------------------------
# sampler glue
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tols", R.ERR_TOLS, ids=lambda t: f"atol{t[0]:g}-rtol{t[1]:g}")
@pytest.mark.parametrize("n", R.ERR_N)
def test_ode_error_norm_form(n, tols):
    from stain2stain_amd import ops
    atol, rtol = tols
    c = R.err_case(n)
    e, y0, y1 = (c[k].to(DEV) for k in ("e", "y0", "y1"))
    out = ops.ode_error_norm(e, y0, y1, atol, rtol)
    torch.cuda.synchronize()
    _hold("err norm", f"n{n} atol{atol:g} rtol{rtol:g}", out, R.err_norm_ref(c["e"], c["y0"], c["y1"], atol, rtol, F64),
          R.err_norm_ref(c["e"], c["y0"], c["y1"], atol, rtol, F32), 1e-6)
    assert R.same_bits(e, c["e"]) and R.same_bits(y0, c["y0"]) and R.same_bits(y1, c["y1"])


@pytest.mark.parametrize("a", R.AXPY_A, ids=lambda a: f"a{a:.3g}")
@pytest.mark.parametrize("n", R.AXPY_N)
def test_axpy_form(n, a):
    from stain2stain_amd import ops
    c = R.axpy_case(n)
    x, xb = _guarded(c["x"])
    y, yb = _guarded(c["y"])
    ops.axpy_(x, y, a)
    torch.cuda.synchronize()
    assert _intact(xb, yb) and R.same_bits(y, c["y"])
    assert R.within_ulps(x, R.axpy_ref(c["x"], c["y"], a), 1.0), "x + a y is more than one fp32 ulp from float64"
    if a == 1.0:
        assert R.same_bits(x, c["x"] + c["y"])
    if a == 0.0:
        assert R.same_bits(x, c["x"])
    # both operands the same buffer (pix2pix_engine's axpy_(losses, losses, a)): x (1 + a)
    z, zb = _guarded(c["x"])
    ops.axpy_(z, z, a)
    torch.cuda.synchronize()
    assert _intact(zb)
    assert R.within_ulps(z, c["x"].double() * (1.0 + R.f32(a)), 1.0), "the aliased call is not x (1 + a)"


@pytest.mark.parametrize("n", R.TICK_N)
def test_euler_tick_form(n):
    from stain2stain_amd import ops
    table, tb = _guarded(torch.tensor(R.TICK_TABLE, dtype=F32))
    cb = torch.full((2 * G + 1,), -77, dtype=torch.int32, device=DEV)
    counter = cb[G:G + 1]
    counter.zero_()
    for k, want in enumerate(R.TICK_TABLE):
        t, tbuf = _nan_guarded((n,))
        ops.euler_tick_(t, table, counter)
        torch.cuda.synchronize()
        assert R.same_bits(t, torch.full((n,), want)), f"call {k}"
        assert int(counter) == k + 1 and _intact(tbuf, tb)
        assert bool((cb[:G] == -77).all()) and bool((cb[G + 1:] == -77).all())
    assert R.same_bits(table, torch.tensor(R.TICK_TABLE, dtype=F32))


@pytest.mark.parametrize("n", R.FILL_N)
def test_fill_form(n):
    from stain2stain_amd import ops
    for v in (0.0, -2.5):
        x, xb = _nan_guarded((n,))
        ops.fill_(x, v)
        torch.cuda.synchronize()
        assert _intact(xb) and bool((x == v).all())
