"""Every form of the segmentation and ROI loss kernels against float64, row by row of
tests/loss_forms_ref.py: s2s_seg_loss, s2s_seg_loss_multiclass (C = 2 ... 8), s2s_seg_eval_binary,
s2s_seg_eval_multiclass, s2s_weighted_mse, s2s_charbonnier_roi, s2s_class_embed_add, s2s_class_embed_bwd.

Every row calls the C ABI directly: ``out``, ``dz`` / ``dv`` / ``dtable``, ``counts`` and ``work`` are each the middle of
a buffer with sentinel guards on either side, ``work`` of exactly the size include/stain2stain_hip.h states, the outputs
NaN (counts -1) before the launch.  Afterwards the guards are intact, every output element is written and finite (but for
the row whose every target is ignored: ce and seg NaN, dice 0, dz exactly zero), and the operands keep their bits.  Every
entry point runs twice on fresh buffers and gives the same bits, dz included; the ops wrappers return the bits of the
direct call on one small and one striding row each.

Exact claims: the counts at every row, the striding ones included (on the knife-edge and specials rows each count lies
between the one taken with z >= 1e-6 and the one taken with z > 0); an empty ROI gives exactly 0.0; class_embed_add is
torch's fp32 temb + table[y]; dtable on a NaN-filled buffer is the sequential fp32 sum over the batch from +0, rows of
absent classes +0, and with accumulate = 1 torch's single fp32 add of that onto known values.

Bounded claims: the project's hard bounds against float64 as relative max and relative L2 (values, binary dz and dv 1e-5,
multiclass dz 1e-4; each of seg, dice and bce / ce on its own) and, on top, K x the yardstick: the deviation of torch's
fp32 evaluation of the same quantity on the CPU from float64 (floored at 1e-7).  The specials (z = 0, +-1e-30, +-20, +-88,
+-104 against g = 0 and 1) are held element by element at 1e-6 relative plus loss_forms_ref.BIN_UNDERFLOW.

K = 4 x the largest ratio measured on the MI355X over the table, rounded up to a power of two (the row in brackets):

  binary value      K 4  ratio 0.566  [n1-gs0.25, bce]
  binary dz         K 8  ratio 1.448  [knife-edge]
  multiclass value  K 8  ratio 1.437  [5x1-C2, seg]
  multiclass dz     K 8  ratio 1.734  [ignore-last-C2]
  eval value        K 8  ratio 1.437  [5x1-C2, seg]
  wmse value        K 4  ratio 0.524  [1x1x5x7]
  wmse dv           K 8  ratio 1.209  [3x3x600x583-gs0.25]
  charbonnier       K 4  ratio 0.613  [1x1x5x7]
  dtable            K 4  ratio 1.000  [16x256x3-one]

No quantity asks for more than 16, none for more than 8: the sums are taken in float64, so a value costs the fp32
roundings of its terms and one rounding of the result (the ratios above 1 are errors of 1.4e-7 to 3.3e-7 against
yardsticks of 0.7e-7 to 2.3e-7), and the gradients perform the roundings of an fp32 evaluation."""
import pytest
import torch

import loss_forms_ref as R
from test_wgrad_forms_gpu import _guards_intact, _slice_of_wide, poison  # noqa: F401  (poison: autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64, I64 = R.F32, R.F64, torch.int64
NAN = float("nan")
G = 8                                  # guard elements on either side
SENT = -1216.0

# quantity -> K; the measurements are in the docstring
K = {"binary value": 4, "binary dz": 8, "multiclass value": 8, "multiclass dz": 8, "eval value": 8, "wmse value": 4, "wmse dv": 8,
     "charbonnier": 4, "dtable": 4}
HARD_VALUE, HARD_DZ_BINARY, HARD_DZ_MULTICLASS, HARD_DV, HARD_DTABLE = 1e-5, 1e-5, 1e-4, 1e-5, 1e-5


def _L():
    from stain2stain_amd import _native
    return _native.lib()


def _stream():
    from stain2stain_amd import ops
    return ops._stream()


def _hold(q, row, got, ref, yard, hard):
    """An fp32 output against the float64 model: finite, the hard bound, then K x the yardstick (its deviations)."""
    got = got.detach().cpu().reshape(ref.shape)
    err = R.deviation(got, ref)
    rat = R.ratios(err, yard)
    line = (f"RATIO {q} | {row} | {max(rat):.3f} | max {err[0]:.2e} l2 {err[1]:.2e} yardstick {yard[0]:.2e} {yard[1]:.2e} "
            f"K {K[q]}")
    print(line)
    assert bool(torch.isfinite(got).all()), line
    assert err[0] < hard and err[1] < hard, f"{line}: over the hard bound {hard}"
    assert max(rat) <= K[q], f"{line}: over K x yardstick"


def _hold_values(q, row, got, case):
    """seg, dice and bce / ce (or the one value of a ROI loss) each on its own, so that no term hides behind another."""
    ref = case["ref"]["out"]
    for i in range(ref.numel()):
        _hold(q, f"{row} out[{i}]", got[i:i + 1], ref[i:i + 1], case["yard"]["out-each"][i], HARD_VALUE)


def _guarded(t):
    """A CPU tensor as the middle of a GPU buffer with G sentinel elements on either side: (view, buffer)."""
    n = t.numel()
    buf = torch.full((n + 2 * G,), SENT, dtype=t.dtype, device=DEV)
    buf[G:G + n] = t.reshape(-1).to(DEV)
    return buf[G:G + n].view(t.shape), buf


def _poisoned(shape, dtype=F32):
    """An output as the middle of a guarded buffer: NaN (fp32 / fp64) or -1 (int64) before the launch."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * G,), SENT, dtype=dtype, device=DEV)
    buf[G:G + n] = -1 if dtype == I64 else NAN
    return buf[G:G + n].view(shape), buf


def _intact(*bufs):
    return all(bool((b[:G] == SENT).all()) and bool((b[-G:] == SENT).all()) for b in bufs)


def _written(*outs):
    return all(not bool((o == -1).any()) if o.dtype == I64 else not bool(torch.isnan(o).any()) for o in outs)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == F32 else I64)


def _same(a, b):
    return all(bool(torch.equal(_bits(x), _bits(y))) for x, y in zip(a, b))


def _twice(run):
    """Two launches on fresh buffers: the same bits."""
    first, second = run(), run()
    assert _same(first, second), "two launches differ"
    return first


# ---------------------------------------------------------------------------------------------------------------------
# direct calls
# ---------------------------------------------------------------------------------------------------------------------
def _seg_loss(z, g, smooth, dw, gs, want_dz=True):
    n = z.numel()
    out, ob = _poisoned((3,))
    dz, db = _poisoned((n,)) if want_dz else (None, None)
    work, wb = _poisoned((R.WORK["seg_loss"],), F64)
    rc = _L().s2s_seg_loss(z.data_ptr(), g.data_ptr(), 0 if dz is None else dz.data_ptr(), out.data_ptr(), work.data_ptr(), n,
                           smooth, dw, gs, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and _intact(*[b for b in (ob, db, wb) if b is not None]), "a guard element was written"
    assert _written(out) and (dz is None or _written(dz)), "an output element was not written"
    return (out, dz) if want_dz else (out,)


def _seg_eval_binary(z, g, smooth, dw):
    out, ob = _poisoned((5,))
    counts, cb = _poisoned((4,), I64)
    work, wb = _poisoned((R.WORK["seg_eval_binary"],), F64)
    rc = _L().s2s_seg_eval_binary(z.data_ptr(), g.data_ptr(), out.data_ptr(), counts.data_ptr(), work.data_ptr(), z.numel(), smooth, dw,
                                  _stream())
    torch.cuda.synchronize()
    assert rc == 0 and _intact(ob, cb, wb), "a guard element was written"
    assert _written(out, counts), "an output element was not written"
    return out, counts


def _seg_loss_mc(z, t, ignore, smooth, dw, gs, want_dz=True, nan_row=False):
    B, C, HW = z.shape
    out, ob = _poisoned((3,))
    dz, db = _poisoned((B, C, HW)) if want_dz else (None, None)
    work, wb = _poisoned((R.WORK["seg_loss_multiclass"],), F64)
    rc = _L().s2s_seg_loss_multiclass(z.data_ptr(), t.data_ptr(), 0 if dz is None else dz.data_ptr(), out.data_ptr(), work.data_ptr(),
                                      B, HW, C, ignore, smooth, dw, gs, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and _intact(*[b for b in (ob, db, wb) if b is not None]), "a guard element was written"
    assert (dz is None or _written(dz)) and _written(out[1:2]) and (nan_row or _written(out)), "an output element was not written"
    return (out, dz) if want_dz else (out,)


def _seg_eval_mc(z, t, ignore, smooth, dw, nan_row=False):
    B, C, HW = z.shape
    out, ob = _poisoned((5,))
    counts, cb = _poisoned((32,), I64)
    work, wb = _poisoned((R.WORK["seg_eval_multiclass"],), F64)
    rc = _L().s2s_seg_eval_multiclass(z.data_ptr(), t.data_ptr(), out.data_ptr(), counts.data_ptr(), work.data_ptr(), B, HW, C, ignore,
                                      smooth, dw, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and _intact(ob, cb, wb), "a guard element was written"
    assert _written(counts, out[1:2], out[3:]) and (nan_row or _written(out)), "an output element was not written"
    return out, counts


def _weighted_mse(v, u, m, lam, gs, want_dv=True):
    B, C, HW = v.shape
    out, ob = _poisoned((1,))
    dv, db = _poisoned((B, C, HW)) if want_dv else (None, None)
    work, wb = _poisoned((R.WORK["weighted_mse"],), F64)
    rc = _L().s2s_weighted_mse(v.data_ptr(), u.data_ptr(), m.data_ptr(), 0 if dv is None else dv.data_ptr(), out.data_ptr(),
                               work.data_ptr(), B, C, HW, lam, gs, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and _intact(*[b for b in (ob, db, wb) if b is not None]), "a guard element was written"
    assert _written(out) and (dv is None or _written(dv)), "an output element was not written"
    return (out, dv) if want_dv else (out,)


def _charbonnier(a, b, m, eps_charb, eps_area):
    B, C, HW = a.shape
    out, ob = _poisoned((1,))
    work, wb = _poisoned((R.WORK["charbonnier_roi"],), F64)
    rc = _L().s2s_charbonnier_roi(a.data_ptr(), b.data_ptr(), m.data_ptr(), out.data_ptr(), work.data_ptr(), B, C, HW, eps_charb,
                                  eps_area, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and _intact(ob, wb) and _written(out)
    return (out,)


def _unchanged(pairs):
    return all(R.same_bits(d, h) if h.dtype == F32 else bool(torch.equal(d.cpu(), h)) for d, h in pairs)


# ---------------------------------------------------------------------------------------------------------------------
# binary Dice + BCE
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.BIN_ROWS))
def test_seg_loss_binary_form(name):
    c = R.bin_case(name)
    z, g = c["z"].to(DEV), c["g"].to(DEV)
    out, dz = _twice(lambda: _seg_loss(z, g, c["smooth"], c["dw"], c["gs"]))
    (only,) = _seg_loss(z, g, c["smooth"], c["dw"], c["gs"], want_dz=False)
    assert _same([only], [out]), "the values depend on whether dz is written"
    assert _unchanged([(z, c["z"]), (g, c["g"])])
    out, dz = out.cpu(), dz.cpu()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dz).all())
    ref = c["ref"]
    if c["logits"] == "specials":
        # element by element (|z| up to 104 against z = 0: a norm would hide the saturated elements)
        for what, got, want, floor in (("out", out, ref["out"], 0.0), ("dz", dz, ref["dz"], R.BIN_UNDERFLOW)):
            off = (got.double() - want).abs()
            bound = 1e-6 * want.abs() + floor
            print(f"specials {name} {what}: worst off / bound {float((off / bound).max()):.3f}")
            assert bool((off <= bound).all()), (name, what, got, want)
        return
    _hold_values("binary value", name, out, c)
    _hold("binary dz", name, dz, ref["dz"], c["yard"]["dz"], HARD_DZ_BINARY)


@pytest.mark.parametrize("name", list(R.BIN_ROWS))
def test_seg_eval_binary_form(name):
    c = R.bin_case(name)
    z, g = c["z"].to(DEV), c["g"].to(DEV)
    out, counts = _twice(lambda: _seg_eval_binary(z, g, c["smooth"], c["dw"]))
    assert _unchanged([(z, c["z"]), (g, c["g"])])
    out, counts = out.cpu(), counts.cpu().tolist()
    assert bool(torch.isfinite(out).all())
    lo, hi = c["counts_lo"], c["counts_hi"]
    assert all(a <= k <= b for a, k, b in zip(lo, counts, hi)), (name, lo, counts, hi)       # lo == hi off the knife edge
    I, P, Gc, U = counts
    dc, iou = R.metric_model(I, P + Gc, U)
    assert abs(float(out[3]) - dc) <= 1e-6 * dc and abs(float(out[4]) - iou) <= 1e-6 * iou
    if c["logits"] == "specials":
        assert bool(((out[:3].double() - c["ref"]["out"]).abs() <= 1e-6 * c["ref"]["out"].abs()).all())
        return
    _hold_values("eval value", name, out[:3], c)


# ---------------------------------------------------------------------------------------------------------------------
# multiclass softmax Dice + cross entropy
# ---------------------------------------------------------------------------------------------------------------------
def _mc_values_when_all_ignored(name, out):
    assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[2])) and float(out[1]) == 0.0, (name, out)


@pytest.mark.parametrize("name", list(R.MC_ROWS))
def test_seg_loss_multiclass_form(name):
    c = R.mc_case(name)
    z, t = c["z"].to(DEV), c["t"].to(DEV)
    nan_row = c["all_ignored"]
    args = (c["ignore"], c["smooth"], c["dw"], c["gs"])
    out, dz = _twice(lambda: _seg_loss_mc(z, t, *args, nan_row=nan_row))
    (only,) = _seg_loss_mc(z, t, *args, want_dz=False, nan_row=nan_row)
    assert _same([only], [out]), "the values depend on whether dz is written"
    assert _unchanged([(z, c["z"]), (t, c["t"])])
    out, dz = out.cpu(), dz.cpu()
    assert bool(torch.isfinite(dz).all())
    if nan_row:
        _mc_values_when_all_ignored(name, out)
        assert float(dz.abs().max()) == 0.0, "dz is not exactly zero where every target is ignored"
        return
    _hold_values("multiclass value", name, out, c)
    _hold("multiclass dz", name, dz, c["ref"]["dz"], c["yard"]["dz"], HARD_DZ_MULTICLASS)


@pytest.mark.parametrize("name", list(R.MC_ROWS))
def test_seg_eval_multiclass_form(name):
    c = R.mc_case(name)
    C = c["C"]
    z, t = c["z"].to(DEV), c["t"].to(DEV)
    nan_row = c["all_ignored"]
    out, counts = _twice(lambda: _seg_eval_mc(z, t, c["ignore"], c["smooth"], c["dw"], nan_row=nan_row))
    assert _unchanged([(z, c["z"]), (t, c["t"])])
    out, counts = out.cpu(), counts.cpu().view(4, 8)
    assert bool(torch.equal(counts[:, :C], c["counts"])), (name, counts, c["counts"])
    assert int(counts[:, C:].abs().sum()) == 0
    dc, iou = R.mc_metric_model(c["counts"], c["ignore"])
    assert abs(float(out[3]) - dc) <= 1e-6 * dc and abs(float(out[4]) - iou) <= 1e-6 * iou
    if nan_row:
        _mc_values_when_all_ignored(name, out)
        return
    assert bool(torch.isfinite(out).all())
    _hold_values("eval value", name, out[:3], c)


# ---------------------------------------------------------------------------------------------------------------------
# ROI-weighted MSE and ROI Charbonnier
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.WMSE_ROWS))
def test_weighted_mse_form(name):
    c = R.wmse_case(name)
    v, u, m = c["v"].to(DEV), c["u"].to(DEV), c["m"].to(DEV)
    out, dv = _twice(lambda: _weighted_mse(v, u, m, c["lam"], c["gs"]))
    (only,) = _weighted_mse(v, u, m, c["lam"], c["gs"], want_dv=False)
    assert _same([only], [out]), "the value depends on whether dv is written"
    assert _unchanged([(v, c["v"]), (u, c["u"]), (m, c["m"])])
    out, dv = out.cpu(), dv.cpu()
    _hold_values("wmse value", name, out, c)
    _hold("wmse dv", name, dv, c["ref"]["dv"], c["yard"]["dv"], HARD_DV)
    if c["lam"] == 0.0:                     # the plain MSE s2s_mse_loss is held to
        plain = R.mse_model(c["v"], c["u"], c["gs"])
        for got, want in ((out, plain["out"]), (dv, plain["dv"])):
            err = R.deviation(got.reshape(want.shape), want)
            assert max(err) < HARD_VALUE, (name, err)


@pytest.mark.parametrize("name", list(R.CHARB_ROWS))
def test_charbonnier_form(name):
    c = R.charb_case(name)
    a, b, m = c["a"].to(DEV), c["b"].to(DEV), c["m"].to(DEV)
    (out,) = _twice(lambda: _charbonnier(a, b, m, c["eps_charb"], c["eps_area"]))
    assert _unchanged([(a, c["a"]), (b, c["b"]), (m, c["m"])])
    out = out.cpu()
    if c["mask"] == "empty":
        assert _bits(out).item() == 0, "an empty ROI does not give exactly +0.0"
        return
    _hold_values("charbonnier", name, out, c)


# ---------------------------------------------------------------------------------------------------------------------
# class embedding
# ---------------------------------------------------------------------------------------------------------------------
def _embed_add(temb, table, y):
    out, ob = _poisoned(tuple(temb.shape))
    rc = _L().s2s_class_embed_add(temb.data_ptr(), table.data_ptr(), y.data_ptr(), out.data_ptr(), temb.shape[0], temb.shape[1], _stream())
    torch.cuda.synchronize()
    assert rc == 0 and _intact(ob) and _written(out)
    return (out,)


def _embed_bwd(dout, y, classes, base=None):
    dt, tb = _poisoned((classes, dout.shape[1])) if base is None else _guarded(base)
    rc = _L().s2s_class_embed_bwd(dout.data_ptr(), y.data_ptr(), dt.data_ptr(), int(base is not None), dout.shape[0], dout.shape[1],
                                  classes, _stream())
    torch.cuda.synchronize()
    assert rc == 0 and _intact(tb) and _written(dt)
    return (dt,)


@pytest.mark.parametrize("name", list(R.EMBED_ROWS))
def test_class_embed_form(name):
    c = R.embed_case(name)
    k = c["classes"]
    temb, table, dout, y = c["temb"].to(DEV), c["table"].to(DEV), c["dout"].to(DEV), c["y"].to(DEV)
    (out,) = _twice(lambda: _embed_add(temb, table, y))
    assert R.same_bits(out, c["temb"] + c["table"][c["y"]]), "out is not torch's fp32 temb + table[y]"
    (dt,) = _twice(lambda: _embed_bwd(dout, y, k))
    assert R.same_bits(dt, c["seq"]), "dtable is not the sequential fp32 sum over the batch from +0"
    absent = ~c["present"]
    assert bool((_bits(dt)[absent] == 0).all()), "the row of an absent class is not +0"
    (acc,) = _twice(lambda: _embed_bwd(dout, y, k, base=c["base"]))
    assert R.same_bits(acc, c["base"] + c["seq"]), "accumulate = 1 is not torch's single fp32 add onto the buffer"
    assert _unchanged([(temb, c["temb"]), (table, c["table"]), (dout, c["dout"]), (y, c["y"])])
    _hold("dtable", name, dt, c["ref"]["dtable"], c["yard"]["dtable"], HARD_DTABLE)


# ---------------------------------------------------------------------------------------------------------------------
# the wrappers return the bits of the direct call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.BIN_OPS_ROWS)
def test_ops_binary_wrappers_return_the_direct_bits(name):
    from stain2stain_amd import ops
    c = R.bin_case(name)
    z, g = c["z"].to(DEV), c["g"].to(DEV)
    direct = _seg_loss(z, g, c["smooth"], c["dw"], c["gs"])
    assert _same(ops.seg_loss(z, g, c["smooth"], c["dw"], True, c["gs"]), direct)
    out, none = ops.seg_loss(z.view(1, 1, 1, -1), g.view(1, 1, -1), c["smooth"], c["dw"], False, c["gs"])      # [B,H,W] mask
    assert none is None and _same([out], direct[:1])
    ev = _seg_eval_binary(z, g, c["smooth"], c["dw"])
    assert _same(ops.seg_eval_binary(z.view(1, 1, 1, -1), g.view(1, 1, 1, -1), c["smooth"], c["dw"]), ev)


@pytest.mark.parametrize("name", R.MC_OPS_ROWS)
def test_ops_multiclass_wrappers_return_the_direct_bits(name):
    from stain2stain_amd import ops
    c = R.mc_case(name)
    B, C, HW = c["z"].shape
    z, t = c["z"].to(DEV), c["t"].to(DEV)
    direct = _seg_loss_mc(z, t, c["ignore"], c["smooth"], c["dw"], c["gs"])
    for validate in (True, False):
        out, dz = ops.seg_loss_multiclass(z.view(B, C, 1, HW), t.view(B, 1, HW), c["ignore"], c["smooth"], c["dw"], True, c["gs"],
                                          validate=validate)
        assert _same([out, dz.view(B, C, HW)], direct)
    ev = _seg_eval_mc(z, t, c["ignore"], c["smooth"], c["dw"])
    out, counts = ops.seg_eval_multiclass(z.view(B, C, 1, HW), t.view(B, 1, HW), c["ignore"], c["smooth"], c["dw"])
    assert _same([out], ev[:1]) and bool(torch.equal(counts.cpu(), ev[1].cpu().view(4, 8)[:, :C]))


@pytest.mark.parametrize("name", R.WMSE_OPS_ROWS)
def test_ops_weighted_mse_returns_the_direct_bits(name):
    from stain2stain_amd import ops
    c = R.wmse_case(name)
    B, C, H, W = c["shape"]
    v, u, m = c["v"].to(DEV), c["u"].to(DEV), c["m"].to(DEV)
    direct = _weighted_mse(v, u, m, c["lam"], c["gs"])
    out, dv = ops.weighted_mse(v.view(B, C, H, W), u.view(B, C, H, W), m.view(B, 1, H, W), c["lam"], True, c["gs"])
    assert _same([out, dv.view(B, C, -1)], direct)


@pytest.mark.parametrize("name", R.CHARB_OPS_ROWS)
def test_ops_charbonnier_returns_the_direct_bits(name):
    from stain2stain_amd import ops
    c = R.charb_case(name)
    B, C, H, W = c["shape"]
    a, b, m = c["a"].to(DEV), c["b"].to(DEV), c["m"].to(DEV)
    direct = _charbonnier(a, b, m, c["eps_charb"], c["eps_area"])
    assert _same([ops.charbonnier_roi(a.view(B, C, H, W), b.view(B, C, H, W), m.view(B, H, W), c["eps_charb"], c["eps_area"])], direct)


@pytest.mark.parametrize("name", R.EMBED_OPS_ROWS)
def test_ops_class_embed_returns_the_direct_bits(name):
    from stain2stain_amd import ops
    c = R.embed_case(name)
    temb, table, dout, y = c["temb"].to(DEV), c["table"].to(DEV), c["dout"].to(DEV), c["y"].to(DEV)
    assert _same([ops.class_embed_add(temb, table, y)], _embed_add(temb, table, y))
    assert _same([ops.class_embed_bwd(dout, y, c["classes"])], _embed_bwd(dout, y, c["classes"]))
