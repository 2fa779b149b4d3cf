"""tests/head_tail_forms_ref.py is right, and its tables reach what they were written for (host code only: no GPU).

  * every row's family is what s2s_head_loss_family / s2s_tail_family / s2s_head_mse_family answer, and its walk label is
    what the library's block counts (s2s_head_loss_blocks, s2s_tail_blocks, s2s_bn_bwd_blocks, s2s_head_mse_eval_blocks)
    give for its pixel count;
  * the tables hold every form by enumeration: deleting a row fails here;
  * every (C, Cout) that ops.tail_fusable accepts has a head_loss_fused kernel (the regression test of the host gate that
    kept head_loss_lanes_kernel<T, 16 | 32 | 64> unreachable);
  * refused shapes answer the entry points' status;
  * the float64 models agree with torch autograd to 1e-12: the loss, the head, and BatchNorm + ReLU + head + MSE through
    torch.nn.functional;
  * the exact tier's preconditions hold for every row."""
import pytest
import torch
import torch.nn.functional as F

import head_tail_forms_ref as R

BF, F32, F64 = R.BF, R.F32, R.F64
TOL = 1e-12
DTYPES = (BF, F32)


def _lib():
    from stain2stain_amd import _native
    return _native.lib()


def _loss_walk(shape, lanes):
    B, H, W, _ = shape
    nb = _lib().s2s_head_loss_blocks(B, H, W)
    assert nb == _lib().s2s_tail_blocks(B, H, W) > 0
    return R.walk_label(B * H * W, 256 // (1 if lanes == R.PIXEL else lanes), nb, R.LOSS_BLOCK_CAP), nb


# ---------------------------------------------------------------------------------------------------------------------
# tables against the queries
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.HEAD))
def test_head_rows_reach_their_form(name):
    from stain2stain_amd import ops
    (B, H, W, C), opt, fam = R.HEAD[name]
    for dt in DTYPES:
        assert ops.head_loss_family(dt, B, H, W, C, opt[0]) == fam
    assert _loss_walk((B, H, W, C), fam)[0] == opt[5]


@pytest.mark.parametrize("name", list(R.TAIL))
def test_tail_rows_reach_their_form(name):
    from stain2stain_amd import ops
    (B, H, W, C), opt, fam = R.TAIL[name]
    for dt in DTYPES:
        assert ops.tail_family(dt, B, H, W, C, opt[0]) == fam
        assert ops.head_loss_family(dt, B, H, W, C, opt[0]) == fam[0]      # the chain the tail is held equal to
    assert _loss_walk((B, H, W, C), fam[0])[0] == opt[5]
    assert ops.tail_fusable(C, opt[0])
    assert _lib().s2s_bn_bwd_blocks(B, H, W, C) >= 1


@pytest.mark.parametrize("name", list(R.EVAL))
def test_eval_rows_reach_their_form(name):
    from stain2stain_amd import ops
    (B, H, W, C), (cout, _bias), fam = R.EVAL[name]
    for dt in DTYPES:
        assert ops.head_mse_family(dt, B, H, W, C, cout) == fam
    nb = _lib().s2s_head_mse_eval_blocks(B, H, W, C)
    per = 256 // fam[0] * R.MSE_UNROLL
    assert nb == min(-(-B * H * W // per), R.MSE_BLOCK_CAP)


def _labels(table, lanes, fam_of=lambda f: f):
    return [o[5] for (_s, o, f) in table.values() if fam_of(f) == lanes]


@pytest.mark.parametrize("table", ["HEAD", "TAIL"])
def test_lane_tables_hold_every_form(table):
    rows = getattr(R, table)
    fam_of = (lambda f: f) if table == "HEAD" else (lambda f: f[0])
    for lanes in (1, 2, 4, 8, 16, 32, 64):
        mine = [(s, o) for (s, o, f) in rows.values() if fam_of(f) == lanes]
        assert all(s[3] == 8 * lanes for s, _ in mine)
        labels = [o[5] for _, o in mine]
        assert "fewer" in labels and "one" in labels, (lanes, labels)
        rounds = [int(p) for lab in labels for p in lab.split("-") if p.isdigit()]
        assert any(r >= 3 and r % 2 for r in rounds) and any(r >= 3 and r % 2 == 0 for r in rounds), (lanes, labels)
        assert any(lab.endswith("ragged") for lab in labels) and any(lab.endswith("last1") for lab in labels), (lanes, labels)
        assert any(lab.startswith(("blocks", "cap")) for lab in labels), (lanes, labels)
        # a workgroup round that straddles two samples
        assert any(s[0] > 1 and (s[1] * s[2]) % (256 // lanes) for s, _ in mine), lanes
        assert {o[0] for _, o in mine} == {1, 2, 3, 4}, lanes                 # the owner-lane map of every output count
        for pick, vals in ((1, {True, False}), (2, {True, False}), (3, {True, False}), (4, {1.0, 0.25})):
            assert {o[pick] for _, o in mine} == vals, (lanes, pick)
    # the block cap with one lane per pixel: the smallest count with a second grid-stride round
    capped = [s for (s, o, f) in rows.values() if fam_of(f) == 1 and o[5] == "cap-2-last1"]
    assert capped and all(s[0] * s[1] * s[2] == 256 * R.LOSS_BLOCK_CAP + 1 and s[3] == 8 for s in capped)
    assert any(s[:3] == (37, 1, 1) for (s, _o, _f) in rows.values())
    if table == "HEAD":
        pixel = {s[3] // 8 for (s, _o, f) in rows.values() if f == R.PIXEL}
        assert pixel == {3, 5, 9, 12}
        assert _lib().s2s_head_loss_family(0, 1, 4, 4, 104, 3) == R.ERR_SHAPE       # 96 is the last width of that kernel
    else:
        assert {f for (_s, _o, f) in rows.values()} == {(p, m) for p in (1, 2, 4, 8, 16, 32, 64) for m in (3, 4)}
        assert any(s[3] == R.TAIL_TWO_GROUPS for (s, _o, _f) in rows.values())


def test_eval_table_holds_every_form():
    fams = {f for (_s, _o, f) in R.EVAL.values()}
    assert fams == {(gl, mo) for gl in (1, 2, 4, 8) for mo in (3, 4, 8)}
    assert {o[0] for (_s, o, _f) in R.EVAL.values()} == {1, 2, 3, 4, 5, 6, 7, 8}
    cs = {s[3] for (s, _o, _f) in R.EVAL.values()}
    assert {24, 40, 72, R.EVAL_MAX_C} <= cs
    assert _lib().s2s_head_mse_family(0, 1, 4, 4, R.EVAL_MAX_C + 8, 3) == R.ERR_SHAPE
    for gl in (1, 2, 4, 8):
        per = 256 // gl * R.MSE_UNROLL
        npix = {s[0] * s[1] * s[2] for (s, _o, f) in R.EVAL.values() if f[0] == gl}
        assert {per - 1, per, per + 1} <= npix, (gl, npix)
    (B, H, W, C), _o, fam = R.EVAL[R.EVAL_CAPPED]
    per = 256 // fam[0] * R.MSE_UNROLL
    assert B * H * W == per * R.MSE_BLOCK_CAP + 1 and _lib().s2s_head_mse_eval_blocks(B, H, W, C) == R.MSE_BLOCK_CAP
    assert any(s[:3] == (37, 1, 1) for (s, _o, _f) in R.EVAL.values())
    assert {o[1] for (_s, o, _f) in R.EVAL.values()} == {True, False}


# ---------------------------------------------------------------------------------------------------------------------
# the host gate, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_whatever_the_tail_takes_the_head_loss_takes():
    from stain2stain_amd import ops
    seen = 0
    for C in range(8, 1032, 8):
        for cout in range(1, 6):
            if not ops.tail_fusable(C, cout):
                continue
            seen += 1
            for dt in DTYPES:
                assert ops.head_loss_family(dt, 2, 16, 16, C, cout) == C // 8, (C, cout)
                assert ops.tail_family(dt, 2, 16, 16, C, cout) == (C // 8, 3 if cout <= 3 else 4), (C, cout)
    assert seen == 7 * 4


def test_refused_shapes_answer_the_entry_points_status():
    L = _lib()
    query = {"head": L.s2s_head_loss_family, "tail": L.s2s_tail_family, "eval": L.s2s_head_mse_family}
    for entry, (B, H, W, C, cout) in R.REFUSED:
        for dt in (0, 1):
            assert query[entry](dt, B, H, W, C, cout) == R.ERR_SHAPE, (entry, C, cout)
    for q in query.values():
        assert q(7, 1, 4, 4, 64, 3) == -3 and q(0, 0, 4, 4, 64, 3) == R.ERR_SHAPE
        assert q(0, 1 << 11, 1 << 10, 1 << 10, 64, 3) == R.ERR_SHAPE             # 2^31 pixels
    # the entry points themselves answer the query's status before they touch an operand (null pointers come first)
    assert L.s2s_head_loss_fused(0, None, 8, None, None, None, None, None, 8, 1.0, None, None, None, None, None, 0, 1, 4, 4,
                                 104, 3, None) == -5
    from stain2stain_amd import ops
    assert not any(ops.tail_fusable(C, cout) for e, (_b, _h, _w, C, cout) in R.REFUSED if e == "tail")


# ---------------------------------------------------------------------------------------------------------------------
# models against autograd
# ---------------------------------------------------------------------------------------------------------------------
def _rel(a, r):
    return float((a.double() - r.double()).abs().max() / r.double().abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("shape,cout,bias,gs", [((2, 5, 7, 24), 3, True, 1.0), ((1, 4, 4, 64), 4, False, 0.25),
                                                ((3, 3, 5, 8), 1, True, 0.25)])
def test_head_and_eval_models_against_autograd(shape, cout, bias, gs):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(7 + C)
    x = torch.randn(shape, generator=g, dtype=F64)
    w = torch.randn(cout, C, generator=g, dtype=F64) * 0.3
    b = torch.randn(cout, generator=g, dtype=F64) if bias else None
    u = torch.randn(B, cout, H, W, generator=g, dtype=F64)
    xa = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wa = w.reshape(cout, C, 1, 1).clone().requires_grad_(True)
    ba = b.clone().requires_grad_(True) if bias else None
    v = F.conv2d(xa, wa, ba)
    v.retain_grad()
    loss = F.mse_loss(v, u)
    (loss * gs).backward()
    coef = 2.0 * gs / u.numel()
    m = R.head_model(x, w, b, u, coef, F64)
    assert _rel(m["loss"], loss.detach()) < TOL and _rel(R.eval_model(x, w, b, u), loss.detach()) < TOL
    assert _rel(m["v"], v.detach()) < TOL and _rel(m["g"], v.grad) < TOL
    assert _rel(m["dx"], xa.grad.permute(0, 2, 3, 1)) < TOL and _rel(m["dw"], wa.grad.reshape(cout, C)) < TOL
    if bias:
        assert _rel(m["db"], ba.grad) < TOL
    assert abs(R.coef_of(gs, u.numel()) - coef) <= 2.0 ** -24 * coef


@pytest.mark.parametrize("shape,cout,bias", [((2, 5, 7, 16), 3, True), ((3, 4, 4, 40), 4, False)])
def test_tail_model_against_autograd(shape, cout, bias):
    B, H, W, C = shape
    eps = 1e-5
    g = torch.Generator().manual_seed(11 + C)
    raw = torch.randn(shape, generator=g, dtype=F64) * 1.5 + 0.2
    gamma = 0.75 + 0.5 * torch.rand(C, generator=g, dtype=F64)
    beta = 0.2 * torch.rand(C, generator=g, dtype=F64)
    w = torch.randn(cout, C, generator=g, dtype=F64) * 0.3
    b = torch.randn(cout, generator=g, dtype=F64) if bias else None
    u = torch.randn(B, cout, H, W, generator=g, dtype=F64)
    r = raw.reshape(-1, C)
    mean, var = r.mean(0), r.var(0, unbiased=False)
    invstd = (var + eps).rsqrt()
    stats = torch.stack([mean, invstd, gamma * invstd, beta - mean * gamma * invstd])
    assert float((raw * stats[2] + stats[3]).abs().min()) > 1e-9           # no pre-activation on the ReLU's kink
    xa = raw.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    wa = w.reshape(cout, C, 1, 1).clone().requires_grad_(True)
    ba = b.clone().requires_grad_(True) if bias else None
    a = F.relu(F.batch_norm(xa, None, None, ga, be, training=True, eps=eps))
    a.retain_grad()
    v = F.conv2d(a, wa, ba)
    loss = F.mse_loss(v, u)
    loss.backward()
    m = R.tail_model(raw, stats, gamma, w, b, u, 2.0 / u.numel(), F64)
    assert _rel(m["loss"], loss.detach()) < TOL and _rel(m["v"], v.detach()) < TOL
    assert _rel(m["act"], a.detach().permute(0, 2, 3, 1)) < TOL and _rel(m["da"], a.grad.permute(0, 2, 3, 1)) < TOL
    assert _rel(m["draw"], xa.grad.permute(0, 2, 3, 1)) < 1e-10            # (cancellation in dz - c1 - xhat c2)
    assert _rel(m["dgamma"], ga.grad) < TOL and _rel(m["dbeta"], be.grad) < TOL
    assert _rel(m["dw"], wa.grad.reshape(cout, C)) < TOL
    if bias:
        assert _rel(m["db"], ba.grad) < TOL
    # the conv bias in front of a train-mode BatchNorm has no gradient: the sum of d raw over the pixels vanishes
    assert float(m["draw"].reshape(-1, C).sum(0).abs().max()) < 1e-12 * float(m["draw"].abs().max()) * r.shape[0]
    # the kernel's means forced into d raw: the same values give the same d raw
    m2 = R.tail_model(raw, stats, gamma, w, b, u, 2.0 / u.numel(), F64, means=(m["c1"], m["c2"]))
    assert torch.equal(m2["draw_forced_pre"], m["draw_pre"])


# ---------------------------------------------------------------------------------------------------------------------
# the exact tier
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("head", n) for n in R.HEAD] + [("tail", n) for n in R.TAIL]
                         + [("eval", n) for n in R.EVAL])
def test_exact_tier_preconditions(kind, name):
    assert R.exact_preconditions(kind, name) == []


def test_exact_tier_has_power_of_two_counts_for_the_tail():
    """c1, c2 and d raw are held bit for bit only there: at least one such row per lanes count."""
    for lanes in (1, 2, 4, 8, 16, 32, 64):
        n = [s[0] * s[1] * s[2] for (s, _o, f) in R.TAIL.values() if f[0] == lanes]
        assert any(v & (v - 1) == 0 for v in n), lanes
