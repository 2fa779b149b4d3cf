"""tests/loss_forms_ref.py is right, and its tables reach what they were written for (host code only: no GPU).

  * the float64 models agree with torch's own float64 evaluation to 1e-12: torch.sigmoid / binary_cross_entropy_with_logits,
    torch.softmax / F.one_hot / F.cross_entropy(ignore_index), autograd for every gradient, index_add_ for the table;
  * every table holds every form by enumeration (one ragged block, several blocks with a ragged last one, exactly full,
    grid-stride with a partial last round, every C, every scalar off its default): trimming a table fails here;
  * every yardstick (torch's fp32 evaluation) is within its quantity's hard bound: the rows are ones the reference passes;
  * the mirrored ``work`` sizes cover what each launcher writes;
  * the wrappers of ops.py refuse a mismatched mask, a target on another device and labels the kernels cannot read,
    before any entry point of the library is reached."""
import pytest
import torch
import torch.nn.functional as F

import loss_forms_ref as R

F32, F64 = R.F32, R.F64
TOL = 1e-12


def _close(a, b, tol=TOL):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
def _torch_binary(z, g, smooth, dw, gs):
    z = z.double().requires_grad_(True)
    g = g.double()
    p = torch.sigmoid(z)
    dice = 1 - (2.0 * (p * g).sum() + R.f32(smooth)) / (p.sum() + g.sum() + R.f32(smooth))
    bce = F.binary_cross_entropy_with_logits(z, g)
    seg = R.f32(dw) * dice + (1 - R.f32(dw)) * bce
    (seg * R.f32(gs)).backward()
    return torch.stack([seg, dice, bce]).detach(), z.grad


@pytest.mark.parametrize("name", [n for n, r in R.BIN_ROWS.items() if r["n"] <= 257 and r["logits"] == "normal"])
def test_binary_model_is_torch_float64(name):
    c = R.bin_case(name)
    out, dz = _torch_binary(c["z"], c["g"], c["smooth"], c["dw"], c["gs"])
    assert _close(c["ref"]["out"], out) and _close(c["ref"]["dz"], dz), name


def test_binary_model_keeps_the_saturated_gradients():
    """Autograd's float64 sigmoid backward is p (1 - p) with 1 - p rounded; the model's 1 - p = sigmoid(-z) is not.  They
    agree to 1e-12 of the largest element (above) and, on the specials, element by element to float64's cancellation."""
    for dw in (1.0, 0.0, 0.3):
        c = R.bin_case(f"specials-dw{dw:g}")
        out, dz = _torch_binary(c["z"], c["g"], c["smooth"], c["dw"], c["gs"])
        ref = c["ref"]["dz"]
        assert _close(c["ref"]["out"], out)
        assert bool(((ref - dz).abs() <= 1e-12 * ref.abs() + 2.0 ** -53).all())
        assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(c["ref"]["out"]).all())
        assert set(R.BIN_SPECIALS) == {0.0, 1e-30, -1e-30, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0}
        assert c["z"].numel() == 18 and float(c["g"].sum()) == 9.0
        assert c["ref"]["a"] < 1.0 and c["ref"]["b"] < 1.0                 # the factors BIN_UNDERFLOW was derived with
    # a saturated logit with the right label has a gradient that fp32's p - g cannot see
    c = R.bin_case("specials-dw0")
    i = R.BIN_SPECIALS.index(20.0) + len(R.BIN_SPECIALS)
    assert float(c["g"][i]) == 1.0 and -1e-9 < float(c["ref"]["dz"][i]) < -1e-11


def _torch_multiclass(z, t, ignore, smooth, dw, gs):
    B, C, HW = z.shape
    z = z.double().requires_grad_(True)
    p = torch.softmax(z, dim=1)
    oh = F.one_hot(t, C).permute(0, 2, 1).double()
    valid = (t != ignore).double().unsqueeze(1) if ignore >= 0 else torch.ones(B, 1, HW, dtype=F64)
    scores = []
    for c in range(C):
        pc, gc = p[:, c:c + 1] * valid, oh[:, c:c + 1] * valid
        scores.append((2.0 * (pc * gc).sum() + R.f32(smooth)) / (pc.sum() + gc.sum() + R.f32(smooth)))
    dice = 1 - torch.stack(scores).mean()
    ce = F.cross_entropy(z, t, ignore_index=ignore)
    return z, dice, ce


@pytest.mark.parametrize("name", [n for n, r in R.MC_ROWS.items() if r["B"] * r["HW"] <= 514 and not r["all_ignored"]])
def test_multiclass_model_is_torch_float64(name):
    c = R.mc_case(name)
    z, dice, ce = _torch_multiclass(c["z"], c["t"], c["ignore"], c["smooth"], c["dw"], c["gs"])
    seg = R.f32(c["dw"]) * dice + (1 - R.f32(c["dw"])) * ce
    (seg * R.f32(c["gs"])).backward()
    assert _close(c["ref"]["out"], torch.stack([seg, dice, ce]).detach()), name
    assert _close(c["ref"]["dz"], z.grad), name
    assert bool(torch.equal(R.first_argmax(c["z"]), torch.argmax(c["z"], dim=1)))        # torch's CPU tie rule, written out


@pytest.mark.parametrize("C", R.MC_VARIANT_C)
def test_multiclass_all_ignored_row_is_torch_float64(C):
    c = R.mc_case(f"all-ignored-C{C}")
    assert bool((c["t"] == c["ignore"]).all()) and 0 <= c["ignore"] < C
    z, dice, ce = _torch_multiclass(c["z"], c["t"], c["ignore"], c["smooth"], c["dw"], c["gs"])
    ce.backward()
    assert bool(torch.isnan(ce)) and float(z.grad.abs().max()) == 0.0                  # NaN value, zero CE gradient
    out, dz = c["ref"]["out"], c["ref"]["dz"]
    assert bool(torch.isnan(out[0])) and bool(torch.isnan(out[2])) and float(out[1]) == 0.0 == float(dice.detach())
    assert float(dz.abs().max()) == 0.0


def test_metric_models():
    c = R.bin_case("n257")
    I, P, G, U = c["counts_hi"]
    pred = torch.sigmoid(c["z"].double()) > 0.5
    m = c["g"] != 0
    assert [I, P, G, U] == [int((pred & m).sum()), int(pred.sum()), int(m.sum()), int((pred | m).sum())]
    d, i = R.metric_model(I, P + G, U)
    assert abs(d - (2 * I + 1e-7) / (P + G + 1e-7)) < 1e-15 and abs(i - (I + 1e-7) / (U + 1e-7)) < 1e-15
    k = R.mc_case("3x85-C5")
    cn = k["counts"]
    pred = torch.argmax(k["z"], dim=1)
    for cl in range(5):
        assert cn[:, cl].tolist() == [int(((pred == cl) & (k["t"] == cl)).sum()), int((pred == cl).sum()), int((k["t"] == cl).sum()),
                                      int(((pred == cl) | (k["t"] == cl)).sum())]
    d, i = R.mc_metric_model(cn, 1)
    want = [R.metric_model(float(cn[0, cl]), float(cn[1, cl] + cn[2, cl]), float(cn[3, cl])) for cl in (0, 2, 3, 4)]
    assert abs(d - sum(w[0] for w in want) / 4) < 1e-15 and abs(i - sum(w[1] for w in want) / 4) < 1e-15


@pytest.mark.parametrize("name", [n for n, r in R.WMSE_ROWS.items() if r["shape"] != R.LV_STRIDING])
def test_wmse_model_is_torch_float64(name):
    c = R.wmse_case(name)
    v = c["v"].double().requires_grad_(True)
    w = (1.0 + R.f32(c["lam"]) * c["m"].double())[:, None, :].expand_as(v)
    loss = (w * (v - c["u"].double()) ** 2).sum() / (w.sum() + 1e-8)
    (loss * R.f32(c["gs"])).backward()
    assert _close(c["ref"]["out"], loss.detach().reshape(1)) and _close(c["ref"]["dv"], v.grad), name
    if c["lam"] == 0.0:
        plain = R.mse_model(c["v"], c["u"], c["gs"])
        u = c["u"].double()
        v2 = c["v"].double().requires_grad_(True)
        (F.mse_loss(v2, u) * R.f32(c["gs"])).backward()
        assert _close(plain["out"], F.mse_loss(v2, u).detach().reshape(1)) and _close(plain["dv"], v2.grad)
        assert _close(c["ref"]["out"], plain["out"], 1e-7) and _close(c["ref"]["dv"], plain["dv"], 1e-7)    # the 1e-8 of the divisor


@pytest.mark.parametrize("name", [n for n, r in R.CHARB_ROWS.items() if r["shape"] != R.LV_STRIDING])
def test_charbonnier_model_is_torch_float64(name):
    c = R.charb_case(name)
    B, C = c["shape"][:2]
    a, b, m = c["a"].double(), c["b"].double(), c["m"].double()
    ec, ea = R.f32(c["eps_charb"]), R.f32(c["eps_area"])
    want = (torch.sqrt((a - b) ** 2 + ec ** 2) * m[:, None, :]).sum() / (m.sum() * C + ea)
    assert _close(c["ref"]["out"], want.reshape(1)), name
    if c["same"]:           # every channel of an ROI pixel contributes eps_charb: eps_charb (sum(m) C) / (sum(m) C + eps_area)
        area = float(m.sum()) * C
        assert abs(float(c["ref"]["out"]) - ec * area / (area + ea)) <= 1e-12 * ec
    if c["mask"] == "empty":
        assert float(c["ref"]["out"]) == 0.0


@pytest.mark.parametrize("name", list(R.EMBED_ROWS))
def test_embed_models(name):
    c = R.embed_case(name)
    k, dim = c["classes"], c["dim"]
    table = c["table"].double().requires_grad_(True)
    out = c["temb"].double() + table[c["y"]]
    (out * c["dout"].double()).sum().backward()
    assert _close(R.embed_add_model(c["temb"], c["table"], c["y"]), out.detach())
    assert _close(c["ref"]["dtable"], table.grad)
    assert _close(c["ref"]["dtable"], torch.zeros(k, dim, dtype=F64).index_add_(0, c["y"], c["dout"].double()))
    assert _close(c["seq"], c["ref"]["dtable"], 1e-5)
    absent = ~c["present"]
    assert bool((c["seq"][absent].view(torch.int32) == 0).all())                       # +0, not -0
    assert int(c["y"].min()) >= 0 and int(c["y"].max()) < k


# ---------------------------------------------------------------------------------------------------------------------
# the tables hold every form
# ---------------------------------------------------------------------------------------------------------------------
def test_constants_mirror_the_sources():
    import os
    import re
    from stain2stain_amd import _native
    src = {f: open(os.path.join(_native.CSRC, f)).read() for f in ("seg_loss.hip", "eval_metrics.hip", "loss_variants.hip")}
    assert (R.THREADS, R.PART_ROWS, R.BWD_CAP, R.MC_SUMS, R.MC_CNTS, R.MC_MAX) == (256, 512, 4096, 26, 32, 8)
    assert "SEG_BLOCKS = 512" in src["seg_loss.hip"] and "EV_BLOCKS = 512" in src["eval_metrics.hip"]
    assert "LV_BLOCKS = 512" in src["loss_variants.hip"]
    assert src["seg_loss.hip"].count("gb > 4096") == 2 and src["loss_variants.hip"].count("gb > 4096") == 1
    assert "MC_SUMS = 26" in src["seg_loss.hip"] and "MC_SUMS = 26, MC_CNTS = 32" in src["eval_metrics.hip"]
    header = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", open(_native.HEADER).read()))
    for text in ("work: double[512*4 + 4]", "work: double[(512 + 1) * 26]", "work: double[512*8]", "work: double[512*58]",
                 "work: double[512*2 + 2]"):
        assert text in header, text
    assert R.WORK == {"seg_loss": 2052, "seg_loss_multiclass": 13338, "seg_eval_binary": 4096, "seg_eval_multiclass": 29696,
                      "weighted_mse": 1026, "charbonnier_roi": 1026}


def test_work_sizes_cover_what_the_launchers_write():
    sizes = {"seg_loss": [r["n"] for r in R.BIN_ROWS.values()], "seg_eval_binary": [r["n"] for r in R.BIN_ROWS.values()],
             "seg_loss_multiclass": [r["B"] * r["HW"] for r in R.MC_ROWS.values()],
             "seg_eval_multiclass": [r["B"] * r["HW"] for r in R.MC_ROWS.values()],
             "weighted_mse": [r["shape"][0] * r["shape"][2] * r["shape"][3] for r in R.WMSE_ROWS.values()],
             "charbonnier_roi": [r["shape"][0] * r["shape"][2] * r["shape"][3] for r in R.CHARB_ROWS.values()]}
    for kind, items in sizes.items():
        extents = [R.work_extent(kind, n) for n in items]
        assert max(extents) == R.WORK[kind], kind                    # a striding row fills it to the last element
        assert all(e <= R.WORK[kind] for e in extents)
        assert R.walk(max(items), R.PART_ROWS)["grid"] == R.PART_ROWS


FORMS = {"one-ragged", "blocks-ragged", "one-full", "blocks-full", "stride-partial"}


def test_binary_table_holds_every_form():
    assert R.BIN_N == [1, 255, 256, 257, 131_072, 131_073, 1_048_576 + 777]
    red = {n: R.reduce_form(n) for n in R.BIN_N}
    bwd = {n: R.bwd_form(n) for n in R.BIN_N}
    assert red == {1: "one-ragged", 255: "one-ragged", 256: "one-full", 257: "blocks-ragged", 131_072: "blocks-full",
                   131_073: "stride-partial", 1_049_353: "stride-partial"}
    assert R.walk(131_073, R.PART_ROWS)["last"] == 1                                     # the first strided element
    assert set(bwd.values()) == FORMS and bwd[131_073] == "blocks-ragged"
    assert [n for n, f in bwd.items() if f.startswith("stride")] == [R.BIN_STRIDING]
    assert R.walk(R.BIN_STRIDING, R.BWD_CAP) == dict(grid=4096, rounds=2, last=777, strides=True, partial_last=True, ragged=True)
    rows = R.BIN_ROWS.values()
    assert {n for n in R.BIN_N} <= {r["n"] for r in rows if r["mask"] == "random" and r["dw"] == 0.3}
    for key, values in (("dw", {1.0, 0.0, 0.3}), ("smooth", {1.0, 1e-6}), ("gs", {1.0, 0.25}),
                        ("mask", {"random", "zeros", "ones", "specials"})):
        assert {r[key] for r in rows} == values, key
        for v in values - {"specials"}:                              # each also on a row whose backward strides, or whose reduce does
            assert any(r[key] == v and R.reduce_form(r["n"]) == "stride-partial" for r in rows), (key, v)
    assert len({r["n"] for r in rows if r["gs"] == 0.25}) == 3
    assert {r["dw"] for r in rows if r["logits"] == "specials"} == {1.0, 0.0, 0.3}
    assert sum(r["logits"] == "knife" for r in rows) == 1 and set(R.BIN_OPS_ROWS) <= set(R.BIN_ROWS)
    assert [R.bwd_form(R.BIN_ROWS[n]["n"]).startswith("stride") for n in R.BIN_OPS_ROWS] == [False, True]


def test_binary_masks_and_count_bands():
    for name, r in R.BIN_ROWS.items():
        c = R.bin_case(name)
        if r["logits"] == "normal":
            assert c["counts_lo"] == c["counts_hi"], name              # no element of these rows is near the threshold
            assert float(c["z"].abs().min()) >= 1e-3
        if r["mask"] == "random" and r["n"] >= 255:
            assert 0.3 < float(c["g"].mean()) < 0.5
    k = R.bin_case("knife-edge")
    assert R.KNIFE == [0.0, -1e-8, 1e-8, 6e-8, 1.2e-7, 1e-6] and k["z"].numel() == 300
    assert k["counts_hi"][1] == 200 and k["counts_lo"][1] == 50 and k["counts_lo"][2] == k["counts_hi"][2]
    assert all(lo <= hi for lo, hi in zip(k["counts_lo"], k["counts_hi"]))
    assert 0 < k["counts_lo"][0] < k["counts_hi"][0] and k["counts_lo"][3] < k["counts_hi"][3]


def test_multiclass_table_holds_every_form():
    assert R.MC_C == [2, 3, 4, 5, 6, 7, 8] and R.MC_SHAPES == [(5, 1), (3, 85), (1, 256), (2, 257), (3, 43_699)]
    assert R.MC_STRIDING == (3, 349_537) and R.MC_STRIDING_C == [2, 8]
    rows = R.MC_ROWS
    for B, HW in R.MC_SHAPES:
        assert all(f"{B}x{HW}-C{C}" in rows for C in R.MC_C)
    npix = {s: s[0] * s[1] for s in R.MC_SHAPES + [R.MC_STRIDING]}
    assert [R.reduce_form(n) for n in npix.values()] == ["one-ragged", "one-ragged", "one-full", "blocks-ragged", "stride-partial",
                                                         "stride-partial"]
    assert [R.bwd_form(n) for n in npix.values()][-2:] == ["blocks-ragged", "stride-partial"]
    assert npix[(3, 85)] == 255 and npix[(3, 43_699)] == 131_097 and npix[R.MC_STRIDING] == 1_048_611
    assert 2 * 85 < 255 <= R.THREADS                                 # two sample boundaries inside one workgroup
    assert (5, 1) in npix                                            # HW = 1: n = i, q = 0
    # on a second trip n = i / HW > 0 and q > 0: the strided pixels of the reduce lie in the last sample
    w = R.walk(131_097, R.PART_ROWS)
    assert (131_072 // 43_699, 131_072 % 43_699) == (2, 43_674) and w["last"] == 25
    assert {r["C"] for r in rows.values() if r["B"] * r["HW"] == 1_048_611} == {2, 8}
    for C in R.MC_C:                                                 # each ignore_index at each C, on the shape rows alone
        assert {r["ignore"] for r in rows.values() if r["C"] == C and (r["B"], r["HW"]) in R.MC_SHAPES} >= {-100, 0, C - 1}, C
    for C in R.MC_VARIANT_C:
        assert {v for v in R.MC_VARIANTS if f"{v}-C{C}" in rows} == set(R.MC_VARIANTS)
    v = {k: rows[f"{k}-C5"] for k in R.MC_VARIANTS}
    assert (v["ignore-100"]["ignore"], v["ignore0"]["ignore"], v["ignore-last"]["ignore"]) == (-100, 0, 4)
    assert v["absent"]["absent"] and v["x4"]["scale"] == 4.0 and v["x40"]["scale"] == 40.0
    assert v["dw1"]["dw"] == 1.0 and v["dw0"]["dw"] == 0.0 and v["smooth1e-6"]["smooth"] == 1e-6 and v["gs0.25"]["gs"] == 0.25
    assert v["all-ignored"]["all_ignored"] and v["all-ignored"]["ignore"] == 4
    assert any(r["gs"] == 0.25 and R.bwd_form(r["B"] * r["HW"]) == "stride-partial" for r in rows.values())
    assert set(R.MC_OPS_ROWS) <= set(rows)
    assert [R.bwd_form(rows[n]["B"] * rows[n]["HW"]).startswith("stride") for n in R.MC_OPS_ROWS] == [False, True]


@pytest.mark.parametrize("C", R.MC_VARIANT_C)
def test_multiclass_cases_are_what_the_rows_say(C):
    c = R.mc_case(f"absent-C{C}")
    assert c["absent"] is not None and not bool((c["t"] == c["absent"]).any())
    z = R.mc_case(f"ignore0-C{C}")
    assert bool(torch.equal(z["z"][:, 1, ::3], z["z"][:, 0, ::3])) and not bool(torch.equal(z["z"][:, 1, 1::3], z["z"][:, 0, 1::3]))
    assert bool((z["t"] == 0).any()) and set(z["t"].unique().tolist()) == set(range(C))
    p = torch.softmax(R.mc_case(f"x40-C{C}")["z"], dim=1)
    zero = float((p == 0).float().mean())                            # of C probabilities at most C - 1 can underflow
    assert zero > (0.5 if C > 2 else 0.1), zero                      # most of them do in fp32 where there are more than two


def test_lv_tables_hold_every_form():
    assert R.LV_SHAPES == [(1, 1, 1, 1), (1, 1, 5, 7), (3, 4, 5, 17), (2, 3, 16, 16), (2, 3, 257, 255), (2, 3, 257, 256), (3, 3, 600, 583)]
    pix = [s[0] * s[2] * s[3] for s in R.LV_SHAPES]
    assert pix == [1, 35, 255, 512, 131_070, 131_584, 1_049_400]
    assert [R.reduce_form(n) for n in pix] == ["one-ragged", "one-ragged", "one-ragged", "blocks-full", "blocks-ragged", "stride-partial",
                                               "stride-partial"]
    elems = [s[0] * s[1] * s[2] * s[3] for s in R.LV_SHAPES]
    assert [R.bwd_form(n).startswith("stride") for n in elems] == [False] * 6 + [True]
    assert R.walk(elems[-1], R.BWD_CAP)["partial_last"] and R.walk(elems[-1], R.BWD_CAP)["rounds"] == 4
    w = R.WMSE_ROWS.values()
    assert all(R._sid(s) in R.WMSE_ROWS and R._sid(s) in R.CHARB_ROWS for s in R.LV_SHAPES)
    for key, values in (("lam", {0.0, 10.0}), ("mask", {"random", "empty", "full"}), ("gs", {1.0, 0.25})):
        for shape in (R.LV_SMALL, R.LV_STRIDING):
            assert {r[key] for r in w if r["shape"] == shape} == values, (key, shape)
    c = R.CHARB_ROWS.values()
    assert {r["eps_charb"] for r in c} == {1e-3, 1e-6} and {r["eps_area"] for r in c} == {1e-8, 1.0}
    assert {r["mask"] for r in c} == {"random", "empty", "full"} and any(r["same"] for r in c)
    assert any(r["shape"] == R.LV_STRIDING and r["eps_area"] == 1.0 for r in c)
    assert set(R.WMSE_OPS_ROWS) <= set(R.WMSE_ROWS) and set(R.CHARB_OPS_ROWS) <= set(R.CHARB_ROWS)
    assert {R.WMSE_ROWS[n]["shape"] for n in R.WMSE_OPS_ROWS} == {R.LV_SMALL, R.LV_STRIDING}
    assert {R.CHARB_ROWS[n]["shape"] for n in R.CHARB_OPS_ROWS} == {R.LV_SMALL, R.LV_STRIDING}


def test_embed_table_holds_every_form():
    assert R.EMBED[:5] == [(1, 4, 1), (3, 32, 3), (16, 256, 3), (5, 1024, 10), (600, 36, 7)]
    assert len(R.EMBED_ROWS) == 3 * len(R.EMBED)
    kinds = {"one": 0, "absent": 0, "every": 0}
    for name, r in R.EMBED_ROWS.items():
        c = R.embed_case(name)
        seen = int(c["present"].sum())
        kinds["one"] += seen == 1
        kinds["absent"] += 1 < seen < r["classes"]
        kinds["every"] += seen == r["classes"] and r["classes"] > 1
    assert all(v >= 2 for v in kinds.values()), kinds
    assert any(r["B"] * r["dim"] % 256 and r["B"] * r["dim"] > 256 for r in R.EMBED_ROWS.values())       # ragged last block of the add
    assert any(r["classes"] * r["dim"] % 256 and r["classes"] * r["dim"] > 256 for r in R.EMBED_ROWS.values())
    assert any(r["B"] * r["dim"] < 256 for r in R.EMBED_ROWS.values()) and set(R.EMBED_OPS_ROWS) <= set(R.EMBED_ROWS)


# ---------------------------------------------------------------------------------------------------------------------
# the reference alone passes: every yardstick within its quantity's hard bound
# ---------------------------------------------------------------------------------------------------------------------
HARD = {"out": 1e-5, "dz-binary": 1e-5, "dz-multiclass": 1e-4, "dv": 1e-5, "dtable": 1e-5}


def test_yardsticks_are_within_the_hard_bounds():
    worst = {}
    def take(q, row, dev):
        if dev[0] == dev[0] and max(dev) > worst.get(q, (0.0, ""))[0]:
            worst[q] = (max(dev), row)
    for name, r in R.BIN_ROWS.items():
        if r["logits"] == "specials":
            continue                                                 # held element by element, not in a norm
        c = R.bin_case(name)
        for dev in c["yard"]["out-each"]:
            take("out", name, dev)
        take("dz-binary", name, c["yard"]["dz"])
    for name, r in R.MC_ROWS.items():
        if r["all_ignored"]:
            continue                                                 # NaN by design
        c = R.mc_case(name)
        for dev in c["yard"]["out-each"]:
            take("out", name, dev)
        take("dz-multiclass", name, c["yard"]["dz"])
    for name in R.WMSE_ROWS:
        c = R.wmse_case(name)
        take("out", name, c["yard"]["out-each"][0])
        take("dv", name, c["yard"]["dv"])
    for name, r in R.CHARB_ROWS.items():
        if r["mask"] != "empty":
            take("out", name, R.charb_case(name)["yard"]["out-each"][0])
    for name in R.EMBED_ROWS:
        take("dtable", name, R.embed_case(name)["yard"]["dtable"])
    print(worst)
    assert set(worst) == set(HARD)
    for q, (dev, row) in worst.items():
        assert dev < HARD[q], (q, row, dev)


# ---------------------------------------------------------------------------------------------------------------------
# the wrappers refuse before the device
# ---------------------------------------------------------------------------------------------------------------------
class _Unreachable:
    """A stand-in for the library: reaching any entry point fails the test."""

    def __getattr__(self, name):
        def entry(*args):                                            # the arguments' own checks run before the call
            pytest.fail(f"the wrapper reached {name} instead of refusing")
        return entry


@pytest.fixture
def no_library(monkeypatch):
    from stain2stain_amd import ops
    monkeypatch.setattr(ops, "_L", lambda: _Unreachable())
    monkeypatch.setattr(ops, "_stream", lambda: pytest.fail("the wrapper asked for a stream instead of refusing"))
    return ops


def test_seg_loss_refuses_a_mask_of_another_shape(no_library):
    ops = no_library
    z = torch.zeros(2, 1, 8, 8)
    for g in (torch.zeros(2, 1, 8, 7), torch.zeros(1, 1, 8, 8), torch.zeros(2, 8), torch.zeros(64), torch.zeros(2, 2, 8, 8),
              torch.zeros(2, 7, 8), torch.zeros(128 - 1)):
        with pytest.raises(RuntimeError, match="does not match logits"):
            ops.seg_loss(z, g)
    with pytest.raises(RuntimeError, match="does not match logits"):
        ops.seg_loss(torch.zeros(128), torch.zeros(127))             # a shorter g would be read past its end
    with pytest.raises(RuntimeError, match="does not match logits"):
        ops.seg_loss(torch.zeros(2, 8, 8), torch.zeros(2, 1, 8, 8))  # the allowance is [B,H,W] for [B,1,H,W] logits only
    for g in (torch.zeros(2, 1, 8, 8), torch.zeros(2, 8, 8)):        # a sound pair is refused only for where it lives
        with pytest.raises(RuntimeError, match="GPU"):
            ops.seg_loss(z, g)


def test_seg_loss_multiclass_refuses_a_target_on_another_device(no_library):
    ops = no_library
    z = torch.zeros(1, 3, 4, 4, device="meta")
    for validate in (True, False):
        with pytest.raises(RuntimeError, match="different devices"):
            ops.seg_loss_multiclass(z, torch.zeros(1, 4, 4, dtype=torch.long), validate=validate)
    with pytest.raises(RuntimeError, match="different devices"):
        ops.seg_loss_multiclass(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long, device="meta"), validate=False)


def test_class_embed_wrappers_refuse_labels_the_kernels_cannot_read(no_library):
    ops = no_library
    temb, table, dout = torch.zeros(4, 8), torch.zeros(3, 8), torch.zeros(4, 8)
    y = torch.zeros(4, dtype=torch.int64)
    bad = [y.int(), y.float(), torch.zeros(8, dtype=torch.int64)[::2], y.to("meta"), y[:3], y.reshape(4, 1), y.reshape(2, 2)]
    for b in bad:
        with pytest.raises(RuntimeError, match="class_embed_add wants"):
            ops.class_embed_add(temb, table, b)
        with pytest.raises(RuntimeError, match="class_embed_bwd wants"):
            ops.class_embed_bwd(dout, b, 3)
    for t in (torch.zeros(8), torch.zeros(1, 3, 8)):
        with pytest.raises(RuntimeError, match="class_embed_add wants temb"):
            ops.class_embed_add(temb, t, y)
        with pytest.raises(RuntimeError, match="class_embed_add wants temb"):
            ops.class_embed_add(t, table, y)
        with pytest.raises(RuntimeError, match="class_embed_bwd wants dout"):
            ops.class_embed_bwd(t, y, 3)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.class_embed_add(temb, torch.zeros(3, 7), y)
    with pytest.raises(RuntimeError, match="GPU"):                   # sound operands are refused only for where they live
        ops.class_embed_add(temb, table, y)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.class_embed_bwd(dout, y, 3)
