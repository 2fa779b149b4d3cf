"""tests/glue_forms_ref.py is right, and its tables reach what they were written for (host code only: no GPU).

  * the float64 models agree with torch: Adam with torch.optim.Adam on float64 tensors over several steps, lerp with
    torch.lerp, linear / SiLU / MSE with autograd, the time embedding and the probability path with the oracle, the pack
    layouts by reshape / permute / pad with a gather by the index formula, the layout permutations with each other;
  * every table holds every form by enumeration (a striding row, an unrolled-loop row, a ragged row, a slice row, an
    accumulate row, a null-pointer row, and the sizes around every threshold): trimming a table fails here;
  * the exact tiers' preconditions hold."""
import pytest
import torch

import glue_forms_ref as R

BF, F32, F64 = R.BF, R.F32, R.F64
TOL = 1e-12


def _close(a, b, tol=TOL):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.ADAM_SCALARS))
def test_adam_ref_is_torch_optim_adam(name):
    sc = dict(R.ADAM_SCALARS[name])
    sc.pop("ema_weight")
    c = R.adam_case(257, "positive")
    p = torch.nn.Parameter(c["p"].double().clone())
    opt = torch.optim.Adam([p], lr=R.f32(sc["lr"]), betas=(R.f32(sc["beta1"]), R.f32(sc["beta2"])), eps=R.f32(sc["eps"]),
                           weight_decay=R.f32(sc["weight_decay"]))
    state = dict(p=c["p"].double(), m=torch.zeros(257, dtype=F64), v=torch.zeros(257, dtype=F64))
    for step in range(1, 5):
        g = torch.randn(257, generator=R._gen("adam-steps", step)) * 0.1
        p.grad = (g.double() * R.f32(sc["grad_scale"])).clone()
        opt.step()
        s = R.adam_scalars(**dict(sc, step=step))
        state = R.adam_ref(state["p"], g, state["m"], state["v"], s)
        assert _close(state["p"], p.detach()), (name, step)
        assert _close(state["m"], opt.state[p]["exp_avg"]) and _close(state["v"], opt.state[p]["exp_avg_sq"])


def test_adam_bias_corrections_are_the_entry_points():
    """ops.adam_hyper is documented as "formed exactly as s2s_adam_step forms its kernel arguments": the model's scalars are
    the same doubles."""
    from stain2stain_amd import ops
    for sc in R.ADAM_SCALARS.values():
        s = R.adam_scalars(**sc)
        h = ops.adam_hyper(sc["step"], sc["lr"], sc["beta1"], sc["beta2"], sc["eps"], sc["weight_decay"], sc["grad_scale"])
        assert h[5] == s["bc1"] and h[6] == s["bc2_sqrt"]
        assert [R.f32(x) for x in h[:5]] == [s["lr"], s["b1"], s["b2"], s["eps"], s["wd"]] and R.f32(h[7]) == s["gs"]


@pytest.mark.parametrize("w", [0.0, 1.0 - 0.999, 0.25, 0.5, 0.75, 1.0])
def test_lerp_ref_is_torch_lerp(w):
    g = R._gen("lerp", w)
    a, b = torch.randn(100, generator=g).double(), torch.randn(100, generator=g).double()
    assert _close(R.lerp_ref(a, b, w), torch.lerp(a, b, R.f32(w)))
    if w == 1.0:
        assert torch.equal(R.lerp_ref(a, b, w), b)


@pytest.mark.parametrize("shape", R.PACK)
def test_pack_ref_two_formulations(shape):
    w = R.pack_case(*shape)
    for dt in (BF, F32):
        a, b = R.pack_ref(w, dt), R.pack_gather(w, dt)
        assert a[0].numel() == R.pack_elems(*shape)[0] and a[1].numel() == R.pack_elems(*shape)[1]
        assert R.same_bits(a[0], b[0]) and R.same_bits(a[1], b[1])
    # spot values straight from the definition
    cout, cin = shape
    wf, wd = R.pack_ref(w, F32)
    for co, ci, tap in [(0, 0, 0), (cout - 1, cin - 1, 8), (cout // 2, cin // 2, 3)]:
        assert wf[(((ci // 32) * 9 + tap) * cout + co) * 32 + ci % 32] == w.reshape(cout, cin, 9)[co, ci, tap]
        assert wd[(((co // 32) * 9 + tap) * cin + ci) * 32 + co % 32] == w.reshape(cout, cin, 9)[co, ci, 8 - tap]
    if cin % 32:
        assert float(wf.reshape(-1, 32)[-1, cin % 32:].abs().max()) == 0.0


def test_pack_case_has_bf16_ties_both_ways():
    w = R.pack_case(32, 32).reshape(-1)
    bits = w.view(torch.int32)
    tie = (bits & 0xFFFF) == 0x8000
    assert int(tie.sum()) >= w.numel() // 3
    up = (R.round_to(w, BF).abs() > w.abs())[tie]
    assert bool(up.any()) and bool((~up).any())


def test_layout_refs_are_inverse_permutations():
    x = R.layout_case((2, 16, 5, 7))["x"]
    for dt in (BF, F32):
        y = R.nchw_to_nhwc_ref(x, dt)
        assert y.shape == (2, 5, 7, 16) and float(y[1, 3, 4, 9]) == float(R.round_to(x, dt)[1, 9, 3, 4])
        assert R.same_bits(R.nhwc_to_nchw_ref(y), R.round_to(x, dt))


def test_pixel_sum_ref():
    c = R.pixsum_case(3, 65, 72, "exact")
    ref = R.pixel_sum_ref(c["x"], c["base"])
    assert float(ref[2, 71]) == float(c["x"][2, 0, :, 71].double().sum() + c["base"][2, 71])
    assert float(c["x"].abs().max()) * 1000 + 8 < 2 ** 24          # the exact tier's sums are fp32 values in any order


@pytest.mark.parametrize("dim", R.TIME_DIMS)
def test_time_embedding_ref_is_the_oracle(dim):
    from oracle import unet_oracle as O
    t = R.time_case(5)
    assert R.same_bits(R.time_embedding_ref(t, dim, F32), O.time_embedding(t, dim))
    assert float((R.time_embedding_ref(t, dim) - O.time_embedding(t, dim).double()).abs().max()) < 1e-6
    assert float(R.time_embedding_ref(t, dim)[0, :dim // 2].abs().max()) == 0.0     # t = 0: sin 0


@pytest.mark.parametrize("shape", R.LINEAR)
def test_linear_and_silu_refs_are_autograd(shape):
    B, K, N = shape
    c = R.linear_case(B, K, N, "real")
    x, w, b = (c[k].double().requires_grad_(True) for k in ("x", "w", "b"))
    h = torch.nn.functional.linear(x, w, b)
    a = torch.nn.functional.silu(h)
    da = c["dy"].double()
    (a * da).sum().backward(retain_graph=True)
    assert _close(R.linear_fwd_ref(c["x"], c["w"], c["b"]), h.detach())
    assert _close(R.silu_fwd_ref(h.detach()), a.detach())
    dh = R.silu_bwd_ref(h.detach(), da)
    r = R.linear_bwd_ref(dh, c["x"], c["w"])
    assert _close(r["dx"], x.grad) and _close(r["dw"], w.grad) and _close(r["db"], b.grad)
    assert _close(R.linear_fwd_ref(c["x"], c["w"], None), (h - b).detach(), 1e-11)


def test_silu_specials_are_finite_in_both_precisions():
    c = R.silu_case(257)
    assert c["specials"] == len(R.SILU_SPECIALS) and set(R.SILU_SPECIALS) <= set(c["h"].tolist()) | {1e-30, -1e-30}
    for cd in (F32, F64):
        assert bool(torch.isfinite(R.silu_fwd_ref(c["h"], cd)).all())
        assert bool(torch.isfinite(R.silu_bwd_ref(c["h"], c["da"], cd)).all())


def test_cfm_and_mse_refs():
    from oracle import unet_oracle as O
    c = R.cfm_case(3, 288)
    t = torch.tensor(R.cfm_times(3)[0])
    sh = (3, 3, 8, 12)
    for sigma, eps in ((0.0, None), (0.1, c["eps"])):
        xt, ut = R.cfm_ref(c["x0"], c["x1"], t, eps, sigma)
        xo, uo = O.cfm_sample(c["x0"].double().reshape(sh), c["x1"].double().reshape(sh), t.double(), R.f32(sigma),
                              None if eps is None else eps.double().reshape(sh))
        assert _close(xt, xo.reshape(3, -1)) and _close(ut, uo.reshape(3, -1))
    xt, _ = R.cfm_ref(c["x0"], c["x1"], t, None, 0.0)
    assert torch.equal(xt[0].float(), c["x0"][0]) and torch.equal(xt[1].float(), c["x1"][1])
    m = R.mse_case(864, "real")
    v = m["v"].double().requires_grad_(True)
    loss = O.cfm_loss(v, m["u"].double())
    (loss * 0.25).backward()
    r = R.mse_ref(m["v"], m["u"], 0.25)
    assert _close(r["loss"], loss.detach()) and _close(r["dv"], v.grad, 1e-7)       # coef is an fp32 value
    assert R.mse_coef(0.25, 4096) == 2.0 * 0.25 / 4096


def test_err_norm_and_axpy_refs():
    c = R.err_case(257)
    for atol, rtol in R.ERR_TOLS:
        sc = R.f32(atol) + R.f32(rtol) * torch.maximum(c["y0"].abs(), c["y1"].abs()).double()
        assert float(sc.min()) > 0
        want = torch.sqrt(torch.mean((c["e"].double() / sc) ** 2))
        assert _close(R.err_norm_ref(c["e"], c["y0"], c["y1"], atol, rtol), want.reshape(1))
    a = R.axpy_case(1020)
    assert _close(R.axpy_ref(a["x"], a["y"], 1.0 / 3.0), torch.add(a["x"].double(), a["y"].double(), alpha=R.f32(1.0 / 3.0)))


# ---------------------------------------------------------------------------------------------------------------------
# the tables hold every form
# ---------------------------------------------------------------------------------------------------------------------
def test_walk_mirrors_the_launch_arithmetic():
    assert (R.THREADS, R.OPTIM_CAP, R.FLOW_CAP, R.EMA_CAP, R.MSE_CAP, R.CHUNK) == (256, 8192, 4096, 2048, 1024, 4096)
    w = R.walk(8192 * 256 + 1, R.OPTIM_CAP)
    assert w == dict(grid=8192, rounds=2, last=1, strides=True, partial_last=True, ragged=True)
    assert R.walk(8192 * 256, R.OPTIM_CAP)["rounds"] == 1 and R.walk(0, R.EMA_CAP)["grid"] == 1
    from stain2stain_amd import _native
    L = _native.lib()
    for n in (1, 4095, 4096, 4097, 12289):
        assert L.s2s_adam_multi_blocks(n) == R.adam_form(n)["multi_blocks"]
    for cout, cin in R.PACK:
        assert (L.s2s_pack_conv3x3_fwd_elems(cout, cin), L.s2s_pack_conv3x3_dgrad_elems(cout, cin)) == R.pack_elems(cout, cin)


def test_adam_tables_hold_every_form():
    forms = {n: R.adam_form(n) for n in R.ADAM_SIZES}
    assert {1, 3, 4, 255, 256, 257, 4095, 4096, 4097} <= set(forms)
    assert {f["tail"] for f in forms.values()} == {0, 1, 2, 3}
    assert any(not f["vector"] for f in forms.values())                              # the tail alone
    s = forms[R.ADAM_STRIDING]
    assert s["plain"]["strides"] and s["plain"]["partial_last"] and s["ema"]["strides"] and s["ema"]["partial_last"]
    assert s["tail"] == 3
    assert sum(f["plain"]["strides"] for f in forms.values()) == 1                   # nothing else needs the size
    assert any(f["plain"]["grid"] > 1 and not f["plain"]["strides"] for f in forms.values())
    assert any(f["multi_blocks"] == 2 and f["multi_ragged"] for f in forms.values())
    assert any(f["multi_blocks"] == 1 and not f["multi_ragged"] for f in forms.values())
    sc = R.ADAM_SCALARS.values()
    assert {s_["step"] for s_ in sc} == {1, 2, 1000, 10 ** 6}
    assert any(s_["weight_decay"] == 0 for s_ in sc) and any(s_["weight_decay"] != 0 and s_["grad_scale"] != 1 for s_ in sc)
    assert any(abs(R.f32(s_["ema_weight"])) < 0.5 for s_ in sc) and any(s_["ema_weight"] == 1.0 for s_ in sc)   # both lerp branches
    assert set(R.ADAM_V_STARTS) == {"zeros", "positive"} and R.ADAM_MAGNITUDES == (1.0, 1e-4, 1e-8)
    # eps is half the denominator somewhere: |g| ~ 1e-8, v = 0, step 1
    c = R.adam_case(4097, "zeros")
    r = R.adam_model(c, R.ADAM_SCALARS["step1"])
    share = 1e-8 / (r["v"].sqrt() / R.adam_scalars(**R.ADAM_SCALARS["step1"])["bc2_sqrt"] + 1e-8)
    assert bool(((share > 0.3) & (share < 0.7)).any()) and bool((share < 1e-6).any())
    z0, z1 = R.adam_zero_block(4097)
    assert z1 > z0 and float(c["g"][z0:z1].abs().max()) == 0 and bool((share[z0:z1] == 1).all())
    assert R.ADAM_MULTI["mixed"] == [1, 4095, 4096, 4097, 7, 12289] and R.ADAM_MULTI["33x1"] == [1] * 33
    assert len(R.ADAM_MULTI["one"]) == 1


def test_pack_tables_hold_every_form():
    forms = {s: R.pack_form(*s) for s in R.PACK}
    assert forms[(32, 32)]["whole"] == 1 and forms[(32, 32)]["element"] == 0
    assert forms[(96, 160)]["whole"] == 15
    assert forms[(64, 66)]["inside_unaligned_rows"] == 4 and forms[(64, 66)]["whole"] == 0      # (Cin * 9) % 4 != 0
    assert any(f["pad_ci"] and not f["pad_co"] for f in forms.values())                # zero lanes in Wf only
    assert any(f["pad_ci"] and f["pad_co"] and f["tiles"] == 1 for f in forms.values())      # one ragged tile
    assert any(f["pad_ci"] and f["pad_co"] and f["tiles"] > 1 for f in forms.values())
    assert forms[(512, 512)]["single"]["strides"] and forms[(512, 512)]["single_fwd_only"]["strides"]
    assert sum(f["single"]["strides"] for f in forms.values()) == 1
    assert set(R.PACK_WANT_DGRAD) == {True, False}                                     # a null wd on the single kernel
    assert len(R.PACK_ORDERS) == 2 and R.PACK_ORDERS[0] != R.PACK_ORDERS[1]
    assert all(sorted(o) == list(range(len(R.PACK))) for o in R.PACK_ORDERS)
    assert 0 <= R.PACK_NULL_WD < len(R.PACK) and R.PACK_MISALIGNED
    # the linear search over `start` passes layers of one tile and of many
    assert any(f["tiles"] == 1 for f in forms.values()) and any(f["tiles"] >= 256 for f in forms.values())


def test_layout_tables_hold_every_form():
    forms = {s: R.layout_form(s) for s in R.LAYOUT}
    assert sum(f["strides"] for f in forms.values()) == 1 and forms[R.LAYOUT[-1]]["partial_last"]
    assert any(f["grid"] == 1 and f["ragged"] for f in forms.values()) and any(s[1] > 8 and s[0] > 1 for s in forms)
    assert None in R.LAYOUT_SLICES and (8, 16) in R.LAYOUT_SLICES and (16, 8) in R.LAYOUT_SLICES
    assert set(R.LAYOUT_ACCUMULATE) == {False, True}
    assert {w for w, _, _ in R.LAYOUT_REFUSED} == {"C", "ld"}
    assert all((s[1] % 8 != 0) != (ld % 8 != 0) for _, s, ld in R.LAYOUT_REFUSED)


def test_pixsum_tables_hold_every_form():
    forms = {(hw, c): R.pixsum_form(hw, c) for hw in R.PIXSUM_HW for c in R.PIXSUM_C}
    groups = {hw: forms[(hw, 8)]["groups"] for hw in R.PIXSUM_HW}
    assert groups[63] == "some" and groups[64] == "every" and groups[4] == "none" and groups[1] == "none"
    assert forms[(64, 8)]["tail"] == [0, 0, 0, 0] and forms[(65, 8)]["tail"] == [1, 0, 0, 0]      # at and one above a pass
    assert forms[(127, 8)]["unrolled"] == [2, 2, 2, 1] and forms[(127, 8)]["tail"] == [0, 0, 0, 15]
    assert max(forms[(1000, 8)]["unrolled"]) >= 3 and forms[(256, 8)]["unrolled"] == [4] * 4
    assert forms[(1, 8)]["tail"] == [1, 0, 0, 0] and forms[(3, 8)]["tail"] == [1, 1, 1, 0]        # groups with no pixel
    assert {f["blocks"] for f in forms.values()} == {1, 2, 3}
    assert any(f["ragged_c"] and f["blocks"] > 1 for f in forms.values()) and any(not f["ragged_c"] for f in forms.values())
    assert set(R.PIXSUM_LAYOUTS) == {"dense", "slice"} and set(R.PIXSUM_ACCUMULATE) == {False, True}
    assert 1 in R.PIXSUM_B and max(R.PIXSUM_B) > 1


def test_time_path_tables_hold_every_form():
    assert {4, 6, 32, 256, 1024} <= set(R.TIME_DIMS) and {1, 5, 600} <= set(R.TIME_B)
    assert any(B * (d // 2) > 256 and (B * (d // 2)) % 256 for B in R.TIME_B for d in R.TIME_DIMS)
    t = R.time_case(5)
    assert float(t[0]) == 0.0 and float(t[-1]) == 1.0
    forms = {s: R.linear_form(*s) for s in R.LINEAR}
    assert {f["waves"] for f in forms.values()} == {"every", "some", "none"}
    assert any(max(f["passes"]) >= 2 and min(f["passes"]) < max(f["passes"]) for f in forms.values())
    assert any(f["bn_mod4"] for f in forms.values()) and any(not f["bn_mod4"] for f in forms.values())
    assert any(f["k_blocks"] > 1 and f["k_ragged"] for f in forms.values()) and any(f["k_blocks"] >= 16 for f in forms.values())
    assert set(R.LINEAR[:8]) == {(1, 1, 1), (5, 32, 48), (3, 64, 64), (2, 65, 67), (3, 130, 3), (2, 100, 113),
                                 (7, 256, 1024), (1, 1024, 256)}
    assert set(R.LINEAR_BIAS) == {True, False}
    assert set(R.LINEAR_BWD_OPTS) == {(a, b, c) for a in (True, False) for b in (True, False) for c in (True, False)}
    assert {1, 255, 256, 257, 5120} <= set(R.SILU_N)
    assert {0.0, 1e-30, -1e-30, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0} <= set(R.SILU_SPECIALS)


def test_flow_tables_hold_every_form():
    forms = {s: R.cfm_form(*s) for s in R.CFM}
    assert sum(f["strides"] for f in forms.values()) == 1 and forms[R.CFM_STRIDING]["partial_last"]
    assert R.CFM_STRIDING[0] * R.CFM_STRIDING[1] // 4 == 1_048_576 + 224 and R.CFM_STRIDING[1] % 4 == 0
    assert {(B, ps) for B in (1, 3) for ps in (4, 12, 288)} <= set(forms)
    assert {(s, e) for s, e in R.CFM_CASES.values()} == {(0.0, None), (0.0, "nan"), (0.1, "eps")}
    assert all(any(t == [0.0] or 0.0 in t for t in R.cfm_times(B)) and any(1.0 in t for t in R.cfm_times(B)) for B in (1, 3))
    assert {w for w, _, _ in R.CFM_REFUSED} == {"per_sample % 4", "misaligned"}
    m = {c: R.mse_form(c) for c in R.MSE_COUNTS}
    assert sum(f["strides"] for f in m.values()) == 1 and m[R.MSE_STRIDING]["grid"] == R.MSE_CAP
    assert {4, 864, 4096} <= set(m) and set(R.MSE_GRAD_SCALES) == {1.0, 0.25} and set(R.MSE_WANT_DV) == {True, False}
    for c in R.MSE_COUNTS:                                        # the exact tier: integer, non-zero differences
        k = R.mse_case(c, "exact")
        d = (k["v"] - k["u"]).double()
        assert bool((d.abs() >= 1).all()) and bool(torch.equal(d, d.round())) and float((d * d).sum()) < 2 ** 53
    e = {n: R.err_form(n) for n in R.ERR_N}
    assert sum(f["strides"] for f in e.values()) == 1 and e[R.ERR_STRIDING]["grid"] == R.MSE_CAP and {1, 255, 257} <= set(e)
    assert set(R.ERR_TOLS) == {(1e-5, 1e-5), (0.0, 1e-3), (1e-6, 0.0)}
    a = {n: R.axpy_form(n) for n in R.AXPY_N}
    assert sum(f["strides"] for f in a.values()) == 1 and a[R.AXPY_STRIDING]["partial_last"] and {4, 1020} <= set(a)
    assert set(R.AXPY_A) == {1.0, -1.0, 0.5, 1.0 / 3.0, 0.0}
    assert {1, 255, 256, 257, 1000} <= set(R.TICK_N) and len(R.TICK_TABLE) == 5 and len(set(R.TICK_TABLE)) == 5
    f = {n: R.fill_form(n) for n in R.FILL_N}
    assert sum(x["strides"] for x in f.values()) == 1 and {1, 257} <= set(f)


def test_linear_exact_tier_sums_are_fp32_values():
    for B, K, N in R.LINEAR:
        c = R.linear_case(B, K, N, "exact")
        assert float(c["x"].abs().max()) * float(c["w"].abs().max()) * max(K, N) + 8 < 2 ** 24
        assert float(c["dy"].abs().max()) * float(c["x"].abs().max()) * B + 8 < 2 ** 24
