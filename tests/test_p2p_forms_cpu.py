"""What the kernel-level tests of the bf16-only pix2pix forms rest on, checked without a GPU (tests/p2p_forms_ref.py):
the decision-free inputs keep their precondition for every case and seed of the GPU tables, the fp64 reference agrees with
torch's own modules under autograd, and every shape table reaches the launch plan it is listed for -- asked of the
library's host-only queries, which the launchers themselves dispatch on."""
import pytest
import torch

import p2p_forms_ref as R
from conftest import relerr


@pytest.fixture(scope="module")
def L():
    from stain2stain_amd import _native
    return _native.lib()


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def test_inputs_of_every_gpu_case_are_decision_free():
    cases = R.all_instnorm_inputs()
    assert len(cases) == len(R.IN_SINGLE) + len(R.IN_SWITCH) + len(R.IN_MULTI) + len(R.IN_SMALL_AFFINE) + len(R.IN_COND)
    worst = float("inf")
    for B, C, H, W, dtype, seed, offset, scale, affine in cases:
        x = R.decision_free_input(B, C, H, W, dtype, seed, offset, scale)
        assert torch.equal(x, x.to(dtype).double())                            # holds values of the storage dtype
        gamma, beta = R.affine_params(C, seed + 1) if affine else (None, None)
        m = R.min_abs_preactivation(x, gamma, beta)
        assert m >= R.MIN_ABS_Z, (B, C, H, W, dtype, seed, m)
        worst = min(worst, m)
    print(f"smallest |z| over {len(cases)} cases: {worst:.3f}")
    assert worst >= 0.05                                   # |gamma| >= 0.5 on |z| >= 0.17, less |beta| <= 0.05: far from the kink


@pytest.mark.parametrize("n_hw", [(1, 2), (7, 9), (5, 13), (32, 32)])
def test_generator_planes_are_balanced(n_hw):
    H, W = n_hw
    x = R.decision_free_input(3, 8, H, W, torch.float64, 5, offset=0.0, scale=1.0)
    assert float(x.sum((2, 3)).abs().max()) < 1e-12                            # +-pairs and one zero-sum triple
    assert float(x.abs().min()) >= 0.25 and float(x.abs().max()) <= 2.0
    y = R.decision_free_input(3, 8, H, W, torch.float64, 5, offset=8.0, scale=0.5)
    assert relerr(y, x * 0.5 + 8.0) < 1e-15


def test_affine_parameters_have_both_signs():
    for C in (8, 72, 264):
        gamma, beta = R.affine_params(C, C)
        assert bool((gamma > 0).any()) and bool((gamma < 0).any())
        assert float(gamma.abs().min()) >= 0.5 and float(gamma.abs().max()) <= 1.5 and float(beta.abs().max()) <= 0.05
        assert torch.equal(gamma, gamma.float().double())


# ----------------------------------------------------------------------------------------------------------------------
# reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("slope", [0.2, 0.0])
def test_reference_is_torchs_operator_pair_in_fp64(affine, slope):
    """Against nn.InstanceNorm2d + nn.LeakyReLU (and nn.ReLU for the second output) as modules, with the two gradients
    sent through separate backward passes and added."""
    B, C, H, W = 2, 24, 5, 13
    x = R.decision_free_input(B, C, H, W, torch.float32, 3)
    gamma, beta = R.affine_params(C, 4) if affine else (None, None)
    g, g2 = R.cotangent(B, C, H, W, torch.float32, 5), R.cotangent(B, C, H, W, torch.float32, 6)
    ref = R.instnorm_reference(x, gamma, beta, slope, g, g2)
    norm = torch.nn.InstanceNorm2d(C, eps=R.EPS, affine=affine).double()
    if affine:
        norm.load_state_dict({"weight": gamma, "bias": beta})
    xr = x.clone().requires_grad_(True)
    z = norm(xr)
    y, y2 = torch.nn.LeakyReLU(slope)(z), torch.nn.ReLU()(z)
    params = [xr] + (list(norm.parameters()) if affine else [])
    d1 = torch.autograd.grad(y, params, g, retain_graph=True)
    d2 = torch.autograd.grad(y2, params, g2)
    assert relerr(ref["y"], y) < 1e-12 and relerr(ref["y2"], y2) < 1e-12
    assert relerr(ref["dx"], d1[0] + d2[0]) < 1e-12
    if affine:
        assert relerr(ref["dgamma"], d1[1] + d2[1]) < 1e-12 and relerr(ref["dbeta"], d1[2] + d2[2]) < 1e-12
    # the statistics reproduce the pre-activation: z = x * scale + shift
    mean, invstd, scale, shift = ref["stats"]
    assert relerr(x * scale[:, :, None, None] + shift[:, :, None, None], z) < 1e-12
    assert relerr(mean, x.mean((2, 3))) < 1e-12
    assert relerr(invstd * (gamma[None] if affine else 1.0), scale) < 1e-12
    # without a second gradient
    ref1 = R.instnorm_reference(x, gamma, beta, slope, g, None)
    assert relerr(ref1["dx"], d1[0]) < 1e-12


def test_convolution_references_are_adjoint():
    """conv_s2_reference and convT_s2_reference are torch's conv2d / conv_transpose2d in fp64: <conv(x), y> = <x, convT(y)>."""
    x, w, _ = R.conv_operands(2, 8, 6, 12, 16, 1)
    g = torch.Generator().manual_seed(2)
    y = torch.randn(2, 16, 3, 6, generator=g, dtype=torch.float64)
    a = float((R.conv_s2_reference(x, w, None) * y).sum())
    b = float((x * R.convT_s2_reference(y, w, None)).sum())
    assert abs(a - b) < 1e-10 * abs(a)


# ----------------------------------------------------------------------------------------------------------------------
# shape tables against the queries
# ----------------------------------------------------------------------------------------------------------------------
def test_plan_queries_answer_for_bad_arguments(L):
    for f in (L.s2s_conv4x4s2_plan, L.s2s_convt4x4s2_plan):
        for bad in ((0, 4, 4, 64, 8), (1, 0, 4, 64, 8), (1, 4, -1, 64, 8), (1, 4, 4, 0, 8), (1, 4, 4, 64, 0)):
            assert f(*bad) < 0
        assert 0 <= f(2, 16, 16, 64, 64) <= 6


def test_conv_tables_reach_every_plan(L):
    for table, plan_of, split_of in ((R.CONV_FWD_PLANS, L.s2s_conv4x4s2_plan, L.s2s_conv4x4s2_ksplit),
                                     (R.CONV_T_PLANS, L.s2s_convt4x4s2_plan, L.s2s_convt4x4s2_ksplit)):
        assert [r[0] for r in table] == [0, 1, 2, 3, 4, 5, 6]
        for plan, B, H, W, C, Cin in table:
            assert plan_of(B, H, W, C, Cin) == plan, (plan, B, H, W, C, Cin)
            assert (split_of(B, H, W, C, Cin) >= 2) == (plan == 6)              # the flat form always splits; these others do not
            assert B * H * W * C * (4 if table is R.CONV_T_PLANS else 1) < 3_000_000
    for table, plan_of, split_of in ((R.CONV_FWD_SPLIT, L.s2s_conv4x4s2_plan, L.s2s_conv4x4s2_ksplit),
                                     (R.CONV_T_SPLIT, L.s2s_convt4x4s2_plan, L.s2s_convt4x4s2_ksplit)):
        for plan, min_split, B, H, W, C, Cin in table:
            assert plan_of(B, H, W, C, Cin) == plan and plan < 6 and split_of(B, H, W, C, Cin) >= min_split >= 2
    for _, _, _, _, C, Cin in R.CONV_FWD_PLANS:
        assert Cin >= 8 and Cin & (Cin - 1) == 0 and C % 8 == 0                # what s2s_conv4x4s2_nhwc accepts
    for _, _, _, _, C, Cin in R.CONV_T_PLANS:
        assert Cin % 8 == 0 and C % 64 == 0                                    # what s2s_convt4x4s2_nhwc accepts


def test_split_tables_split_and_fit_the_single_launch_norm(L):
    rows = R.SPLIT_FWD + R.SPLIT_T
    for kind, plan, min_split, B, H, W, C, Cin in rows:
        T = kind == "convT"
        plan_of, split_of = (L.s2s_convt4x4s2_plan, L.s2s_convt4x4s2_ksplit) if T else (L.s2s_conv4x4s2_plan, L.s2s_conv4x4s2_ksplit)
        assert plan_of(B, H, W, C, Cin) == plan
        assert split_of(B, H, W, C, Cin) >= max(2, min_split)
        assert L.s2s_instnorm_split_ok(0, 2 * H if T else H, 2 * W if T else W, C) == 1
    for table in (R.SPLIT_FWD, R.SPLIT_T):
        flat = [r for r in table if r[1] == 6]
        assert any(r[6] <= 64 for r in flat) and any(r[6] > 64 for r in flat)          # the flat form at both widths
        assert any(r[1] == 5 for r in table) and any(r[1] in (1, 3) for r in table)    # non-flat split-K, narrow and wide
        assert any(r[2] >= 3 for r in table)                                           # a split of three or more
    assert any(r[6] % 64 for r in R.SPLIT_FWD)                                         # a tail in the 64-channel workgroup
    assert L.s2s_instnorm_split_ok(0, 32, 33, 64) == 0 and L.s2s_instnorm_split_ok(1, 8, 8, 64) == 0


def test_instnorm_tables_cover_what_they_claim(L):
    hw = {2, 63, 64, 65, 1023, 1024}
    cs = {8, 24, 64, 72, 264}
    groups = {"bf16 <true,false>": [r for r in R.IN_SINGLE if r[0] == R.BF16 and not r[6]],
              "bf16 <true,true>": [r for r in R.IN_SINGLE if r[0] == R.BF16 and r[6]],
              "fp32": [r for r in R.IN_SINGLE if r[0] == R.F32]}
    for name, rows in groups.items():
        assert {r[3] * r[4] for r in rows} == hw, name
        assert {r[2] for r in rows} == cs, name
        assert {r[5] for r in rows} == {False, True} and {r[7] for r in rows} == {0.2, 0.0}, name
    assert {r[6] for r in groups["fp32"]} == {False, True}
    assert len(R.IN_SINGLE) <= 40
    assert all(r[3] * r[4] == 1025 for r in R.IN_SWITCH) and {r[0] for r in R.IN_SWITCH} == {R.BF16, R.F32}
    for dtype, B, C, H, W, affine, with_y2, with_g2, slope in R.IN_MULTI:
        nb, lanes = L.s2s_instnorm_blocks(B, H, W, C), 256 // R.in_pcb(C)
        assert nb > 1 and nb * lanes < H * W and (H * W) % (nb * lanes) != 0
    assert any(r[5] for r in R.IN_MULTI) and any(not r[5] for r in R.IN_MULTI)
    assert {(r[6], r[7]) for r in R.IN_MULTI} >= {(False, False), (True, True)}
    assert all(r[3] * r[4] <= 1024 for r in R.IN_SMALL_AFFINE)
    assert any(r[3] * r[4] <= 1024 for r in R.IN_COND) and any(r[3] * r[4] > 1024 for r in R.IN_COND)


def test_wgrad_tables_reach_their_kernels(L):
    for name, ks, plain, B, H, W, C, Cout in R.WGRAD:
        cin = 4 * C if ks == 2 else C
        S, tiles = L.s2s_convkxk_wgrad_splits(0, B, H, W, cin, Cout, ks), R.wgrad_tiles(B, H, W)
        assert 1 <= S <= tiles
        flat_map = plain and H <= 8 and W <= 8 and H & (H - 1) == 0 and W & (W - 1) == 0
        small = flat_map and (B * H * W + 127) // 128 <= 8 and C % 16 == 0
        assert flat_map == name.startswith(("flat", "small")) and small == name.startswith("small")
        if name in R.WGRAD_UNEVEN:
            assert (S, tiles) == R.WGRAD_UNEVEN[name] and tiles % S and -(-tiles // S) >= 3
        if name in R.WGRAD_FOLD4:
            assert S == R.WGRAD_FOLD4[name] and S >= 16 and -(-C // 64) * Cout <= 1024
        if plain:
            assert C & (C - 1) == 0
    tiles_small = {(B * H * W + 127) // 128 for n, _, _, B, H, W, _, _ in R.WGRAD if n.startswith("small")}
    assert 1 in tiles_small and max(tiles_small) > 1
    assert {r[1] for r in R.WGRAD} == {2, 4} and {r[0] for r in R.WGRAD_LAYOUT0} == {2, 4}


def test_convsm_tables_are_taken_by_the_kernel(L):
    for B, ho, cin, cout, slope in R.CONVSM_FWD:
        assert L.s2s_convsm_ok(0, 1, B, ho, ho, cin, cout) > 0
    for B, hi, cin, cout in R.CONVSM_T:
        assert L.s2s_convsm_ok(0, 2, B, hi, hi, cin, cout) > 0
    assert any(r[3] % 64 not in (0, 16, 32, 48) or r[3] > 64 and r[3] % 64 for r in R.CONVSM_FWD)      # a channel tail
