"""The tables of tests/conv3x3_forms_ref.py against the library's plan query (s2s_conv3x3_plan: host code, no GPU): every
row still gets the launch plan it was written for -- with no switch set in this process, under a row's own switch or
under S2S_CONV_PERS=2 S2S_CONV_STAGE=0 in a child process (the switches are read once per process) -- and the tables as
a whole still contain every form the 3x3 forward / data-gradient kernels have.  A retuning of select_cfg, stage_grid,
pers_eligible, split_count or xcd_cut that moves a row out of its form fails here, so that
tests/test_conv3x3_forms_gpu.py cannot quietly stop covering it.

Also here: the preconditions of the exact operand tier, from the reference alone; the float64 references against autograd;
and the reachability claims the tables rest on, by a search through the query."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import conv3x3_forms_ref as R

BF, F32 = torch.bfloat16, torch.float32
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
SWITCHES = ("S2S_CONV_STAGE", "S2S_CONV_PERS", "S2S_CONV_XCD", "S2S_CONV_DBG")


def query(name):
    from stain2stain_amd import ops
    B, H, W, c0, c1, cout = R.row(name)[0]
    return ops.conv3x3_plan(R.row_dtype(name), B, H, W, c0, c1, cout, **R.plan_query_args(name))


def plans_of(names):
    return {n: list(query(n).values()) for n in names}


# the shapes of the reachability search: maps around every tile size, batches up to the persistent threshold, and Cout
# through the Cout % 128 sliver (576 = 4 * 128 + 64, 520, 1088) as well as the ordinary widths
SEARCH_B = (1, 2, 3, 7, 16, 45, 50, 100, 150, 300, 600, 1500)
SEARCH_HW = ((4, 8), (4, 33), (8, 8), (8, 16), (8, 17), (8, 32), (9, 8), (9, 33), (16, 16), (17, 33), (32, 32), (64, 64))
SEARCH_COUT = (8, 64, 72, 128, 136, 192, 256, 512, 520, 576, 640, 1088)
SEARCH_CIN = ((32, 8), (64, 0), (96, 0))


def pers_search():
    """{cfg: [rows on the persistent kernel, largest tile count, smallest gy]} over the search grid, statistics launches of
    the preferred layout and plain ones, under whatever switches this process has."""
    from stain2stain_amd import ops
    out = {}
    for B in SEARCH_B:
        for H, W in SEARCH_HW:
            for cout in SEARCH_COUT:
                for c0, c1 in SEARCH_CIN:
                    if 1.0 * B * H * W * max(c0, cout) * 2 >= 1e9:
                        continue
                    for stats in (False, True):
                        p = ops.conv3x3_plan(BF, B, H, W, c0, c1, cout, stats=stats)
                        if p["family"] in (R.PERS, R.PERS_CARRY):
                            e = out.setdefault(str(p["cfg"]), [0, 0, 1 << 30])
                            e[0] += 1
                            e[1] = max(e[1], p["gx"] * p["gy"])
                            e[2] = min(e[2], p["gy"])
    return out


def _child(env, names):
    code = ("import json, sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import test_conv3x3_forms_cpu as t; "
            "print(json.dumps({'plans': t.plans_of(sys.argv[3].split(',')), 'search': t.pers_search()}))")
    clean = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    run = subprocess.run([sys.executable, "-c", code, ROOT, TESTS, ",".join(names)], env={**clean, **env},
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout.strip().splitlines()[-1])


def _no_switch():
    return not any(os.environ.get(k) for k in SWITCHES)


@pytest.mark.parametrize("name", list(R.CASES))
def test_conv3x3_forms_row_has_its_plan(name):
    assert _no_switch(), "the table holds the plans with no launch switch set"
    shape, flags, _, plan = R.row(name)
    got = query(name)
    assert tuple(got.values()) == tuple(plan), (got, plan)
    B, H, W, c0, c1, cout = shape
    assert c0 % 8 == 0 and c1 % 8 == 0 and cout % 8 == 0 and R.flop(name) <= R.MAX_FLOP
    # the plan against the queries a caller sizes its buffers with
    from stain2stain_amd import ops
    L = ops._L()
    dt = 1 if "f32" in flags else 0
    if "stats" in flags and "affine" not in flags and "kwork" not in flags:
        rows = L.s2s_conv3x3_stat_blocks(dt, B, H, W, cout) if "rows0" in flags else \
            L.s2s_conv3x3_stat_rows(dt, B, H, W, cout, c0, c1, c0, max(c1, 8), int("bias" in flags or "relu" in flags))
        assert rows == got["stat_rows"]
    if "kwork" in flags:
        assert L.s2s_conv3x3_ksplit(dt, B, H, W, cout, c0 + c1) == got["ksplit"] > 1
    fam = L.s2s_conv3x3_family(dt, B, H, W, cout, c0, c1, c0, max(c1, 8), cout, int(R.plan_query_args(name)["bias"]),
                               int("affine" in flags), int("stats" in flags),
                               (0 if "rows0" in flags else -1) if "stats" in flags else 0, int("kwork" in flags))
    assert fam == got["family"]


def test_conv3x3_forms_switch_rows_have_their_plans():
    """The rows that name a switch, and the persistent table, each in a child process under its switches; in the same
    children, what the persistent table rests on: with S2S_CONV_PERS=2 the cfg 2 and cfg 6 launches never carry statistics
    (gy >= 5) and never walk (at most 512 tiles)."""
    envs = []
    for name in R.SWITCH_CASES:
        if R.row(name)[2] not in envs:
            envs.append(R.row(name)[2])
    envs.append(R.PERS_ENV)
    for env in envs:
        names = [n for n in list(R.SWITCH_CASES) + list(R.PERS_CASES) if R.row(n)[2] == env]
        got = _child(env, names)
        bad = [(n, got["plans"][n], list(R.row(n)[3])) for n in names if got["plans"][n] != list(R.row(n)[3])]
        assert not bad, (env, bad)
        if env == R.PERS_ENV:
            s = got["search"]
            assert set(s) == {"1", "2", "3", "5", "6", "7"}, s
            for cfg in ("2", "6"):
                assert s[cfg][1] <= 512 and s[cfg][2] >= 5, (cfg, s[cfg])
            for cfg in ("1", "3", "5", "7"):
                assert s[cfg][1] > 512 and s[cfg][2] == 1, (cfg, s[cfg])


def test_conv3x3_no_default_launch_reaches_the_persistent_kernel_on_cfg_2_3_6_7():
    """With no switch set the 1024-tile threshold is met by cfgs 1 and 5 alone (the cfgs behind them in the selection order
    have at most twice the tiles of one that already failed the 448 test), so twelve persistent instantiations run only
    under S2S_CONV_PERS=<threshold>.  Were the search to find such a shape, it belongs into CASES as a default row."""
    assert _no_switch()
    s = pers_search()
    assert set(s) == {"1", "5"}, s
    assert s["1"][0] > 10 and s["5"][0] > 10


def _keys(table):
    """(family, cfg, statistics form, (xsp, xsn), ksplit) of every row of a table."""
    out = {}
    for name in table:
        _, flags, _, plan = R.row(name)
        p = dict(zip(R.FIELDS, plan))
        out[name] = (p["family"], p["cfg"], R.stats_form(p, flags), (p["xsp"], p["xsn"]), p["ksplit"])
    return out


def test_conv3x3_forms_tables_contain_every_form():
    D, S, P = _keys(R.CASES), _keys(R.SWITCH_CASES), _keys(R.PERS_CASES)
    flags = {n: R.row(n)[1] for n in list(R.CASES) + list(R.SWITCH_CASES) + list(R.PERS_CASES)}
    shape = {n: R.row(n)[0] for n in flags}
    missing = []

    def need(table, what, pred):
        if not [n for n in table if pred(n, table[n])]:
            missing.append(what)

    # staged kernel
    for form in ("carried", "none"):
        need(D, f"staged resident, statistics {form}, XCD order", lambda n, k: k[0] == 0 and k[2] == form and k[3][0] == 8 and "affine" not in flags[n])
        need(D, f"staged resident, statistics {form}, plain order", lambda n, k: k[0] == 0 and k[2] == form and k[3][0] == 0 and "affine" not in flags[n])
        need(D, f"staged streaming, gy 1, statistics {form}", lambda n, k: k[0] == 1 and k[2] == form and "affine" not in flags[n])
        need(S, f"staged streaming, gy > 1, statistics {form}", lambda n, k: k[0] == 1 and k[2] == form and R.row(n)[3][3] > 1)
    need(D, "staged resident, gy 8 and gx < 256", lambda n, k: k[0] == 0 and R.row(n)[3][3] == 8 and R.row(n)[3][2] < 256 and k[2] == "carried")
    need(D, "staged resident, two sources with a partial second chunk", lambda n, k: k[0] == 0 and shape[n][4] % 32 and shape[n][3] % 32 == 0 and shape[n][4])
    need(D, "staged resident, affine", lambda n, k: k[0] == 0 and "affine" in flags[n])
    need(D, "staged streaming, affine", lambda n, k: k[0] == 1 and "affine" in flags[n])
    # persistent kernel with no switch set: cfgs 1 and 5, per-tile statistics and none; carried under S2S_CONV_STAGE=0
    for cfg in (1, 5):
        for form in ("tile", "none"):
            need(D, f"persistent cfg {cfg}, statistics {form}", lambda n, k: k[0] == R.PERS and k[1] == cfg and k[2] == form)
    need(D, "persistent, a walk of three tiles", lambda n, k: k[0] == R.PERS and R.row(n)[3][2] * R.row(n)[3][3] > 2 * R.row(n)[3][4])
    need(D, "persistent, per-tile rows asked of a single channel tile", lambda n, k: k[0] == R.PERS and "rows0" in flags[n] and R.row(n)[3][3] == 1)
    need(S, "persistent, carried statistics", lambda n, k: k[0] == R.PERS_CARRY and k[2] == "carried")
    # per-tap kernel: every tile with bias, per-tile statistics and affine; every XCD cut; the split counts
    for cfg in range(8):
        need(D, f"tap cfg {cfg}, bias + statistics", lambda n, k: k[:3] == (R.TAP, cfg, "tile") and "bias" in flags[n] and k[4] == 1)
        need(D, f"tap cfg {cfg}, bias + affine + relu", lambda n, k: k[:2] == (R.TAP, cfg) and {"bias", "affine", "relu"} <= set(flags[n]) and k[4] == 1)
    for cut in ((8, 1), (4, 2), (2, 4), (1, 8), (0, 1)):
        need(D, f"tap, XCD cut {cut}", lambda n, k: k[0] == R.TAP and k[3] == cut and k[4] == 1)
    for ks in (2, 3, 4, 8, 16):
        need(D, f"tap, {ks} splits", lambda n, k: k[0] == R.TAP and k[4] == ks)
    nchunk = {n: -(-(shape[n][3] + shape[n][4]) // 32) for n in D}
    if len([n for n in D if D[n][4] > 1 and nchunk[n] % D[n][4]]) < 2:
        missing.append("two split rows with nchunk % ksplit != 0")
    need(D, "split, two sources with c0 % 32 != 0", lambda n, k: k[4] > 1 and shape[n][4] and shape[n][3] % 32)
    need(D, "split with bias", lambda n, k: k[4] > 1 and "bias" in flags[n])
    need(D, "split with affine + relu", lambda n, k: k[4] > 1 and {"affine", "relu"} <= set(flags[n]))
    # relu without an affine: plain, statistics, split, and in fp32
    need(D, "relu alone, plain", lambda n, k: "relu" in flags[n] and "affine" not in flags[n] and k[2] == "none" and k[4] == 1 and k[0] == R.TAP)
    need(D, "relu alone, statistics", lambda n, k: "relu" in flags[n] and "affine" not in flags[n] and k[2] == "tile" and k[0] == R.TAP)
    need(D, "relu alone, split", lambda n, k: "relu" in flags[n] and "affine" not in flags[n] and k[4] > 1)
    need(D, "relu alone, fp32", lambda n, k: "relu" in flags[n] and "affine" not in flags[n] and k[0] == R.SPLIT_F32)
    # fp32
    for cfg in (0, 1):
        need(D, f"fp32 cfg {cfg}, statistics", lambda n, k: k[:2] == (R.SPLIT_F32, cfg) and "stats" in flags[n])
        need(D, f"fp32 cfg {cfg}, bias + affine + relu", lambda n, k: k[:2] == (R.SPLIT_F32, cfg) and {"bias", "affine", "relu"} <= set(flags[n]))
    need(D, "fp32, two sources with a straddling chunk", lambda n, k: k[0] == R.SPLIT_F32 and shape[n][4] and shape[n][3] % 32)
    # data gradients
    for fam in (0, 1, R.PERS, R.TAP, R.SPLIT_F32):
        need(D, f"a data gradient on family {fam}", lambda n, k: k[0] == fam and "dgrad" in flags[n])
    # edges
    need(D, "one pixel", lambda n, k: shape[n][:3] == (1, 1, 1) and shape[n][3:] == (8, 0, 8))
    need(D, "one row", lambda n, k: shape[n][1] == 1 and shape[n][2] > 32)
    need(D, "one column", lambda n, k: shape[n][2] == 1 and shape[n][1] > 16)
    for h in (3, 5, 7, 9, 15, 17):
        need(D, f"H = {h}", lambda n, k: shape[n][1] == h)
    for w in (15, 17, 31, 33):
        need(D, f"W = {w}", lambda n, k: shape[n][2] == w)
    for cout in (8, 72):
        need(D, f"Cout = {cout}", lambda n, k: shape[n][5] == cout and k[0] == R.TAP)
    for cin in (8, 40):
        need(D, f"cin = {cin}", lambda n, k: shape[n][3] + shape[n][4] == cin and k[0] == R.TAP)
    # the persistent table: cfgs 1, 3, 5, 7 with STATS 0 / 1 / 2, one tile per workgroup and a walk; cfgs 2, 6 with STATS 0 / 1
    for cfg in (1, 2, 3, 5, 6, 7):
        for form, fam in (("none", R.PERS), ("tile", R.PERS), ("carried", R.PERS_CARRY)):
            if form == "carried" and cfg in (2, 6):
                continue                                      # gy >= 5 there (test_conv3x3_forms_switch_rows_have_their_plans)
            need(P, f"S2S_CONV_PERS=2: cfg {cfg}, statistics {form}, one tile per workgroup",
                 lambda n, k: k[:3] == (fam, cfg, form) and R.row(n)[3][2] * R.row(n)[3][3] == R.row(n)[3][4]
                 and (form != "tile" or R.row(n)[3][3] > 1))
            if cfg not in (2, 6):                             # at most 512 tiles there (same test)
                need(P, f"S2S_CONV_PERS=2: cfg {cfg}, statistics {form}, more than 512 tiles",
                     lambda n, k: k[:3] == (fam, cfg, form) and R.row(n)[3][2] * R.row(n)[3][3] > 512
                     and (form != "tile" or R.row(n)[3][3] > 1))
    assert not missing, "the tables lack: " + "; ".join(missing)


ALL_ROWS = list(R.CASES) + list(R.SWITCH_CASES) + list(R.PERS_CASES)
_TIES = []


@pytest.mark.parametrize("name", ALL_ROWS)
def test_conv3x3_forms_exact_tier_preconditions(name):
    """Every product and partial sum of the exact tier is an integer (or, behind a scale of 1/2, a half) below 2^24 in any
    order: conv(|x|, |w|) + |b| < 2^24 per element (times |scale|, plus |shift|, behind an affine, with one bit to spare
    for the half); in a statistics row the sum of the squared stored values of a channel stays below 2^24."""
    _, flags, _, _ = R.row(name)
    dtype = R.row_dtype(name)
    c = R.case(name, dtype, "exact")
    for t in (c["x"], c["w"], c["b"], c["sh"]):
        assert t is None or bool((t == t.round()).all())
    assert c["sc"] is None or set(c["sc"].tolist()) <= {0.5, 1.0, 2.0, -1.0}
    assert bool((c["x"].abs() <= 1).all()) and bool((c["w"].abs() <= 1).all())
    assert float(c["mag"].max()) < 2.0 ** 23
    assert bool((c["pre"] * 2 == (c["pre"] * 2).round()).all())
    assert torch.equal(c["pre"].float().double(), c["pre"])
    st = R.stored(c["ref"], dtype)
    if "stats" in flags:
        assert "affine" not in flags
        s1, s2 = R.stat_sums(st)
        assert float(s2.max()) < 2.0 ** 24, float(s2.max())
        assert float(st.double().abs().sum((0, 2, 3)).max()) < 2.0 ** 24
        assert float(s2.max()) > 0
    elif dtype == BF and "affine" not in flags:
        v = c["ref"]
        ties = int(((v.abs() > 256) & (v.abs() < 512) & (v.abs() % 2 == 1)).sum())
        if ties:
            _TIES.append((name, ties))
            # the reference's rounding at a tie is to even: the stored value is a multiple of 4 there
            tie = (v.abs() > 256) & (v.abs() < 512) & (v.abs() % 2 == 1)
            assert bool((st.double()[tie] % 4 == 0).all())


def test_conv3x3_forms_exact_tier_has_a_bf16_tie():
    """Runs after the parametrised test above (same module, definition order): some bf16 row without statistics holds an
    element whose exact value is an odd integer between 256 and 512, so the rounding mode is tested and not assumed."""
    if not _TIES:                                             # (run alone: look at the deep rows)
        for name in ("split16", "split8", "split4"):
            test_conv3x3_forms_exact_tier_preconditions(name)
    assert _TIES, "no bf16 tie in any row"


@pytest.mark.parametrize("name", ["tap3_affine", "f32_dgrad", "hw_7x31", "split16_dgrad"])
def test_conv3x3_forms_reference_against_autograd(name):
    """The float64 reference of a forward row is the adjoint of conv_transpose2d with the same weight, that of a data-gradient
    row the gradient of conv2d with the forward weight [c0 + c1, Cout, 3, 3] -- which is the packing
    ops.pack_conv3x3(w)[1] is made for (the GPU test runs it)."""
    shape, flags, _, _ = R.row(name)
    B, H, W, c0, c1, cout = shape
    c = R.case(name, R.row_dtype(name), "real")
    x, w = c["x"].double(), c["wr"].double()
    z = torch.zeros(B, cout, H, W, dtype=torch.float64, requires_grad=True)
    if "dgrad" in flags:
        assert w.shape == (c0 + c1, cout, 3, 3)
        (F.conv2d(z, w, None, padding=1) * x).sum().backward()
    else:
        assert w.shape == (cout, c0 + c1, 3, 3)
        (F.conv_transpose2d(z, w, None, padding=1) * x).sum().backward()
    acc = z.grad
    if c["b"] is not None:
        acc = acc + c["b"].double().reshape(1, cout, 1, 1)
    if c["sc"] is not None:
        acc = acc * c["sc"].double().reshape(1, cout, 1, 1) + c["sh"].double().reshape(1, cout, 1, 1)
    assert float((acc - c["pre"]).abs().max()) <= 1e-12 * float(c["pre"].abs().max())
    want = acc.clamp_min(0) if "relu" in flags else acc
    assert float((want - c["ref"]).abs().max()) <= 1e-12 * float(c["ref"].abs().max())
    assert c["yard"][0] >= R.YARD_FLOOR and c["yard"][2] >= R.YARD_FLOOR


def test_conv3x3_plan_refuses_what_the_launch_refuses():
    import ctypes
    from stain2stain_amd import _native
    L = _native.lib()
    out = (ctypes.c_int * 9)()
    p = ctypes.cast(out, ctypes.c_void_p)
    assert L.s2s_conv3x3_plan(0, 1, 8, 8, 8, 8, 0, 8, 8, 8, 0, 0, 0, 0, 0, None) == -5
    assert L.s2s_conv3x3_plan(0, 0, 8, 8, 8, 8, 0, 8, 8, 8, 0, 0, 0, 0, 0, p) == -1
    assert L.s2s_conv3x3_plan(7, 1, 8, 8, 8, 8, 0, 8, 8, 8, 0, 0, 0, 0, 0, p) == -3
    # a statistics layout no kernel writes: refused by the plan as by the launch
    assert L.s2s_conv3x3_plan(0, 1, 8, 8, 8, 8, 0, 8, 8, 8, 0, 0, 1, 7, 0, p) == -1
    assert L.s2s_conv3x3_plan(0, 1, 8, 8, 8, 8, 0, 8, 8, 8, 0, 0, 1, -1, 0, p) == 0 and list(out)[0] == R.TAP
