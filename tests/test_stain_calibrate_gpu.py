"""The stain-calibration kernels (csrc/stain_calibrate.hip) against the numpy / Python-integer restatement of
tests/stain_calibrate_ref.py, on poisoned memory (every ``torch.empty`` and every ``ops._workspace`` slab starts as NaN /
0xFF, as in tests/test_stain_quant_gpu.py).

Tolerances.  Histograms, tissue counts, suffix sums, bins and valid flags are integers; thresholds are
bin / 1024 and the Dice curves and burdens one double quotient of exact integers, which the restatement forms with the
same operations: everything is compared for equality.  The only exceptions are the cross-checks against the fp32 Dice and
IoU of ``stain_agreement``: one fp32 rounding of the same double quotient, 2^-23 relative (the bound of 3.17)."""
import numpy as np
import pytest
import torch

import stain_calibrate_ref as C
import stain_quant_ref as R
from stain2stain_amd import (calibrate_thresholds, match_thresholds, region_stain_histogram,
                             region_stain_pair_histogram, stain_agreement, stain_histogram, stain_pair_histogram,
                             stain_quantify, stain_thresholds, thresholds_tuple)
from stain2stain_amd.stain_quant import unmix_matrix

pytestmark = pytest.mark.gpu
DEV = "cuda"
NB = 4096
F32 = 2.0 ** -23
QS = (0.05, 0.5)
JT = 205                                           # 0.2001953125 OD: the grid point next to the conventional 0.2


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    from stain2stain_amd import ops
    import torch.utils.deterministic as tud
    prev_det, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    prev_fill = tud.fill_uninitialized_memory
    orig = ops._workspace

    def poisoned(device, numel, tag):
        buf = orig(device, numel, tag)
        buf.view(torch.uint8).fill_(255)
        return buf

    torch.use_deterministic_algorithms(True, warn_only=True)
    tud.fill_uninitialized_memory = True
    try:
        for buf in ops._WORKSPACE.values():
            buf.view(torch.uint8).fill_(255)
        monkeypatch.setattr(ops, "_workspace", poisoned)
        yield
    finally:
        torch.use_deterministic_algorithms(prev_det, warn_only=prev_warn)
        tud.fill_uninitialized_memory = prev_fill


def _stained(B, H, W, seed, plaque=0.08):
    """uint8 [B, H, W, 3]: haematoxylin background with DAB blobs, glass patches, black specks and noise."""
    rng = np.random.default_rng(seed)
    conc = np.zeros((B, H, W, 3))
    conc[..., 0] = rng.uniform(0.05, 0.5, size=(B, H, W))
    conc[..., 1] = np.where(rng.random((B, H, W)) < plaque, rng.uniform(0.1, 1.2, size=(B, H, W)), 0.02)
    img = R.synthesise(conc, "hdab").astype(np.int32) + rng.integers(-3, 4, size=(B, H, W, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    glass = rng.random((B, H, W)) < 0.2
    img[glass] = rng.integers(225, 256, size=(int(glass.sum()), 3), dtype=np.uint8)
    img[rng.random((B, H, W)) < 0.01] = 0
    return img


def _pair(B, H, W, seed):
    a, b = _stained(B, H, W, seed), _stained(B, H, W, seed + 1000, plaque=0.12)
    b[:, : H // 2] = a[:, : H // 2]                                        # the masks overlap
    return a, b


def _network(u8, seed):
    """uint8 [B, H, W, 3] -> fp32 [B, 3, H, W] in the network's range with a sub-level jitter (the quantiser has work)."""
    rng = np.random.default_rng(seed)
    lv = u8.astype(np.float64).transpose(0, 3, 1, 2) + rng.random(u8.transpose(0, 3, 1, 2).shape) * 0.98
    return np.ascontiguousarray((lv / 127.5 - 1.0).astype(np.float32))


def _crop_view(u8):
    """The batch as a crop view of a larger GPU array: odd row pitch, unaligned base."""
    B, H, W, _ = u8.shape
    big = torch.full((B, H + 5, W + 6, 3), 77, dtype=torch.uint8, device=DEV)
    view = big[:, 2:2 + H, 3:3 + W]
    view.copy_(torch.from_numpy(u8))
    assert (3 * (W + 6)) % 4 != 0 or view.data_ptr() % 4 != 0 or W % 4 != 0
    return view


def _m32():
    return unmix_matrix("hdab").numpy()


def _same(got, want, what):
    """Equality of a device tensor and the restatement's array, dtype included."""
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), what


def _check_hist(h, ref_hist, ref_tissue, what):
    _same(h["hist"], ref_hist, what + " hist")
    _same(h["tissue"], ref_tissue, what + " tissue")


def _check_rules(t, ref_hist, coarse, what):
    ref = C.thresholds(ref_hist, coarse, QS)
    for k, v in ref.items():
        _same(t[k], v, f"{what} {k}")


def _check_match(m, ref_hist, jt, what):
    refs = [C.match(ref_hist[o], jt) for o in range(ref_hist.shape[0])]
    assert sorted(m) == sorted(refs[0]), what
    for k in refs[0]:
        want = np.stack([np.asarray(r[k]) for r in refs])
        if k.endswith("_bin") or k.endswith("_valid"):
            want = want.astype(np.int32)
        _same(m[k], want, f"{what} {k}")


def _inputs(kind, B, H, W, crop, seed):
    """(GPU pair, the uint8 bytes the kernels see)."""
    a, b = _pair(B, H, W, seed)
    if kind == "f32":
        xa, xb = _network(a, 1), _network(b, 2)
        xa.reshape(-1)[:: 7] += 3.0                                        # out of range: the clamp has work
        xb.reshape(-1)[:: 11] -= 3.0
        return (torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)), (R.nchw_to_u8(xa), R.nchw_to_u8(xb))
    if crop:
        return (_crop_view(a), _crop_view(b)), (a, b)
    return (torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)), (a, b)


CASES = [("u8", 1, 1, 1, False), ("u8", 2, 37, 53, True), ("u8", 2, 64, 64, False), ("u8", 3, 256, 256, False),
         ("f32", 2, 37, 53, False), ("f32", 2, 64, 64, False)]


# ---- 1. parity with the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,H,W,crop", CASES)
def test_parity_single(kind, B, H, W, crop):
    m32 = _m32()
    (ga, _), (a, _) = _inputs(kind, B, H, W, crop, 100 + H)
    what = f"{kind} {B}x{H}x{W}"
    for pool in (False, True):
        ref_hist, ref_tissue = C.histogram(a, m32, pool=pool)
        h = stain_histogram(ga, pool=pool)
        _check_hist(h, ref_hist, ref_tissue, f"{what} pool {pool}")
        assert torch.equal(h["hist"].sum(-1), h["tissue"][:, None].expand(-1, 3))
        _check_rules(stain_thresholds(h, coarse=16, quantiles=QS), ref_hist, 16, f"{what} pool {pool}")
    ref_hist, ref_tissue = C.histogram(a, m32, 256, 40)
    _check_hist(stain_histogram(ga, white=256, black=40), ref_hist, ref_tissue, what + " white 256 black 40")
    t = calibrate_thresholds(ga, quantiles=QS)
    assert torch.equal(t["hist"], stain_histogram(ga)["hist"])
    _check_rules(t, C.histogram(a, m32)[0], 16, what + " calibrate")


@pytest.mark.parametrize("coarse", [1, 4, 512, 4096])
def test_parity_triangle_groupings(coarse):
    a = _stained(2, 64, 64, 164)
    h = stain_histogram(torch.from_numpy(a).to(DEV))
    _check_rules(stain_thresholds(h, coarse=coarse, quantiles=QS), C.histogram(a, _m32())[0], coarse, f"coarse {coarse}")


def test_other_basis():
    a = _stained(2, 40, 44, 7)
    ref_hist, ref_tissue = C.histogram(a, unmix_matrix("hed").numpy())
    h = stain_histogram(torch.from_numpy(a).to(DEV), stains="hed")
    _check_hist(h, ref_hist, ref_tissue, "hed")
    _check_rules(stain_thresholds(h, quantiles=QS), ref_hist, 16, "hed")


@pytest.mark.parametrize("kind,B,H,W,crop", CASES)
def test_parity_paired(kind, B, H, W, crop):
    m32 = _m32()
    (ga, gb), (a, b) = _inputs(kind, B, H, W, crop, 200 + H)
    what = f"{kind} pair {B}x{H}x{W}"
    for jt, stain, pool in ((JT, 1, False), (0, 1, False), (52, 0, False), (JT, 1, True)):
        ref_hist, ref_tissue = C.pair_histogram(a, b, m32, stain, jt, pool=pool)
        p = stain_pair_histogram(ga, gb, stain=stain, target_threshold=jt / 1024 if jt else None, pool=pool)
        _same(p["hist"], ref_hist, f"{what} jt {jt} hist")
        _same(p["tissue_pred"], ref_tissue[:, 0], what)
        _same(p["tissue_target"], ref_tissue[:, 1], what)
        assert p["target_bin"] == jt and p["stain"] == stain
        m = match_thresholds(p)
        assert ("best_dice" in m) == bool(jt)
        _check_match(m, ref_hist, jt, f"{what} jt {jt} stain {stain} pool {pool}")


# ---- 2. special images ------------------------------------------------------------------------------------------------
def _no_nan(d):
    for k, v in d.items():
        if isinstance(v, torch.Tensor) and v.is_floating_point():
            assert not torch.isnan(v).any(), k


def test_special_images():
    m32 = _m32()
    glass = torch.full((2, 33, 47, 3), 255, dtype=torch.uint8, device=DEV)
    t = calibrate_thresholds(glass, quantiles=QS)
    assert (t["tissue"] == 0).all() and (t["hist"] == 0).all() and (t["positive"] == 0).all()
    for k in ("otsu", "triangle", "quantile"):
        assert (t[k + "_valid"] == 0).all(), k
    _no_nan(t)
    _check_rules(t, np.zeros((2, 3, NB), np.int64), 16, "glass")
    m = match_thresholds(stain_pair_histogram(glass, glass.clone(), target_threshold=JT / 1024))
    assert (m["match_burden_valid"] == 0).all() and (m["best_dice_valid"] == 0).all()
    assert (m["dice_common"] == 1).all() and (m["dice_cond"] == 1).all() and (m["dice_at_best"] == 1).all()
    _no_nan(m)
    # one flat tissue colour: a single occupied bin per stain, nothing for Otsu or the triangle to separate
    colour = R.synthesise([0.3, 0.4, 0.0], "hdab")
    flat = np.broadcast_to(colour, (1, 20, 24, 3)).copy()
    t = calibrate_thresholds(torch.from_numpy(flat).to(DEV), quantiles=QS)
    assert int(t["tissue"][0]) == 480 and ((t["hist"] > 0).sum(-1) == 1).all() and (t["hist"].amax(-1) == 480).all()
    assert (t["otsu_valid"] == 0).all() and (t["triangle_valid"] == 0).all() and (t["otsu_bin"] == 0).all()
    occupied = t["hist"].argmax(-1)
    assert (t["quantile_valid"] == 1).all() and torch.equal(t["quantile_bin"][..., 0].long(), (occupied + 1).clamp_min(1))
    _check_rules(t, C.histogram(flat, m32)[0], 16, "flat")
    _no_nan(t)
    # all-black bytes with black = 0 are tissue (u = 0 takes the table entry of u = 1); black = 1 drops them
    zero = np.zeros((1, 33, 47, 3), np.uint8)
    gz = torch.from_numpy(zero).to(DEV)
    h = stain_histogram(gz)
    _check_hist(h, *C.histogram(zero, m32), "zero bytes")
    assert int(h["tissue"][0]) == 33 * 47 and int(stain_histogram(gz, black=1)["tissue"][0]) == 0
    # saturated colours: concentrations from -1.6 to 4.5, so both clamps are hit
    sat = np.array([(1, 1, 1), (0, 0, 255), (255, 0, 0), (0, 255, 0), (200, 100, 20)], np.uint8)
    c = R.concentrations32(sat, m32)
    assert c.min() < -1.5 and c.max() > 4.4
    img = np.ascontiguousarray(sat[np.arange(2 * 15 * 25) % 5].reshape(2, 15, 25, 3))
    ref_hist, ref_tissue = C.histogram(img, m32)
    assert ref_hist[..., 0].max() > 0 and ref_hist[..., NB - 1].max() > 0
    t = calibrate_thresholds(torch.from_numpy(img).to(DEV), quantiles=QS)
    _check_hist(t, ref_hist, ref_tissue, "saturated")
    _check_rules(t, ref_hist, 16, "saturated")
    pr = C.pair_histogram(img, img[:, ::-1].copy(), m32, 1, JT)[0]
    p = stain_pair_histogram(torch.from_numpy(img).to(DEV), torch.from_numpy(img[:, ::-1].copy()).to(DEV),
                             target_threshold=JT / 1024)
    _same(p["hist"], pr, "saturated pair")
    _check_match(match_thresholds(p), pr, JT, "saturated pair")


# ---- 3. cross-checks against the existing kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_curves_are_what_quantify_and_agreement_return(kind):
    (ga, gb), _ = _inputs(kind, 3, 64, 80, False, 31)
    t = calibrate_thresholds(ga)
    m = match_thresholds(stain_pair_histogram(ga, gb, stain=1, target_threshold=JT / 1024))
    pa, pb, both = (m[k].cpu().numpy().astype(np.float64) for k in ("positive_pred", "positive_target", "both_common"))
    assert torch.equal(m["dice_cond"][:, JT], m["dice_common"][:, JT])
    assert torch.equal(m["positive_pred"], t["positive"][:, 1])
    for j in (1, 52, 205, 1024, 4095):
        thr = (j / 1024,) * 3
        q = stain_quantify(ga, thresholds=thr)
        assert torch.equal(t["positive"][:, :, j], q["positive"]), j
        assert torch.equal(t["tissue"], q["tissue"])
        ag = {k: v.cpu().numpy().astype(np.float64) for k, v in stain_agreement(ga, gb, stain=1, thresholds=thr).items()}
        union = pa[:, j] + pb[:, j] - both[:, j]
        dice = np.where(union == 0, 1.0, 2 * both[:, j] / np.maximum(pa[:, j] + pb[:, j], 1))
        iou = np.where(union == 0, 1.0, both[:, j] / np.maximum(union, 1))
        for name, want in (("dice", dice), ("iou", iou)):
            err = np.abs(ag[name] - want) / np.maximum(np.abs(want), 1e-300)
            err = np.where(want == 0, np.abs(ag[name]), err)
            print(f"{kind} j {j} {name}: max rel err {err.max():.3e} (tolerance {F32:.1e})")
            assert (err <= F32).all(), (j, name)
        err = np.abs(m["dice_common"][:, j].cpu().numpy() - dice)
        assert (err <= 2.0 ** -52).all(), j


# ---- 4. batch independence and accumulation ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_a_sample_does_not_see_its_batch_mates_runs_repeat_and_out_accumulates(kind):
    (ga, gb), _ = _inputs(kind, 4, 64, 80, False, 41)
    h1, h2 = stain_histogram(ga), stain_histogram(ga)
    p1 = stain_pair_histogram(ga, gb, target_threshold=JT / 1024)
    p2 = stain_pair_histogram(ga, gb, target_threshold=JT / 1024)
    assert torch.equal(h1["hist"], h2["hist"]) and torch.equal(h1["tissue"], h2["tissue"])
    assert torch.equal(p1["hist"], p2["hist"]) and torch.equal(p1["tissue"], p2["tissue"])
    t1, t2 = stain_thresholds(h1, quantiles=QS), stain_thresholds(h2, quantiles=QS)
    assert all(torch.equal(t1[k], t2[k]) for k in t1)
    m1, m2 = match_thresholds(p1), match_thresholds(p2)
    assert all(torch.equal(m1[k], m2[k]) for k in m1)
    for n in (0, 3):
        ts = calibrate_thresholds(ga[n:n + 1], quantiles=QS)
        assert all(torch.equal(ts[k][0], t1[k][n]) for k in t1), n
        ms = match_thresholds(stain_pair_histogram(ga[n:n + 1], gb[n:n + 1], target_threshold=JT / 1024))
        assert all(torch.equal(ms[k][0], m1[k][n]) for k in m1), n
    # a dataset-level histogram: two half-batches added into one result equal the pooled whole
    whole = stain_histogram(ga, pool=True)
    acc = stain_histogram(ga[:2], pool=True)
    assert stain_histogram(ga[2:], pool=True, out=acc) is acc
    assert torch.equal(acc["hist"], whole["hist"]) and torch.equal(acc["tissue"], whole["tissue"])
    assert torch.equal(whole["hist"][0], h1["hist"].sum(0))
    pw = stain_pair_histogram(ga, gb, target_threshold=JT / 1024, pool=True)
    pacc = stain_pair_histogram(ga[:2], gb[:2], target_threshold=JT / 1024, pool=True)
    stain_pair_histogram(ga[2:], gb[2:], target_threshold=JT / 1024, pool=True, out=pacc)
    assert torch.equal(pacc["hist"], pw["hist"]) and torch.equal(pacc["tissue_target"], pw["tissue_target"])
    with pytest.raises(ValueError):
        stain_pair_histogram(ga[2:], gb[2:], target_threshold=0.25, pool=True, out=pacc)      # another target threshold
    with pytest.raises(ValueError):
        stain_histogram(ga, out=acc)                                                          # four owners into one
    # the one read-back
    thr = thresholds_tuple(t1, "quantile", owner=3, quantile=1)
    assert (t1["quantile_valid"][3] == 1).all() and thr == tuple(t1["quantile"][3, :, 1].tolist())
    q = stain_quantify(ga, thresholds=thr)["positive"][3]
    for k in range(3):
        assert int(q[k]) == int(t1["positive"][3, k, int(t1["quantile_bin"][3, k, 1])]), k
        assert int(q[k]) <= int(t1["tissue"][3]) // 2


# ---- 5. regions -------------------------------------------------------------------------------------------------------
def test_regions_for_host_and_gpu_input_and_every_banding():
    H, W = 301, 203
    a, b = _pair(1, H, W, 51)
    m32 = _m32()
    ha, hb = torch.from_numpy(a[0]), torch.from_numpy(b[0])
    big = torch.zeros((H + 2, W + 3, 3), dtype=torch.uint8, device=DEV)
    ga = big[1:1 + H, 2:2 + W]                                             # a crop view: odd pitch, unaligned base
    ga.copy_(ha)
    gb = hb.to(DEV)
    base = stain_histogram(ga[None])
    _check_hist(base, *C.histogram(a, m32), "region bytes")
    pbase = stain_pair_histogram(ga[None], gb[None], target_threshold=JT / 1024)
    _same(pbase["hist"], C.pair_histogram(a, b, m32, 1, JT)[0], "region pair bytes")
    tbase, mbase = stain_thresholds(base, quantiles=QS), match_thresholds(pbase)
    for src in (ga, ha):
        for band_rows in (16, 48, None):
            got = region_stain_histogram(src, band_rows=band_rows)
            assert torch.equal(got["hist"], base["hist"]) and torch.equal(got["tissue"], base["tissue"]), (src.is_cuda, band_rows)
            if band_rows is not None:
                assert region_stain_histogram.last_stats["bands"] == -(-H // band_rows)
            t = calibrate_thresholds(src, band_rows=band_rows, quantiles=QS)
            assert all(torch.equal(t[k], tbase[k]) for k in tbase), (src.is_cuda, band_rows)
    for pair in ((ga, gb), (ha, hb), (ga, hb)):                            # the last: one on the GPU, one on the host
        for band_rows in (16, 48, None):
            got = region_stain_pair_histogram(*pair, band_rows=band_rows, target_threshold=JT / 1024)
            assert torch.equal(got["hist"], pbase["hist"]) and torch.equal(got["tissue"], pbase["tissue"]), band_rows
            m = match_thresholds(got)
            assert all(torch.equal(m[k], mbase[k]) for k in mbase), band_rows
    two = region_stain_histogram(ha, out=region_stain_histogram(ga))      # two regions of one slide
    assert torch.equal(two["hist"], 2 * base["hist"]) and torch.equal(two["tissue"], 2 * base["tissue"])


# ---- 6. capture and replay --------------------------------------------------------------------------------------------
def test_calibration_in_a_captured_graph():
    a, b = _pair(2, 64, 64, 61)
    a2, b2 = _pair(2, 64, 64, 62)
    ga, gb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    eager_t = calibrate_thresholds(ga, quantiles=QS)
    eager_m = match_thresholds(stain_pair_histogram(ga, gb, target_threshold=JT / 1024))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                  # one stream, a plain chain of launches: no parallel branches
        out_t = calibrate_thresholds(ga, quantiles=QS)
        out_m = match_thresholds(stain_pair_histogram(ga, gb, target_threshold=JT / 1024))
    for v in list(out_t.values()) + list(out_m.values()):
        v.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out_t[k], eager_t[k]) for k in eager_t)
    assert all(torch.equal(out_m[k], eager_m[k]) for k in eager_m)
    ga.copy_(torch.from_numpy(a2))                 # the graph reads its inputs at replay
    gb.copy_(torch.from_numpy(b2))
    graph.replay()
    torch.cuda.synchronize()
    m32 = _m32()
    _check_rules(out_t, C.histogram(a2, m32)[0], 16, "replay")
    _same(out_t["hist"], C.histogram(a2, m32)[0], "replay hist")
    _check_match(out_m, C.pair_histogram(a2, b2, m32, 1, JT)[0], JT, "replay pair")
    del graph
