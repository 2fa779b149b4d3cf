"""Stain threshold calibration (stain2stain_amd/stain_calibrate.py, csrc/stain_calibrate.hip) without a
GPU: the restatement of tests/stain_calibrate_ref.py against the definitions it restates (the bin rule against
``positive32`` at every threshold of the grid, Otsu and the matching rules against exact rational arithmetic, the
triangle rule against closed forms), the boundary (exports, the status codes of the new entry points) and the argument
checks the wrappers make before they touch the device."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import stain_calibrate_ref as C
import stain_quant_ref as R

NB = C.NB


def _m32():
    from stain2stain_amd.stain_quant import unmix_matrix
    return unmix_matrix("hdab").numpy()


def _stained(B, H, W, seed, plaque=0.08):
    """The generator of tests/test_stain_quant_gpu.py: haematoxylin background with DAB blobs, glass, specks, noise."""
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


# ---- the boundary ----------------------------------------------------------------------------------------------------
SYMBOLS = {"s2s_stain_hist_u8", "s2s_stain_hist_f32", "s2s_stain_pair_hist_u8", "s2s_stain_pair_hist_f32",
           "s2s_stain_thresholds", "s2s_stain_pair_thresholds"}
EXPORTS = ("stain_histogram", "region_stain_histogram", "stain_thresholds", "calibrate_thresholds", "thresholds_tuple",
           "stain_pair_histogram", "region_stain_pair_histogram", "match_thresholds")


def test_exports_sources_and_symbols():
    import re
    import os
    import stain2stain_amd
    from stain2stain_amd import _native, stain_calibrate
    for name in EXPORTS:
        assert name in stain2stain_amd.__all__ and getattr(stain2stain_amd, name) is getattr(stain_calibrate, name), name
    assert "stain_calibrate.hip" in _native.SOURCES
    assert SYMBOLS <= set(_native.declared_symbols())
    lib = _native.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    text = open(os.path.join(_native.CSRC, "stain_calibrate.hip")).read()
    assert not re.search(r'getenv\("S2S_', text)
    assert stain_calibrate.NB == NB and stain_calibrate.BINS_PER_OD == 1024


# ---- the bin rule ----------------------------------------------------------------------------------------------------
def test_bin_rule_reproduces_the_strict_comparison_at_every_grid_threshold():
    m32 = _m32()
    img = np.concatenate([_stained(1, 64, 64, 3), np.random.default_rng(4).integers(0, 256, (1, 64, 64, 3), dtype=np.uint8)])
    img[1, 0, :5] = [(1, 1, 1), (0, 0, 255), (255, 0, 0), (0, 255, 0), (200, 100, 20)]     # saturated colours
    c = R.concentrations32(img, m32)
    b = C.bins32(c)
    assert c.min() < -1.0 and c.max() > 4.0 and b.min() == 0 and b.max() == NB - 1          # both clamps are hit
    t = R.tissue(img)
    for j in range(1, NB):
        thr = (j / 1024.0,) * 3
        assert np.float32(j / 1024.0) == j / 1024.0            # on the grid a threshold is exact in fp32
        want = R.positive32(img, m32, thr)
        assert np.array_equal(t[..., None] & (b >= j), want), j
    hist, tissue = C.histogram(img, m32)
    assert np.array_equal(hist.sum(-1), np.repeat(tissue[:, None], 3, 1))
    pooled, pt = C.histogram(img, m32, pool=True)
    assert np.array_equal(pooled[0], hist.sum(0)) and pt[0] == tissue.sum()
    # edge values of the rule itself
    edge = np.array([-2.0, 0.0, 1 / 1024, np.nextafter(np.float32(1 / 1024), np.float32(1)), 2 / 1024, 0.2,
                     4095 / 1024, np.nextafter(np.float32(4095 / 1024), np.float32(9)), 4.5], dtype=np.float32)
    assert C.bins32(edge).tolist() == [0, 0, 0, 1, 1, 204, 4094, 4095, 4095]


# ---- Otsu ------------------------------------------------------------------------------------------------------------
def _otsu_exact(h):
    pos = C.suffix(h)
    s1 = C.suffix([b * int(v) for b, v in enumerate(h)])
    N, S = pos[0], s1[0]
    best, arg = Fraction(0), 0
    for j in range(1, NB):
        P = pos[j]
        if P in (0, N):
            continue
        s = Fraction((N * s1[j] - P * S) ** 2, P * (N - P))
        if s > best:
            best, arg = s, j
    return arg


def test_otsu_lands_between_two_clusters_and_equals_exact_arithmetic():
    h = np.zeros(NB, np.int64)
    h[40:60] = [5, 9, 14, 30, 55, 80, 96, 110, 96, 80, 55, 30, 14, 9, 5, 3, 2, 1, 1, 1]
    h[600:620] = [1, 2, 4, 8, 12, 20, 24, 30, 24, 20, 12, 8, 4, 2, 1, 1, 1, 1, 1, 1]
    j, ok = C.otsu(h)
    assert ok == 1 and 60 <= j <= 600 and j == _otsu_exact(h) == 60       # sigma is flat over the gap: the smallest j
    rng = np.random.default_rng(7)
    for scale in (1, 1 << 20, 1 << 39):                                   # counts up to the 2^40 of one owner
        h = (rng.integers(0, 50, NB) * (rng.random(NB) < 0.05)).astype(np.int64)
        h[100:140] += rng.integers(1, 400, 40)
        h[900:1000] += rng.integers(1, 90, 100)
        h *= scale
        assert C.otsu(h)[0] == _otsu_exact(h), scale
    assert C.otsu(np.zeros(NB, np.int64)) == (0, 0)
    one = np.zeros(NB, np.int64)
    one[77] = 1234
    assert C.otsu(one) == (0, 0)


# ---- the triangle rule -----------------------------------------------------------------------------------------------
def test_triangle_closed_forms():
    g = np.zeros(256, np.int64)
    g[10:60] = 1000 - 20 * (np.arange(10, 60) - 10)            # the peak at 10, a straight tail that ends at 59
    assert g[59] == 20
    fine = np.zeros(NB, np.int64)
    fine[16 * np.arange(256) + 3] = g
    assert C.triangle(fine, 16) == (16 * 11, 1)                # every T is 0: the smallest index right of the peak
    g[30] -= 150                                               # one dip: T(30) = 150 (e - p), every other T is 0
    fine[16 * np.arange(256) + 3] = g
    assert C.triangle(fine, 16) == (16 * 30, 1)
    assert C.triangle(fine, 1) == (164, 1)                     # ungrouped: the empty bin right of the peak at 163
    # two equal peaks: the first is the peak; a histogram that ends right after its peak has no tail
    two = np.zeros(NB, np.int64)
    two[[32, 64, 480]] = [500, 500, 1]
    assert C.triangle(two, 16) == (16 * 3, 1)                  # (from the second peak it would be 16 * 5)
    short = np.zeros(NB, np.int64)
    short[[160, 176]] = [9, 3]
    assert C.triangle(short, 16) == (0, 0) and C.triangle(np.zeros(NB, np.int64), 16) == (0, 0)
    assert C.triangle(short, 4096) == (0, 0)


def test_triangle_finds_the_plaque_share_of_a_synthetic_tile():
    m32 = _m32()
    img = _stained(1, 256, 256, 5)
    hist, tissue = C.histogram(img, m32, black=1)
    j, ok = C.triangle(hist[0, 1], 16)
    burden = C.suffix(hist[0, 1])[j] / int(tissue[0])
    print(f"triangle on DAB: threshold {j / 1024:.4f}, burden {burden:.4f}")
    assert ok == 1 and 0.07 <= burden <= 0.09                  # the plaque share of the generator is 0.08


# ---- quantiles -------------------------------------------------------------------------------------------------------
def test_quantile_edge_cases():
    h = np.zeros(NB, np.int64)
    h[[0, 10, 20, 30]] = [60, 20, 15, 5]
    assert C.quantile(h, 1.0) == (1, 1)                        # everything may stay positive: the smallest threshold
    assert C.quantile(h, 0.4) == (1, 1)                        # positive[1] = 40 <= 40
    assert C.quantile(h, 0.399) == (11, 1)                     # floor(39.9) = 39 < 40: past bin 10
    assert C.quantile(h, 0.05) == (21, 1) and C.quantile(h, 0.049) == (31, 1)
    assert C.quantile(h, 0.0) == (31, 1)                       # nothing positive: one past the last occupied bin
    top = h.copy()
    top[NB - 1] = 1
    assert C.quantile(top, 0.0) == (NB - 1, 0)                 # the last bin cannot be cleared
    assert C.quantile(top, 0.01) == (31, 1)
    assert C.quantile(np.zeros(NB, np.int64), 0.5) == (NB - 1, 0)
    t = C.thresholds(np.stack([h, top, np.zeros(NB, np.int64)])[None], quantiles=(0.0, 0.4))
    assert t["quantile_bin"][0].tolist() == [[31, 1], [NB - 1, 11], [NB - 1, NB - 1]]     # (top: 41 of 101 > floor(40.4))
    assert t["quantile_valid"][0].tolist() == [[1, 1], [0, 1], [0, 0]]
    assert t["positive"][0, 0, 0] == 100 and t["positive"][0, 0, 11] == 20 and t["quantile"][0, 0, 0] == 31 / 1024


# ---- the matching rules ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,jt", [(1, 205), (2, 52), (3, 1)])
def test_matching_rules_against_brute_force(seed, jt):
    m32 = _m32()
    a, b = _stained(1, 48, 56, seed, plaque=0.15), _stained(1, 48, 56, 10 + seed, plaque=0.10)
    b[:, :24] = a[:, :24]
    hist, tissue = C.pair_histogram(a, b, m32, stain=1, jt=jt)
    got = C.match(hist[0], jt)
    ta, tb = R.tissue(a[0]), R.tissue(b[0])
    ba = C.bins32(R.concentrations32(a[0], m32)[..., 1])
    bb = C.bins32(R.concentrations32(b[0], m32)[..., 1])
    Na, Nb = int(ta.sum()), int(tb.sum())
    assert (Na, Nb) == tuple(tissue[0])
    pbt = int((tb & (bb >= jt)).sum())
    err, dice = [], []
    for j in range(1, NB):
        pa = int((ta & (ba >= j)).sum())
        both = int((ta & tb & (ba >= j) & (bb >= jt)).sum())
        err.append(abs(Fraction(pa, Na) - Fraction(pbt, Nb)))
        dice.append(Fraction(1) if pa + pbt == 0 else Fraction(2 * both, pa + pbt))
        assert got["both_cond"][j] == both and got["positive_pred"][j] == pa
        assert got["both_common"][j] == int((ta & tb & (ba >= j) & (bb >= j)).sum())
    assert got["match_burden_bin"] == 1 + err.index(min(err))
    assert got["best_dice_bin"] == 1 + dice.index(max(dice))
    assert got["dice_at_best"] == float(2 * int(got["both_cond"][got["best_dice_bin"]])) / float(
        int(got["positive_pred"][got["best_dice_bin"]]) + pbt)
    assert abs(got["dice_at_best"] - float(max(dice))) <= 2.0 ** -52
    assert got["dice_cond"][jt] == got["dice_common"][jt]
    assert got["match_burden_valid"] == 1 and got["best_dice_valid"] == 1
    # agreement32 of the restatement of 3.17 at the common threshold jt
    ref = R.agreement32(a, b, m32, (jt / 1024.0,) * 3, stain=1)
    assert abs(got["dice_common"][jt] - ref["dice"][0]) <= 2.0 ** -52
    glass = np.full_like(a, 255)
    h0, _ = C.pair_histogram(glass, b, m32, jt=jt)
    m0 = C.match(h0[0], jt)
    assert m0["match_burden_valid"] == 0 and m0["best_dice_valid"] == 0 and m0["match_burden_bin"] == 1


# ---- status codes of the entry points: returned before any HIP call ---------------------------------------------------
def test_entry_points_return_status_codes():
    from stain2stain_amd import _native
    lib = _native.lib()
    od, um = (ctypes.c_float * 256)(), (ctypes.c_float * 12)()
    X = 4096                                      # a non-null pointer that is never dereferenced: every call below fails first

    def u8(img=X, pitch=96, B=1, band_top=0, band_h=32, H=32, W=32, od=od, um=um, white=220, black=0, mask=7, pool=0,
           hist=X, tissue=X, stride=None):
        return lib.s2s_stain_hist_u8(img, pitch, pitch * band_h if stride is None else stride, B, band_top, band_h, H, W,
                                     od, um, white, black, mask, pool, 1, hist, tissue, None)

    assert u8(img=0) == -5 and u8(hist=0) == -5 and u8(tissue=0) == -5 and u8(od=None) == -5 and u8(um=None) == -5
    assert u8(B=0) == -1 and u8(B=-2) == -1 and u8(B=65536) == -1 and u8(H=0) == -1 and u8(W=-1) == -1
    assert u8(mask=0) == -1 and u8(mask=8) == -1 and u8(mask=-1) == -1
    assert u8(pitch=95) == -1 and u8(band_h=0) == -1 and u8(band_h=33) == -1 and u8(band_top=1) == -1 and u8(band_top=-1) == -1
    assert u8(B=2, stride=96 * 31) == -1
    assert u8(white=0) == -1 and u8(white=257) == -1 and u8(black=256) == -1 and u8(black=-1) == -1
    assert u8(H=1 << 30, W=1 << 11, pitch=3 << 11, band_h=1) == -1         # 2^41 pixels in one owner
    assert u8(H=1 << 20, W=1 << 10, pitch=3 << 10, band_h=1, B=2048, pool=1, stride=3 << 10) == -1   # pooled: 2^41

    def f32(img=X, B=1, H=8, W=8, od=od, um=um, mask=7, hist=X, tissue=X, white=220):
        return lib.s2s_stain_hist_f32(img, B, H, W, od, um, white, 0, mask, 0, 1, hist, tissue, None)

    assert f32(img=0) == -5 and f32(hist=0) == -5 and f32(tissue=0) == -5 and f32(od=None) == -5 and f32(um=None) == -5
    assert f32(B=0) == -1 and f32(H=0) == -1 and f32(W=-3) == -1 and f32(mask=0) == -1 and f32(white=300) == -1

    def p8(a=X, b=X, pitch=96, B=1, band_top=0, band_h=32, H=32, W=32, od=od, um=um, stain=1, jt=205, hist=X, tissue=X,
           pitch_b=96):
        return lib.s2s_stain_pair_hist_u8(a, pitch, pitch * band_h, b, pitch_b, pitch_b * band_h, B, band_top, band_h, H,
                                          W, od, um, 220, 0, stain, jt, 0, 1, hist, tissue, None)

    assert p8(a=0) == -5 and p8(b=0) == -5 and p8(hist=0) == -5 and p8(tissue=0) == -5 and p8(od=None) == -5
    assert p8(B=0) == -1 and p8(stain=3) == -1 and p8(stain=-1) == -1 and p8(jt=-1) == -1 and p8(jt=4096) == -1
    assert p8(pitch=95) == -1 and p8(pitch_b=95) == -1 and p8(band_h=33) == -1 and p8(W=0) == -1

    def pf(a=X, b=X, B=1, H=8, W=8, um=um, stain=1, jt=0, hist=X, tissue=X):
        return lib.s2s_stain_pair_hist_f32(a, b, B, H, W, od, um, 220, 0, stain, jt, 0, 1, hist, tissue, None)

    assert pf(a=0) == -5 and pf(b=0) == -5 and pf(hist=0) == -5 and pf(tissue=0) == -5 and pf(um=None) == -5
    assert pf(B=0) == -1 and pf(H=0) == -1 and pf(stain=5) == -1 and pf(jt=4096) == -1 and pf(jt=-3) == -1

    q = (ctypes.c_double * 8)(0.05)
    bad = (ctypes.c_double * 8)(1.5)
    nan = (ctypes.c_double * 8)(float("nan"))

    def th(hist=X, rows=3, coarse=16, q=q, nq=1, positive=X, bins=X, valid=X, thr=X):
        return lib.s2s_stain_thresholds(hist, rows, coarse, q, nq, positive, bins, valid, thr, None)

    assert th(hist=0) == -5 and th(positive=0) == -5 and th(bins=0) == -5 and th(valid=0) == -5 and th(thr=0) == -5
    assert th(q=None) == -5
    assert th(rows=0) == -1 and th(rows=-3) == -1 and th(nq=-1) == -1 and th(nq=9) == -1
    assert th(coarse=0) == -1 and th(coarse=3) == -1 and th(coarse=24) == -1 and th(coarse=8192) == -1 and th(coarse=-16) == -1
    assert th(q=bad) == -1 and th(q=nan) == -1

    def pt(hist=X, owners=1, jt=205, counts=X, dice=X, bins=X, valid=X, vals=X):
        return lib.s2s_stain_pair_thresholds(hist, owners, jt, counts, dice, bins, valid, vals, None)

    assert pt(hist=0) == -5 and pt(counts=0) == -5 and pt(dice=0) == -5 and pt(bins=0) == -5 and pt(valid=0) == -5
    assert pt(vals=0) == -5 and pt(owners=0) == -1 and pt(jt=-1) == -1 and pt(jt=4096) == -1


# ---- argument checks that need no GPU --------------------------------------------------------------------------------
def test_wrappers_reject():
    from stain2stain_amd import (calibrate_thresholds, match_thresholds, region_stain_histogram,
                                 region_stain_pair_histogram, stain_histogram, stain_pair_histogram, stain_thresholds,
                                 thresholds_tuple)
    from stain2stain_amd.stain_calibrate import threshold_bin
    u = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    f = torch.zeros((2, 3, 16, 16))
    r = torch.zeros((40, 40, 3), dtype=torch.uint8)
    for fn in (stain_histogram, calibrate_thresholds):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(u)                                                         # CPU tensors: there is no CPU path
        with pytest.raises(RuntimeError, match="GPU"):
            fn(f)
        with pytest.raises(ValueError):
            fn(torch.zeros((2, 16, 16, 4), dtype=torch.uint8))
        with pytest.raises(ValueError):
            fn(f.double())
        with pytest.raises(TypeError):
            fn(u.numpy())
        with pytest.raises(ValueError):
            fn(u, stains="he")
        with pytest.raises(ValueError):
            fn(u, white=0)
        with pytest.raises(ValueError):
            fn(u, black=256)
    for bad in (0, 3, 24, 8192, -16):
        with pytest.raises(ValueError):
            calibrate_thresholds(u, coarse=bad)
        with pytest.raises(ValueError):
            stain_thresholds({"hist": torch.zeros((1, 3, 4096), dtype=torch.int64), "tissue": None}, coarse=bad)
    for bad in ((1.5,), (-0.1,), (float("nan"),), (0.1,) * 9, 0.5):
        with pytest.raises(ValueError):
            calibrate_thresholds(u, quantiles=bad)
    with pytest.raises(TypeError):
        stain_thresholds(torch.zeros((1, 3, 4096), dtype=torch.int64))
    with pytest.raises(ValueError):
        stain_thresholds({"hist": torch.zeros((1, 3, 4096)), "tissue": None})
    with pytest.raises(ValueError):
        stain_thresholds({"hist": torch.zeros((1, 4, 4096), dtype=torch.int64), "tissue": None})
    with pytest.raises(RuntimeError, match="GPU"):
        stain_thresholds({"hist": torch.zeros((1, 3, 4096), dtype=torch.int64), "tissue": None})
    # regions
    with pytest.raises(ValueError):
        region_stain_histogram(r.float())
    with pytest.raises(ValueError):
        region_stain_histogram(r[:, ::2])
    with pytest.raises(ValueError):
        region_stain_histogram(r, band_rows=0)
    with pytest.raises(TypeError):
        region_stain_histogram(None)
    with pytest.raises(ValueError):
        region_stain_pair_histogram(r, r[:39])
    with pytest.raises(ValueError):
        region_stain_pair_histogram(r, r.clone(), stain=3)
    with pytest.raises(ValueError):
        region_stain_pair_histogram(r, r.clone(), band_rows=-4)
    # pairs: the target threshold must lie on the grid
    assert threshold_bin(0.2001953125) == 205 and threshold_bin(1 / 1024) == 1 and threshold_bin(4095 / 1024) == 4095
    for bad in (0.2, 0.0, 4.0, -0.5, float("nan"), float("inf"), "x", 1 / 2048):
        with pytest.raises(ValueError):
            stain_pair_histogram(u, u.clone(), target_threshold=bad)
        with pytest.raises(ValueError):
            region_stain_pair_histogram(r, r.clone(), target_threshold=bad)
    with pytest.raises(RuntimeError, match="GPU"):
        stain_pair_histogram(u, u.clone(), target_threshold=0.25)
    with pytest.raises(ValueError):
        stain_pair_histogram(u, u[:, :15])
    with pytest.raises(ValueError):
        stain_pair_histogram(u, f)
    with pytest.raises(ValueError):
        stain_pair_histogram(u, u.clone(), stain=-1)
    with pytest.raises(TypeError):
        stain_pair_histogram(u, None)
    with pytest.raises(TypeError):
        match_thresholds({"hist": torch.zeros((1, 4, 4096), dtype=torch.int64)})
    with pytest.raises(ValueError):
        match_thresholds({"hist": torch.zeros((1, 3, 4096), dtype=torch.int64), "target_bin": 0})
    with pytest.raises(ValueError):
        match_thresholds({"hist": torch.zeros((1, 4, 4096), dtype=torch.int64), "target_bin": 4096})
    # thresholds_tuple works on host tensors too: it is the read-back
    t = {"otsu": torch.tensor([[0.25, 0.5, 0.0]], dtype=torch.float64), "otsu_valid": torch.tensor([[1, 1, 0]]),
         "quantile": torch.tensor([[[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]]], dtype=torch.float64),
         "quantile_valid": torch.ones((1, 3, 2), dtype=torch.int32)}
    assert thresholds_tuple(t, "quantile", quantile=1) == (0.2, 0.4, 0.6)
    assert thresholds_tuple(t, "otsu", fallback=(0.2, 0.2, 0.2)) == (0.25, 0.5, 0.2)
    with pytest.raises(ValueError, match="no answer"):
        thresholds_tuple(t, "otsu")
    with pytest.raises(ValueError):
        thresholds_tuple(t, "mean")
    with pytest.raises(TypeError):
        thresholds_tuple(t, "triangle")
    with pytest.raises(ValueError):
        thresholds_tuple(t, "otsu", owner=1)
    with pytest.raises(ValueError):
        thresholds_tuple(t, "quantile", quantile=2)
    with pytest.raises(ValueError):
        thresholds_tuple(t, "otsu", fallback=(0.2,))
