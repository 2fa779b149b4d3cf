"""Hysteresis thresholding and seeded component selection without a GPU: the restatement of tests/hysteresis_ref.py
(scipy.ndimage.label + bincount) against scipy's own binary reconstruction, the case the feature exists for, the exports,
the status codes of the new entry points (returned before any HIP call) and the argument checks the wrappers make before
they touch the device."""
import numpy as np
import pytest
import torch

import hysteresis_ref as Y
import objects_ref as O

SHAPES = [(1, 1), (1, 70), (33, 65), (70, 130), (97, 200)]
PS = (0.3, 0.55, 0.62, 0.9)
NEW_SYMBOLS = ["s2s_objects_label_seeded", "s2s_hyst_mask", "s2s_hyst_finalize"]
PUBLIC = ["select_components", "reconstruct_mask", "clear_border", "hysteresis_mask", "stain_objects_hysteresis",
          "stain_agreement_hysteresis", "region_stain_objects_hysteresis", "hysteresis_thresholds"]


# ---- the reference against scipy's reconstruction ---------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_selection_equals_binary_propagation(H, W):
    for p in PS:
        mask = O.bernoulli((H, W), p, seed=H * W + int(100 * p))
        marker = O.bernoulli((H, W), 0.01, seed=H + W + int(100 * p))
        for conn in (4, 8):
            sel, cand, seeded, pixels = Y.selected(mask, marker, conn)
            assert np.array_equal(sel, Y.propagation(mask, marker, conn)), (p, conn)
            assert pixels == int(((mask != 0) & (marker != 0)).sum()) and seeded <= cand
            inv = Y.selected(mask, marker, conn, invert=True)[0]
            assert np.array_equal(inv, (mask != 0) & ~sel), (p, conn)
            r = Y.select(mask, marker, conn)
            assert r["count"] == seeded and r["kept_pixels"] == sel.sum() and np.array_equal(r["labels"] > 0, sel)
            # clear_border: the mask minus the propagation of the border pixels
            want = (mask != 0) & ~Y.propagation(mask, Y.border(H, W), conn)
            assert np.array_equal(Y.clear_border(mask, conn), want), (p, conn)


def test_selection_options():
    mask = O.bernoulli((33, 65), 0.55, seed=3)
    marker = O.bernoulli((33, 65), 0.05, seed=4)
    lab, n = O.flood_label(mask, 8)
    seeds = np.bincount(lab[(marker != 0) & (mask != 0)], minlength=n + 1)
    for min_seed in (1, 2, int(seeds[1:].max()) + 1):
        sel, cand, seeded, _ = Y.selected(mask, marker, 8, min_seed)
        keep = seeds >= min_seed
        keep[0] = False
        assert np.array_equal(sel, keep[lab]) and cand == n and seeded == int(keep.sum())
    assert not Y.selected(mask, marker, 8, int(seeds[1:].max()) + 1)[0].any()
    # marker = mask, and no marker with invert, are the plain labelling
    for r in (Y.select(mask, mask, 8, min_area=3, max_objects=5),
              Y.select(mask, np.zeros_like(mask), 8, invert=True, min_area=3, max_objects=5)):
        want = O.components(mask, 8, 3, 5)
        for k in want:
            assert np.array_equal(r[k], want[k]), k


def test_dual_mask_definition():
    rng = np.random.default_rng(2)
    t = rng.integers(0, 4096, size=(2, 9, 11)).astype(np.int16)
    tis = rng.random((2, 9, 11)) < 0.8
    byte, counts = Y.dual(t, tis, 1000, 3000)
    assert np.array_equal(byte & 2 != 0, tis) and np.array_equal(byte & 1 != 0, tis & (t >= 1000))
    assert np.array_equal(byte & 4 != 0, tis & (t >= 3000)) and ((byte & 4 == 0) | (byte & 1 != 0)).all()
    assert np.array_equal(counts[:, 0], tis.reshape(2, -1).sum(1)) and (counts[:, 2] <= counts[:, 1]).all()
    assert np.array_equal(Y.dual(t, tis, 1000, 3000, pool=True)[1], counts.sum(0, keepdims=True))
    # low == high: every weak pixel is its own seed
    assert np.array_equal(Y.hysteresis(t, tis, 1000, 1000), (tis & (t >= 1000)).astype(np.uint8))
    assert not Y.hysteresis(t, None, 1000, 4095)[t.max(axis=(1, 2)) < 4095].any()


def test_plaques_with_halo_and_speckle():
    """The case the feature exists for: at low = 128 / 1024, high = 320 / 1024 the hysteresis mask is exactly the four
    halo discs; the low threshold alone keeps every speckle, the high one only the cores."""
    t, halo = Y.plaques()
    assert t.shape == (96, 160)
    hyst = Y.hysteresis(t[None], None, 128, 320, connectivity=8)[0]
    assert np.array_equal(hyst != 0, halo) and int(hyst.sum()) == 1012
    assert O.label(hyst, 8)[1] == 4
    low = t >= 128
    assert int(low.sum()) == 1259 and O.label(low, 8)[1] == 233
    assert int((t >= 320).sum()) == 116


# ---- exports ----------------------------------------------------------------------------------------------------------
def test_exports():
    import stain2stain_amd
    from stain2stain_amd import _native, hysteresis, objects
    for name in PUBLIC:
        assert name in stain2stain_amd.__all__ and getattr(stain2stain_amd, name) is getattr(hysteresis, name)
    assert "hysteresis.hip" in _native.SOURCES and "objects.hip" in _native.SOURCES
    declared = _native.declared_symbols()
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in declared and hasattr(lib, sym), sym
    assert hysteresis.MAX_PIXELS == objects.MAX_PIXELS == 2 ** 31 - 2


# ---- status codes of the entry points: returned before any HIP call ---------------------------------------------------
def test_entry_points_return_status_codes():
    from stain2stain_amd import _native
    lib = _native.lib()
    X = 4096                                      # a non-null pointer that is never dereferenced: every call below fails first

    def seeded(mask=X, pitch=64, img=64 * 32, fg=255, marker=X, mpitch=64, mimg=64 * 32, bits=255, min_seed=1, invert=0,
               B=1, H=32, W=64, conn=8, min_area=1, M=0, scratch=X, labels=X, count=X, kept=X, largest=X, hist=X,
               ta=X, tb=X, ts=X, out=X, opitch=64, oimg=64 * 32, cand=X, nseeded=X, pixels=X):
        return lib.s2s_objects_label_seeded(mask, pitch, img, fg, marker, mpitch, mimg, bits, min_seed, invert, B, H, W,
                                            conn, min_area, M, scratch, labels, count, kept, largest, hist, ta, tb, ts,
                                            out, opitch, oimg, cand, nseeded, pixels, None)

    for name in ("mask", "marker", "scratch", "labels", "count", "kept", "largest", "hist", "cand", "nseeded", "pixels"):
        assert seeded(**{name: 0}) == -5, name
    assert seeded(M=4, ta=0) == -5 and seeded(M=4, tb=0) == -5 and seeded(M=4, ts=0) == -5
    assert seeded(fg=0) == -1 and seeded(fg=256) == -1 and seeded(bits=0) == -1 and seeded(bits=256) == -1
    assert seeded(min_seed=0) == -1 and seeded(min_seed=-3) == -1 and seeded(invert=2) == -1 and seeded(invert=-1) == -1
    assert seeded(conn=6) == -1 and seeded(min_area=0) == -1 and seeded(M=-1) == -1
    assert seeded(B=0) == -1 and seeded(B=65536) == -1 and seeded(H=0) == -1 and seeded(W=0) == -1
    assert seeded(H=65536, W=32768, pitch=32768, mpitch=32768, opitch=32768) == -1          # 2^31 pixels
    assert seeded(pitch=63) == -1 and seeded(mpitch=63) == -1 and seeded(opitch=63) == -1
    assert seeded(B=2, img=64 * 31) == -1 and seeded(B=2, mimg=64 * 31) == -1 and seeded(B=2, oimg=64 * 31) == -1
    assert seeded(B=65535, M=65535) == -1

    def hyst(t=X, tissue=X, B=1, rows=32, W=64, row0=0, nrows=32, j_low=100, j_high=200, pool=0, reset=1, counts=X,
             mask=X, out_img=32 * 64):
        return lib.s2s_hyst_mask(t, tissue, B, rows, W, row0, nrows, j_low, j_high, pool, reset, counts, mask, out_img,
                                 None)

    assert hyst(t=0) == -5 and hyst(counts=0) == -5 and hyst(mask=0) == -5
    assert hyst(j_low=201) == -1 and hyst(j_low=-1) == -1 and hyst(j_high=4096) == -1 and hyst(j_low=4096, j_high=4096) == -1
    assert hyst(B=0) == -1 and hyst(B=65536) == -1 and hyst(rows=0) == -1 and hyst(W=0) == -1
    assert hyst(rows=32768, nrows=1) == -1 and hyst(W=32768) == -1
    assert hyst(row0=-1) == -1 and hyst(nrows=0) == -1 and hyst(row0=1) == -1 and hyst(nrows=33) == -1
    assert hyst(B=2, out_img=32 * 64 - 1) == -1
    assert hyst(B=65535, rows=32767, W=32767, nrows=32767, pool=1, out_img=32767 * 32767) == -1   # 2^32 pixels a workgroup

    fin = lib.s2s_hyst_finalize
    assert fin(0, X, 1, X, None) == -5 and fin(X, 0, 1, X, None) == -5 and fin(X, X, 1, 0, None) == -5
    assert fin(X, X, 0, X, None) == -1 and fin(X, X, 65536, X, None) == -1


# ---- argument checks that need no GPU ---------------------------------------------------------------------------------
def test_wrappers_reject_before_the_gpu():
    from stain2stain_amd import (clear_border, hysteresis_mask, reconstruct_mask, region_stain_objects_hysteresis,
                                 select_components, stain_agreement_hysteresis, stain_objects_hysteresis)
    from stain2stain_amd.hysteresis import MAX_PIXELS
    m = torch.zeros((2, 16, 16), dtype=torch.uint8)
    with pytest.raises(TypeError):
        select_components(m.numpy(), m)
    with pytest.raises(TypeError):
        select_components(m, m.numpy())
    for bad in (m.float(), m[0, 0], m[None], m[:1], m[:, :8], m[0]):
        with pytest.raises(ValueError):
            select_components(m, bad)
        with pytest.raises(ValueError):
            reconstruct_mask(m, bad)
    for kw in ({"connectivity": 6}, {"min_seed": 0}, {"min_seed": -1}, {"min_seed": MAX_PIXELS + 1}, {"min_area": 0},
               {"max_objects": 0}):
        with pytest.raises(ValueError):
            select_components(m, m, **kw)
    with pytest.raises(TypeError):
        select_components(m, m, min_seed=1.5)
    with pytest.raises(ValueError):
        reconstruct_mask(m, m, connectivity=5)
    with pytest.raises(ValueError):
        clear_border(m.float())
    with pytest.raises(ValueError):
        clear_border(m, connectivity=5)

    t = torch.zeros((2, 16, 16), dtype=torch.int16)
    lo, hi = 128 / 1024, 320 / 1024
    with pytest.raises(TypeError):
        hysteresis_mask(t.numpy(), lo, hi)
    for bad in (t.float(), t.to(torch.uint8), t[0, 0], torch.zeros((0, 4, 4), dtype=torch.int16)):
        with pytest.raises(ValueError):
            hysteresis_mask(bad, lo, hi)
    with pytest.raises(ValueError):
        hysteresis_mask(t, lo, hi, tissue=torch.zeros((2, 16, 15), dtype=torch.bool))
    with pytest.raises(ValueError):
        hysteresis_mask(t, lo, hi, tissue=t)

    tiles = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    region = tiles[0]
    calls = [lambda *a, **kw: hysteresis_mask(t, *a, **kw), lambda *a, **kw: stain_objects_hysteresis(tiles, *a, **kw),
             lambda *a, **kw: stain_agreement_hysteresis(tiles, tiles, *a, **kw),
             lambda *a, **kw: region_stain_objects_hysteresis(region, *a, **kw)]
    for f in calls:
        for low, high in ((0.2, hi), (lo, 0.3), (0.0, hi), (lo, 4.0), (128.5 / 1024, hi), (lo, float("nan")),
                          (-lo, hi), (hi, lo), ("a", hi)):                    # off the grid, or low > high
            with pytest.raises(ValueError):
                f(low, high)
        for kw in ({"connectivity": 6}, {"min_seed": 0}, {"min_seed": MAX_PIXELS + 1}):
            with pytest.raises(ValueError):
                f(lo, hi, **kw)
    for f in calls[1:]:
        for kw in ({"radius": -1}, {"radius": float("nan")}, {"radius": 129}, {"radius": 4, "smooth": -1},
                   {"radius": 4, "smooth": 17}, {"stain": 3}, {"radius": 4, "footprint": "ball"}, {"white": 0}):
            with pytest.raises(ValueError):
                f(lo, hi, **kw)
        with pytest.raises(TypeError):
            f(lo, hi, radius="4")
    for kw in ({"min_area": 0}, {"max_objects": 0}, {"mpp": 0.0}):
        with pytest.raises(ValueError):
            stain_objects_hysteresis(tiles, lo, hi, **kw)
        with pytest.raises(ValueError):
            region_stain_objects_hysteresis(region, lo, hi, **kw)
    with pytest.raises(TypeError):
        stain_objects_hysteresis(tiles.numpy(), lo, hi)
    for bad in (tiles[0], tiles[..., :2], tiles.to(torch.int16)):
        with pytest.raises(ValueError):
            stain_objects_hysteresis(bad, lo, hi)
    with pytest.raises(ValueError):
        stain_agreement_hysteresis(tiles, tiles[:1], lo, hi)
    with pytest.raises(TypeError):
        region_stain_objects_hysteresis(region.numpy(), lo, hi)
    for bad in (tiles, region[..., 0], region.float()):
        with pytest.raises(ValueError):
            region_stain_objects_hysteresis(bad, lo, hi)
    for br in (0, -3):
        with pytest.raises(ValueError):
            region_stain_objects_hysteresis(region, lo, hi, band_rows=br)


def _rules(triangle, otsu, valid=(1, 1)):
    """A stain_thresholds result with the given bins for stain 1 of one owner (host tensors: the call only reads them)."""
    tb, ob = torch.zeros((1, 3), dtype=torch.int32), torch.zeros((1, 3), dtype=torch.int32)
    tv, ov = torch.zeros((1, 3), dtype=torch.int32), torch.zeros((1, 3), dtype=torch.int32)
    tb[0, 1], ob[0, 1], tv[0, 1], ov[0, 1] = triangle, otsu, valid[0], valid[1]
    return {"triangle_bin": tb, "otsu_bin": ob, "triangle_valid": tv, "otsu_valid": ov}


def test_hysteresis_thresholds():
    from stain2stain_amd import hysteresis_thresholds
    assert hysteresis_thresholds(_rules(128, 320)) == (128 / 1024, 320 / 1024)
    assert hysteresis_thresholds(_rules(128, 320), low="otsu", high="triangle") == (320 / 1024, 320 / 1024)   # raised
    assert hysteresis_thresholds(_rules(400, 320)) == (400 / 1024, 400 / 1024)                                # raised
    assert hysteresis_thresholds(_rules(128, 320), low="otsu", high="otsu") == (320 / 1024, 320 / 1024)
    with pytest.raises(ValueError):
        hysteresis_thresholds(_rules(128, 320, valid=(1, 0)))
    with pytest.raises(ValueError):
        hysteresis_thresholds(_rules(128, 320), stain=0)                      # no answer for that stain
    assert hysteresis_thresholds(_rules(128, 0, valid=(1, 0)), fallback=(100 / 1024, 300 / 1024)) == (128 / 1024, 300 / 1024)
    assert hysteresis_thresholds(_rules(0, 320, valid=(0, 1)), fallback=(100 / 1024, 300 / 1024)) == (100 / 1024, 320 / 1024)
    assert hysteresis_thresholds(_rules(0, 50, valid=(0, 1)), fallback=(100 / 1024, 300 / 1024)) == (100 / 1024, 100 / 1024)
    for kw in ({"low": "mean"}, {"high": "quantile"}, {"stain": 3}, {"owner": 1}, {"fallback": (0.1,)},
               {"fallback": (0.1, 0.3)}):
        with pytest.raises(ValueError):
            hysteresis_thresholds(_rules(128, 320), **kw)
    with pytest.raises(TypeError):
        hysteresis_thresholds({"otsu_bin": torch.zeros((1, 3))})
