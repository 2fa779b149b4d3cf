"""Stain background subtraction without a GPU: the restatement of tests/background_ref.py against itself (brute force over
the footprint, scipy's grey morphology, the row-span form the GPU references are taken from), the exports, the status
codes of the s2s_grey_* entry points (returned before any HIP call) and the argument checks the wrappers make before
they touch the device.

scipy's ``grey_erosion`` / ``grey_dilation`` (``mode="constant"``, ``cval`` the type's maximum / minimum) are the border
convention of this feature and are compared everywhere.  ``grey_opening``, ``grey_closing``, ``white_tophat`` and
``black_tophat`` take ONE ``cval`` for both of their halves, so near an image edge they follow another convention; they are
compared on the pixels farther than 2 floor(radius) from every edge, where no footprint of either half leaves the image,
and the compositions of the two verified halves are compared with brute force over the whole image."""
import numpy as np
import pytest
import torch

import background_ref as G

SMALL = [(1, 1), (1, 9), (5, 1), (23, 31)]
LARGE = [(63, 65), (129, 131), (70, 300)]
# 2 w + 1 crosses 2 (w = 1), 4 (2), 8 (4), 16 (8), 32 (16): both sides of each are here
RADII = (0, 1, 1.5, 2, 3.5, 4, 5, 7.5, 8, 16, 17)
RADIUS_BEYOND = 40          # larger than the diagonal of every SMALL shape
NEW_SYMBOLS = ["s2s_grey_words", "s2s_grey_morph", "s2s_grey_box_mean", "s2s_grey_bins_u8", "s2s_grey_bins_f32",
               "s2s_grey_corrected", "s2s_grey_corrected_finalize", "s2s_grey_pair", "s2s_grey_pair_finalize"]
PUBLIC = ["grey_morphology", "concentration_bins", "stain_background", "stain_quantify_corrected",
          "stain_objects_corrected", "stain_agreement_corrected", "region_stain_quantify_corrected"]


# ---- the reference against itself -------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SMALL)
def test_restatement_equals_brute_force(H, W):
    for dtype in (np.uint8, np.int16):
        for name, x in G.patterns(H, W, dtype, seed=H * W):
            for kind in G.FOOTPRINTS:
                for r in RADII + (RADIUS_BEYOND,):
                    want, spans, sci = (G.all_ops(x, r, kind, form=f) for f in ("brute", "spans", "scipy"))
                    for op in G.OPS:
                        assert np.array_equal(spans[op], want[op]), (name, kind, r, op)
                        assert np.array_equal(sci[op], want[op]), (name, kind, r, op)


def test_one_high_pixel_dilates_to_the_footprint():
    names, x = G.stack(23, 31, np.int16, seed=1)
    x = x[names.index("one high")]
    for kind in G.FOOTPRINTS:
        for r in (0, 1.5, 4, 7.5):
            F = G.footprint(r, kind)
            R = F.shape[0] // 2
            canvas = np.zeros((23 + 2 * R, 31 + 2 * R), bool)
            canvas[23 // 3:23 // 3 + 2 * R + 1, 31 // 2:31 // 2 + 2 * R + 1] = F
            assert np.array_equal(G.dilate(x, r, kind) == 4095, canvas[R:R + 23, R:R + 31]), (kind, r)


@pytest.mark.parametrize("H,W", SMALL + LARGE)
def test_restatement_equals_scipy(H, W):
    small = (H, W) in SMALL
    for dtype in (np.uint8, np.int16):
        names, x = G.stack(H, W, dtype, seed=H + W)
        keep = [i for i, n in enumerate(names) if small or n in ("random", "one low", "disc mask", "signed")]
        unsigned = [i for i in keep if names[i] != "signed"]
        for kind in G.FOOTPRINTS:
            for r in RADII + ((RADIUS_BEYOND,) if small else ()):
                e, d = G.erode(x, r, kind), G.dilate(x, r, kind)
                for i in keep:
                    assert np.array_equal(e[i], G.erode_scipy(x[i], r, kind)), (names[i], kind, r)
                    assert np.array_equal(d[i], G.dilate_scipy(x[i], r, kind)), (names[i], kind, r)
                if r in (1.5, 4, 8):                        # scipy's own compositions, away from the edges
                    ops = G.all_ops(x, r, kind)
                    for op in ("open", "close", "tophat", "bothat"):
                        got = ops[op]
                        for i in unsigned:
                            want = G.scipy_composite(x[i], op, r, kind)
                            assert np.array_equal(G.interior(got[i], r), G.interior(want, r)), (names[i], kind, r, op)


def test_box_mean_and_corrected_definitions():
    rng = np.random.default_rng(5)
    b = rng.integers(0, 4096, size=(9, 11)).astype(np.int16)
    for s in (0, 1, 2, 5, 16):
        assert np.array_equal(G.box_mean(b, s), G.box_mean_brute(b, s)), s
    assert np.array_equal(G.box_mean(b[None], 2)[0], G.box_mean_brute(b, 2))
    assert np.array_equal(G.box_mean(np.full((4, 5), 7, np.int16), 3), np.full((4, 5), 7))
    # nothing subtracted: the counts of the histogram restatement
    import stain_calibrate_ref as C
    import stain_quant_ref as Q
    u8 = rng.integers(0, 256, size=(2, 12, 13, 3), dtype=np.uint8)
    m32 = np.linalg.inv(Q.stain_matrix("hdab")).astype(np.float32)
    c = G.corrected(u8, m32, None, 205)
    hist, tissue = C.histogram(u8, m32)
    assert np.array_equal(c["hist"][:, 1], hist[:, 1]) and np.array_equal(c["tissue"], tissue)
    assert (c["hist"][:, 0] == 0).all() and (c["hist"][:, 2] == 0).all()
    assert np.array_equal(c["positive"], hist[:, 1, 205:].sum(1))
    c5 = G.corrected(u8, m32, 3, 100, smooth=1)
    assert np.array_equal(c5["positive"], c5["hist"][:, 1, 100:].sum(1)) and (c5["corrected"] <= c5["bins"]).all()
    assert np.array_equal(c5["mask"] & 1, ((c5["corrected"] >= 100) & (c5["mask"] >> 1 == 1)).astype(np.uint8))
    p = G.corrected(u8, m32, 3, 100, smooth=1, pool=True)
    assert np.array_equal(p["hist"][0], c5["hist"].sum(0)) and p["positive"][0] == c5["positive"].sum()
    z = np.full((1, 6, 6, 3), 255, np.uint8)
    a = G.agreement(z, z, m32, 2, 205)
    assert a["dice"][0] == 1.0 and a["iou"][0] == 1.0 and a["burden_abs_err"][0] == 0.0


# ---- exports ----------------------------------------------------------------------------------------------------------
def test_exports():
    import stain2stain_amd
    from stain2stain_amd import _native, background
    for name in PUBLIC:
        assert name in stain2stain_amd.__all__ and getattr(stain2stain_amd, name) is getattr(background, name)
    assert "grey_morph.hip" in _native.SOURCES
    declared = _native.declared_symbols()
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in declared and hasattr(lib, sym), sym
    assert background.MAX_RADIUS >= 128 and background.MAX_SIDE == 32767 and background.MAX_BATCH == 65535
    src = open(_native.CSRC + "/grey_morph.hip").read()
    assert f"GM_MAX_RADIUS = {background.MAX_RADIUS};" in src and f"GM_MAX_SMOOTH = {background.MAX_SMOOTH};" in src


# ---- status codes of the entry points: returned before any HIP call ---------------------------------------------------
def test_entry_points_return_status_codes():
    from stain2stain_amd import _native, background
    lib = _native.lib()
    X = 4096                                      # a non-null pointer that is never dereferenced: every call below fails first
    R2 = background.MAX_RADIUS ** 2
    words = lib.s2s_grey_words
    # radius 2: spans up to 5 pixels, tables k = 0..2, plus the intermediate plane: 4 int16 planes
    assert words(1, 64, 64, 0, 4) == 4 * 64 * 64 // 2 and words(3, 5, 7, 1, 0) == (2 * 105 + 1) // 2
    assert words(1, 9, 3, 0, R2) == 3 * 27 // 2 + 1                       # spans clipped to W = 3: k = 0..1
    assert words(1, 300, 300, 0, R2) == 10 * 90000 // 2 and words(1, 300, 300, 1, 128) == 10 * 90000 // 2
    assert words(0, 8, 8, 0, 4) == -1 and words(65536, 8, 8, 0, 4) == -1 and words(1, 0, 8, 0, 4) == -1
    assert words(1, 8, 32768, 0, 4) == -1 and words(1, 32768, 8, 0, 4) == -1 and words(1, 32767, 32767, 0, 4) > 0
    assert words(1, 8, 8, 0, R2 + 1) == -1 and words(1, 8, 8, 1, 129) == -1 and words(1, 8, 8, 0, -1) == -1
    assert words(1, 8, 8, 2, 4) == -1

    def morph(src=X, dtype=1, pitch=64, img=64 * 32, B=1, H=32, W=64, op=2, fp=0, size=25, scratch=X, out=X):
        return lib.s2s_grey_morph(src, dtype, pitch, img, B, H, W, op, fp, size, scratch, out, None)

    assert morph(src=0) == -5 and morph(scratch=0) == -5 and morph(out=0) == -5
    assert morph(dtype=2) == -3 and morph(dtype=-1) == -3
    assert morph(B=0) == -1 and morph(B=65536) == -1 and morph(H=0) == -1 and morph(W=-1) == -1 and morph(pitch=63) == -1
    assert morph(B=2, img=64 * 31) == -1 and morph(H=32768) == -1 and morph(W=32768, pitch=32768) == -1
    assert morph(op=-1) == -1 and morph(op=6) == -1 and morph(fp=2) == -1 and morph(size=-1) == -1
    assert morph(size=R2 + 1) == -1 and morph(fp=1, size=background.MAX_RADIUS + 1) == -1

    def mean(src=X, B=1, H=32, W=64, smooth=2, out=X):
        return lib.s2s_grey_box_mean(src, B, H, W, smooth, out, None)

    assert mean(src=0) == -5 and mean(out=0) == -5
    assert mean(B=0) == -1 and mean(H=32768) == -1 and mean(W=0) == -1 and mean(smooth=-1) == -1
    assert mean(smooth=background.MAX_SMOOTH + 1) == -1

    import ctypes
    od, m = (ctypes.c_float * 256)(), (ctypes.c_float * 12)()

    def bins_u8(img=X, pitch=192, stride=192 * 32, B=1, rows=32, W=64, od=od, m=m, white=220, black=0, stain=1, bins=X,
                tissue=X):
        return lib.s2s_grey_bins_u8(img, pitch, stride, B, rows, W, od, m, white, black, stain, bins, tissue, None)

    def bins_f32(img=X, B=1, H=32, W=64, od=od, m=m, white=220, black=0, stain=1, bins=X, tissue=X):
        return lib.s2s_grey_bins_f32(img, B, H, W, od, m, white, black, stain, bins, tissue, None)

    for f in (bins_u8, bins_f32):
        assert f(img=0) == -5 and f(bins=0) == -5 and f(od=None) == -5 and f(m=None) == -5
        assert f(B=0) == -1 and f(B=65536) == -1 and f(W=0) == -1 and f(W=32768) == -1 and f(stain=3) == -1
        assert f(stain=-1) == -1 and f(white=0) == -1 and f(white=257) == -1 and f(black=-1) == -1 and f(black=256) == -1
    assert bins_u8(rows=0) == -1 and bins_u8(rows=32768) == -1 and bins_u8(pitch=191) == -1
    assert bins_u8(B=2, stride=192 * 31) == -1 and bins_f32(H=0) == -1 and bins_f32(H=32768) == -1

    def corr(bins=X, bg=X, tissue=X, B=1, rows=32, W=64, row0=0, nrows=32, j=205, stain=1, pool=0, reset=1, counts=X,
             hist=X, mask=X, corrected=X, out_img=32 * 64):
        return lib.s2s_grey_corrected(bins, bg, tissue, B, rows, W, row0, nrows, j, stain, pool, reset, counts, hist, mask,
                                      corrected, out_img, None)

    assert corr(bins=0) == -5 and corr(tissue=0) == -5 and corr(counts=0) == -5 and corr(hist=0) == -5
    assert corr(B=0) == -1 and corr(B=65536) == -1 and corr(rows=0) == -1 and corr(W=32768) == -1
    assert corr(row0=-1) == -1 and corr(nrows=0) == -1 and corr(row0=1) == -1 and corr(nrows=33) == -1
    assert corr(j=0) == -1 and corr(j=4096) == -1 and corr(stain=3) == -1 and corr(stain=-1) == -1
    assert corr(B=2, out_img=32 * 64 - 1) == -1
    assert corr(B=65535, rows=32767, W=32767, nrows=32767, pool=1, out_img=32767 * 32767) == -1   # 2^32 pixels a workgroup

    fin = lib.s2s_grey_corrected_finalize
    assert fin(0, 1, X, None) == -5 and fin(X, 1, 0, None) == -5 and fin(X, 0, X, None) == -1 and fin(X, 65536, X, None) == -1

    def pair(a=X, b=X, B=1, H=32, W=64, both=X):
        return lib.s2s_grey_pair(a, b, B, H, W, both, None)

    assert pair(a=0) == -5 and pair(b=0) == -5 and pair(both=0) == -5
    assert pair(B=0) == -1 and pair(B=65536) == -1 and pair(H=0) == -1 and pair(W=32768) == -1
    pf = lib.s2s_grey_pair_finalize
    assert pf(0, X, X, 1, X, None) == -5 and pf(X, 0, X, 1, X, None) == -5 and pf(X, X, 0, 1, X, None) == -5
    assert pf(X, X, X, 1, 0, None) == -5 and pf(X, X, X, 0, X, None) == -1 and pf(X, X, X, 65536, X, None) == -1


# ---- argument checks that need no GPU ---------------------------------------------------------------------------------
def test_wrappers_reject_before_the_gpu():
    from stain2stain_amd import (concentration_bins, grey_morphology, region_stain_quantify_corrected,
                                 stain_agreement_corrected, stain_background, stain_objects_corrected,
                                 stain_quantify_corrected)
    from stain2stain_amd.background import MAX_RADIUS, MAX_SMOOTH
    x = torch.zeros((2, 16, 16), dtype=torch.int16)
    with pytest.raises(TypeError):
        grey_morphology(x.numpy(), "open", 2)
    for bad in (x.float(), x.int(), x.bool(), x[0, 0], x[None], torch.zeros((0, 4, 4), dtype=torch.uint8),
                torch.zeros((2, 0, 4), dtype=torch.int16), torch.zeros((1, 1), dtype=torch.uint8).expand(32768, 4),
                torch.zeros((1, 1), dtype=torch.uint8).expand(4, 32768)):
        with pytest.raises(ValueError):
            grey_morphology(bad, "open", 2)
    for op, r, fp in (("shrink", 2, "disc"), ("open", -1, "disc"), ("open", float("nan"), "disc"),
                      ("dilate", float("inf"), "square"), ("open", 2, "diamond"), ("open", MAX_RADIUS + 0.5, "disc"),
                      ("erode", MAX_RADIUS + 1, "square")):
        with pytest.raises(ValueError):
            grey_morphology(x, op, r, fp)
    for r in (None, "2", [2]):
        with pytest.raises(TypeError):
            grey_morphology(x, "open", r)

    tiles = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    region = tiles[0]
    calls = [lambda **kw: stain_quantify_corrected(tiles, **kw), lambda **kw: stain_objects_corrected(tiles, **kw),
             lambda **kw: stain_agreement_corrected(tiles, tiles, **kw),
             lambda **kw: region_stain_quantify_corrected(region, **kw)]
    for f in calls:
        for thr in (0.2, 0.0, 4.0, 205.5 / 1024, float("nan"), -205 / 1024):          # off the grid
            with pytest.raises(ValueError):
                f(radius=4, threshold=thr)
        for kw in ({"radius": -1}, {"radius": float("nan")}, {"radius": float("inf")}, {"radius": MAX_RADIUS + 1},
                   {"radius": 4, "smooth": -1}, {"radius": 4, "smooth": MAX_SMOOTH + 1}, {"radius": 4, "stain": 3},
                   {"radius": 4, "footprint": "ball"}, {"radius": 4, "white": 0}):
            with pytest.raises(ValueError):
                f(threshold=205 / 1024, **kw)
        for kw in ({"radius": "4"}, {"radius": 4, "smooth": 1.5}, {"radius": 4, "smooth": float("nan")}):
            with pytest.raises(TypeError):
                f(threshold=205 / 1024, **kw)
    for f in (lambda t: stain_quantify_corrected(t, 4), lambda t: stain_objects_corrected(t, 4),
              lambda t: stain_background(t, 4), concentration_bins, lambda t: stain_agreement_corrected(t, t, 4)):
        with pytest.raises(TypeError):
            f(tiles.numpy())
        for bad in (tiles[0], tiles[..., :2], tiles.to(torch.int16), tiles.double()):
            with pytest.raises(ValueError):
                f(bad)
    with pytest.raises(TypeError):
        stain_background(tiles, None)
    with pytest.raises(ValueError):
        stain_background(tiles, -2)
    with pytest.raises(ValueError):
        stain_agreement_corrected(tiles, tiles[:1], 4)
    with pytest.raises(TypeError):
        region_stain_quantify_corrected(region.numpy(), 4)
    for bad in (tiles, region[..., 0], region.float()):
        with pytest.raises(ValueError):
            region_stain_quantify_corrected(bad, 4)
    for br in (0, -3):
        with pytest.raises(ValueError):
            region_stain_quantify_corrected(region, 4, band_rows=br)
    with pytest.raises(ValueError):
        stain_objects_corrected(tiles, 4, connectivity=6)
    with pytest.raises(ValueError):
        stain_objects_corrected(tiles, 4, min_area=0)
