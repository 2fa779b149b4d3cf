"""Stain object analysis without a GPU: the scipy restatement (tests/objects_ref.py) against a pure-Python flood fill that
numbers objects by first raster pixel by construction, the exports, the status codes of the new entry points (returned
before any HIP call) and the argument checks the wrappers make before they touch the device."""
import ctypes

import numpy as np
import pytest
import torch

import objects_ref as O

NEW_SYMBOLS = ["s2s_objects_words", "s2s_objects_hit_words", "s2s_objects_label", "s2s_objects_centroid",
               "s2s_objects_hits", "s2s_objects_scores", "s2s_objects_density", "s2s_stain_mask_u8", "s2s_stain_mask_f32"]


def _masks():
    d1, d2 = O.diagonals(23)
    yield "empty", np.zeros((7, 9), np.uint8)
    yield "full", np.ones((7, 9), np.uint8)
    yield "pixel", np.ones((1, 1), np.uint8)
    yield "row", O.bernoulli((1, 9), 0.5, 1)
    yield "column", O.bernoulli((5, 1), 0.5, 2)
    yield "serpentine", O.serpentine(21, 13)
    yield "serpentine even", O.serpentine(20, 7)
    yield "checkerboard", O.checkerboard(9, 11)
    yield "diagonal", d1
    yield "anti-diagonal", d2
    for seed, p in enumerate((0.3, 0.41, 0.5, 0.59, 0.7)):
        yield f"bernoulli {p}", O.bernoulli((31, 37), p, 10 + seed)


# ---- the reference against the flood fill -----------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_scipy_numbers_objects_by_first_raster_pixel(connectivity):
    for name, m in _masks():
        lab, n, area = O.label(m, connectivity)
        want, nw = O.flood_label(m, connectivity)
        assert n == nw and np.array_equal(lab, want), (name, connectivity)
        assert np.array_equal(area, np.bincount(want.ravel(), minlength=nw + 1)[1:]), (name, connectivity)
        # the first pixels of the objects, in raster order, carry 1, 2, 3, ...
        first = [int(np.flatnonzero(want.ravel() == k)[0]) for k in range(1, nw + 1)]
        assert first == sorted(first), (name, connectivity)


def test_reference_closed_forms():
    assert O.label(O.serpentine(97, 131), 4)[1] == 1 and O.label(O.serpentine(200, 70), 8)[1] == 1
    assert O.label(O.checkerboard(65, 67), 8)[1] == 1 and O.label(O.checkerboard(65, 67), 4)[1] == 2178
    d1, d2 = O.diagonals(130)
    for d in (d1, d2):
        assert O.label(d, 8)[1] == 1 and O.label(d, 4)[1] == 130
    # filter, then renumber: the survivors keep their order
    m = np.zeros((5, 12), np.uint8)
    m[0, 0] = 1                      # area 1
    m[0, 3:6] = 1                    # area 3
    m[2, 0:2] = 1                    # area 2
    m[3:5, 8:12] = 1                 # area 8
    c = O.components(m, 8, min_area=2, max_objects=4)
    assert c["count"] == 3 and c["kept_pixels"] == 13 and c["largest"] == 8
    assert c["labels"][0, 0] == 0 and c["labels"][0, 4] == 1 and c["labels"][2, 1] == 2 and c["labels"][4, 11] == 3
    assert c["size_hist"][1] == 2 and c["size_hist"][3] == 1 and c["size_hist"].sum() == 3
    assert c["area"].tolist() == [3, 2, 8, 0]
    assert c["bbox"].tolist() == [[0, 3, 1, 6], [2, 0, 3, 2], [3, 8, 5, 12], [0, 0, 0, 0]]
    assert c["centroid"].tolist() == [[0.0, 4.0], [2.0, 0.5], [3.5, 9.5], [0.0, 0.0]]
    assert O.components(m, 8, max_objects=2)["area"].tolist() == [1, 3] and O.components(m, 8, min_area=9)["count"] == 0
    # hits and the empty-count conventions
    a, na, _ = O.label(m, 8)
    t = np.zeros_like(m)
    t[0, 5:8] = 1                    # touches the area-3 object only
    t[4, 0] = 1                      # touches nothing
    b, nb, _ = O.label(t, 8)
    assert O.touched(a, b) == (1, 1)
    s = O.agreement(a, na, b, nb)
    assert s["recall"] == np.float32(0.5) and s["precision"] == np.float32(0.25) and s["count_abs_err"] == 2
    assert s["f1"] == np.float32(2 * 0.25 * 0.5 / 0.75)
    z = np.zeros_like(a)
    e = O.agreement(z, 0, z, 0)
    assert e["recall"] == 1 and e["precision"] == 1 and e["f1"] == 1
    e = O.agreement(a, na, z, 0)
    assert e["recall"] == 0 and e["precision"] == 0 and e["f1"] == 0
    e = O.agreement(z, 0, b, nb)
    assert e["recall"] == 0 and e["precision"] == 0 and e["f1"] == 0


# ---- exports ----------------------------------------------------------------------------------------------------------
def test_exports():
    import stain2stain_amd
    from stain2stain_amd import _native, objects
    for name in ("label_components", "stain_objects", "stain_object_agreement", "region_stain_objects"):
        assert name in stain2stain_amd.__all__ and getattr(stain2stain_amd, name) is getattr(objects, name)
    assert "objects.hip" in _native.SOURCES
    declared = _native.declared_symbols()
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in declared and hasattr(lib, sym), sym
    assert objects.MAX_PIXELS == 2 ** 31 - 2 and objects.TILE == (32, 64)


# ---- status codes of the entry points: returned before any HIP call ---------------------------------------------------
def test_entry_points_return_status_codes():
    from stain2stain_amd import _native
    lib = _native.lib()
    X = 4096                                      # a non-null pointer that is never dereferenced: every call below fails first
    assert lib.s2s_objects_words(1, 32, 64) == 32 * 64 + 2 and lib.s2s_objects_words(3, 33, 65) == 3 * (33 * 65 + 3)
    assert lib.s2s_objects_words(0, 8, 8) == -1 and lib.s2s_objects_words(1, 0, 8) == -1 and lib.s2s_objects_words(1, 8, -1) == -1
    assert lib.s2s_objects_words(1, 65536, 32768) == -1 and lib.s2s_objects_words(1, 2 ** 31 - 2, 1) > 0
    assert lib.s2s_objects_words(65536, 8, 8) == -1
    assert lib.s2s_objects_hit_words(2, 8, 8) == 2 * 2 * 2 and lib.s2s_objects_hit_words(1, 65536, 32768) == -1

    def label(mask=X, pitch=64, img=64 * 32, fg=255, B=1, H=32, W=64, conn=8, min_area=1, M=0, scratch=X, labels=X, count=X,
              kept=X, largest=X, hist=X, ta=0, tb=0, ts=0):
        return lib.s2s_objects_label(mask, pitch, img, fg, B, H, W, conn, min_area, M, scratch, labels, count, kept, largest,
                                     hist, ta, tb, ts, None)

    for name in ("mask", "scratch", "labels", "count", "kept", "largest", "hist"):
        assert label(**{name: 0}) == -5, name
    assert label(M=4) == -5 and label(M=4, ta=X, tb=X) == -5 and label(M=4, ta=X, ts=X) == -5
    assert label(B=0) == -1 and label(B=65536) == -1 and label(H=0) == -1 and label(W=-1) == -1
    assert label(H=65536, W=32768, pitch=32768) == -1
    assert label(conn=6) == -1 and label(conn=0) == -1 and label(min_area=0) == -1 and label(M=-1) == -1
    assert label(fg=0) == -1 and label(fg=256) == -1 and label(pitch=63) == -1 and label(B=2, img=64 * 31) == -1

    cen = lib.s2s_objects_centroid
    assert cen(0, X, X, 1, 4, X, None) == -5 and cen(X, 0, X, 1, 4, X, None) == -5 and cen(X, X, 0, 1, 4, X, None) == -5
    assert cen(X, X, X, 1, 4, 0, None) == -5 and cen(X, X, X, 0, 4, X, None) == -1 and cen(X, X, X, 1, 0, X, None) == -1

    hits = lib.s2s_objects_hits
    assert hits(0, X, 1, 8, 8, X, X, None) == -5 and hits(X, 0, 1, 8, 8, X, X, None) == -5
    assert hits(X, X, 1, 8, 8, 0, X, None) == -5 and hits(X, X, 1, 8, 8, X, 0, None) == -5
    assert hits(X, X, 0, 8, 8, X, X, None) == -1 and hits(X, X, 1, 0, 8, X, X, None) == -1
    assert hits(X, X, 1, 65536, 32768, X, X, None) == -1

    sc = lib.s2s_objects_scores
    assert sc(0, X, X, 1, X, X, None) == -5 and sc(X, 0, X, 1, X, X, None) == -5 and sc(X, X, 0, 1, X, X, None) == -5
    assert sc(X, X, X, 1, 0, X, None) == -5 and sc(X, X, X, 1, X, 0, None) == -5 and sc(X, X, X, 0, X, X, None) == -1

    den = lib.s2s_objects_density
    k, bad = (ctypes.c_double * 1)(0.25e-6), (ctypes.c_double * 1)(0.0)
    assert den(0, X, X, 1, None, X, 0, None) == -5 and den(X, 0, X, 1, None, X, 0, None) == -5
    assert den(X, X, 0, 1, None, X, 0, None) == -5 and den(X, X, X, 1, None, 0, 0, None) == -5
    assert den(X, X, X, 1, k, X, 0, None) == -5 and den(X, X, X, 0, None, X, 0, None) == -1
    assert den(X, X, X, 1, bad, X, X, None) == -1

    od, um = (ctypes.c_float * 256)(), (ctypes.c_float * 12)()

    def mu8(img=X, pitch=96, B=1, band_top=0, band_h=32, H=32, W=32, od=od, um=um, white=220, black=0, stain=1, mask=X,
            mpitch=32, mimg=32 * 32, tissue=X):
        return lib.s2s_stain_mask_u8(img, pitch, pitch * band_h, B, band_top, band_h, H, W, od, um, white, black, stain, mask,
                                     mpitch, mimg, tissue, None)

    assert mu8(img=0) == -5 and mu8(mask=0) == -5 and mu8(tissue=0) == -5 and mu8(od=None) == -5 and mu8(um=None) == -5
    assert mu8(B=0) == -1 and mu8(H=0) == -1 and mu8(W=-1) == -1 and mu8(pitch=95) == -1 and mu8(mpitch=31) == -1
    assert mu8(band_h=0) == -1 and mu8(band_h=33) == -1 and mu8(band_top=1) == -1 and mu8(band_top=-1) == -1
    assert mu8(white=0) == -1 and mu8(black=256) == -1 and mu8(stain=3) == -1 and mu8(B=2, mimg=32 * 31) == -1

    def mf32(img=X, B=1, H=8, W=8, od=od, um=um, stain=1, mask=X, mpitch=8, mimg=64, tissue=X):
        return lib.s2s_stain_mask_f32(img, B, H, W, od, um, 220, 0, stain, mask, mpitch, mimg, tissue, None)

    assert mf32(img=0) == -5 and mf32(mask=0) == -5 and mf32(tissue=0) == -5 and mf32(od=None) == -5
    assert mf32(B=0) == -1 and mf32(H=0) == -1 and mf32(mpitch=7) == -1 and mf32(stain=-1) == -1 and mf32(B=2, mimg=63) == -1


# ---- argument checks that need no GPU --------------------------------------------------------------------------------
def test_label_components_rejects():
    from stain2stain_amd import label_components
    m = torch.zeros((2, 16, 16), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        label_components(m)
    with pytest.raises(RuntimeError, match="GPU"):
        label_components(m[0] > 0)
    with pytest.raises(TypeError):
        label_components(m.numpy())
    for bad in (m.float(), m.int(), m[0, 0], m[None], torch.zeros((0, 4, 4), dtype=torch.bool),
                torch.zeros((2, 0, 4), dtype=torch.bool)):
        with pytest.raises(ValueError):
            label_components(bad)
    for kw in ({"connectivity": 6}, {"connectivity": 0}, {"min_area": 0}, {"min_area": -3}, {"max_objects": 0},
               {"max_objects": -1}):
        with pytest.raises(ValueError):
            label_components(m, **kw)
    with pytest.raises(TypeError):
        label_components(m, min_area=1.5)
    with pytest.raises(TypeError):
        label_components(m, connectivity="8")


def test_stain_wrappers_reject():
    from stain2stain_amd import stain_object_agreement, stain_objects
    u = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    f = torch.zeros((2, 3, 16, 16))
    for t in (u, f):
        with pytest.raises(RuntimeError, match="GPU"):
            stain_objects(t)
        with pytest.raises(RuntimeError, match="GPU"):
            stain_object_agreement(t, t.clone())
    with pytest.raises(TypeError):
        stain_objects(u.numpy())
    for bad in (torch.zeros((2, 16, 16, 4), dtype=torch.uint8), torch.zeros((16, 16, 3), dtype=torch.uint8), f.double(),
                torch.zeros((2, 4, 16, 16))):
        with pytest.raises(ValueError):
            stain_objects(bad)
    for kw in ({"stain": 3}, {"stains": "he"}, {"thresholds": (0.1, 0.2)}, {"white": 0}, {"black": 256},
               {"connectivity": 5}, {"min_area": 0}, {"max_objects": 0}, {"mpp": 0.0}, {"mpp": -0.5},
               {"mpp": float("nan")}):
        with pytest.raises(ValueError):
            stain_objects(u, **kw)
    for kw in ({"stain": -1}, {"thresholds": 0.2}, {"connectivity": 2}, {"min_area": 0}):
        with pytest.raises(ValueError):
            stain_object_agreement(u, u.clone(), **kw)
    with pytest.raises(ValueError):
        stain_object_agreement(u, u[:, :15])
    with pytest.raises(ValueError):
        stain_object_agreement(u, f)
    with pytest.raises(TypeError):
        stain_object_agreement(u, None)


def test_region_wrapper_rejects_and_names_the_pixel_limit():
    from stain2stain_amd import region_stain_objects
    from stain2stain_amd.objects import MAX_PIXELS, _check_pixels
    r = torch.zeros((40, 40, 3), dtype=torch.uint8)
    with pytest.raises(TypeError):
        region_stain_objects(None)
    for bad in (r.float(), r[..., :2], r[:, ::2], r[None]):
        with pytest.raises(ValueError):
            region_stain_objects(bad)
    for kw in ({"stain": 5}, {"thresholds": (0.1,)}, {"connectivity": 3}, {"min_area": 0}, {"max_objects": 0},
               {"mpp": 0}, {"band_rows": 8}):
        with pytest.raises(ValueError):
            region_stain_objects(r, **kw)
    # the limit, without allocating 2 GiB: a region of 2^31 pixels whose rows all alias one row
    row = torch.zeros((1, 32768, 3), dtype=torch.uint8)
    huge = row.expand(65536, 32768, 3)
    assert huge.shape[0] * huge.shape[1] == MAX_PIXELS + 2
    with pytest.raises(ValueError, match=r"2\^31 - 2"):
        region_stain_objects(huge)
    _check_pixels(2 ** 31 - 2, 1, "x")
    _check_pixels(46340, 46340, "x")
    with pytest.raises(ValueError, match=str(MAX_PIXELS)):
        _check_pixels(2 ** 31 - 1, 1, "x")
    with pytest.raises(ValueError, match="label_components"):
        from stain2stain_amd import label_components
        label_components(torch.zeros((1, 1), dtype=torch.bool).expand(65536, 32768))
