"""Mask morphology without a GPU: the restatement of tests/morphology_ref.py against itself (brute force, scipy's nearest-site
indices, scipy's binary morphology with true discs, binary_fill_holes), the degenerate rules of the boundary agreement, the
exports, the status codes of the s2s_morph_* entry points (returned before any HIP call) and the argument checks the
wrappers make before they touch the device."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

import morphology_ref as M

SHAPES = [(1, 1), (1, 9), (5, 1), (63, 65), (129, 131), (97, 131)]
SMALL = [(1, 1), (1, 9), (5, 1), (23, 31)]
RADII = (0, 1, 1.5, 2, 5)
RADIUS_BEYOND = 40          # larger than the diagonal of every SMALL shape (a 81 x 81 disc: small shapes only)
NEW_SYMBOLS = ["s2s_morph_words", "s2s_morph_fill_holes_words", "s2s_morph_edt", "s2s_morph_threshold", "s2s_morph_boundary",
               "s2s_morph_fill_holes", "s2s_morph_boundary_agreement", "s2s_morph_boundary_finalize"]


# ---- the reference against itself -------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SMALL)
def test_indices_equal_brute_force(H, W):
    for name, m in M.patterns(H, W, seed=H * W):
        for to in ("background", "foreground"):
            assert np.array_equal(M.d2_indices(m, to), M.d2_brute(m, to)), (name, to)


@pytest.mark.parametrize("H,W", SHAPES + SMALL[-1:])
def test_thresholds_equal_scipy_morphology(H, W):
    for name, m in M.patterns(H, W, seed=H + W):
        if name.startswith("corner") and name != "corner 3":
            continue
        for r in RADII + ((RADIUS_BEYOND,) if (H, W) in SMALL else ()):
            assert np.array_equal(M.dilate(m, r), M.scipy_dilate(m, r)), (name, r)
            assert np.array_equal(M.erode(m, r), M.scipy_erode(m, r)), (name, r)


def test_max_dist_and_far():
    m = M.corners(9, 12)[0]
    d = M.d2(m, "foreground")
    assert d[8, 11] == 64 + 121 and d[0, 0] == 0
    cut = M.d2(m, "foreground", max_dist=4.5)
    assert np.array_equal(cut, np.where(d > 20, M.FAR, d)) and (cut == M.FAR).any()
    assert (M.d2(np.ones((4, 5), np.uint8), "background") == M.FAR).all()
    assert (M.d2(np.zeros((4, 5), np.uint8), "foreground") == M.FAR).all()
    assert (M.d2(np.zeros((4, 5), np.uint8), "background") == 0).all()


def test_fill_holes_equals_scipy():
    cases = [M.ring(40, 50, 20, 25, 12, 6), M.ring(40, 50, 8, 25, 12, 6), M.bernoulli((31, 37), 0.6, 4),
             M.ring(60, 60, 30, 30, 25, 20) | M.ring(60, 60, 30, 30, 12, 6), np.zeros((5, 5), np.uint8),
             np.ones((5, 5), np.uint8)]
    for m in cases:
        assert np.array_equal(M.fill_holes(m, 4), ndimage.binary_fill_holes(m).astype(np.uint8))
        assert np.array_equal(M.fill_holes(m, 8), ndimage.binary_fill_holes(m, M.SQUARE).astype(np.uint8))
    ringed = M.ring(40, 50, 20, 25, 12, 6)
    assert M.fill_holes(ringed)[20, 25] == 1 and M.fill_holes(ringed).sum() == M.discs(40, 50, [(20, 25, 12)]).sum()
    # a hole that reaches the outside through a diagonal gap only: a hole for 4-connected background, open for 8
    m = np.ones((7, 7), np.uint8)
    m[3, 3] = m[2, 2] = m[1, 1] = m[0, 0] = 0
    assert M.fill_holes(m, 4)[3, 3] == 1 and M.fill_holes(m, 8)[3, 3] == 0 and M.fill_holes(m, 4)[0, 0] == 0


def test_boundary_rule():
    m = np.ones((5, 6), np.uint8)
    b = M.boundary(m)
    assert b.sum() == 2 * 6 + 2 * 3 and b[2, 2] == 0 and b[0, 0] == 1
    m[2, 3] = 0
    b = M.boundary(m)
    assert b[2, 2] == 1 and b[1, 3] == 1 and b[2, 3] == 0 and b[1, 2] == 0      # 4-neighbours only
    assert M.boundary(np.zeros((3, 3), np.uint8)).sum() == 0
    assert M.boundary(np.ones((1, 1), np.uint8)).sum() == 1


def test_agreement_definitions_and_degenerate_rules():
    H, W = 40, 50
    a = M.discs(H, W, [(20, 25, 8)])
    same = M.agreement(a, a)
    assert all(same[k] == 0 for k in ("max_d2", "pq_d2", "sum_q8")) and same["surface_dice"] == 1 and same["valid"] == 1
    assert same["within"] == same["boundary_pred"] + same["boundary_target"]
    z = np.zeros_like(a)
    both = M.agreement(z, z)
    assert all(both[k] == 0 for k in M.INT_KEYS) and both["surface_dice"] == 1 and both["assd"] == 0 and both["hd"] == 0
    far = (H - 1) ** 2 + (W - 1) ** 2
    for one in (M.agreement(a, z), M.agreement(z, a)):
        n = int(one["boundary_pred"] + one["boundary_target"])
        assert n == int(M.boundary(a).sum()) and one["max_d2"] == far and one["pq_d2"] == far and one["within"] == 0
        assert one["sum_q8"] == n * math.isqrt(65536 * far) and one["valid"] == 0 and one["surface_dice"] == 0
        assert all(np.isfinite(one[k]) for k in M.F64_KEYS)
    # shifted by (3, 4): every directed distance is at most 5
    big = np.zeros((60, 70), np.uint8)
    big[20:40, 20:45] = 1
    sh = np.roll(big, (3, 4), axis=(0, 1))
    s = M.agreement(big, sh, tolerance=5)
    assert s["max_d2"] <= 25 and s["surface_dice"] == 1 and s["hd"] <= 5
    # percentile 100 is the maximum; the sum is within 1/256 pixel per element of the float sum
    b = M.discs(H, W, [(20, 25, 13)])
    S, n_p, n_t = M.pooled(a, b)
    s = M.agreement(a, b, percentile=100)
    assert s["pq_d2"] == s["max_d2"] == S.max() and s["hausdorff"] == s["hd"]
    assert 0 <= np.sqrt(S.astype(np.float64)).mean() - s["assd"] < 1 / 256
    assert M.agreement(a, b, percentile=1)["pq_d2"] == np.sort(S)[(1 * S.size + 99) // 100 - 1]
    assert M.agreement(a, b, tolerance=0)["within"] == (S == 0).sum()
    assert M.agreement(a, b, tolerance=4.5)["within"] == (S <= 20).sum()


# ---- exports ----------------------------------------------------------------------------------------------------------
def test_exports():
    import stain2stain_amd
    from stain2stain_amd import _native, morphology
    for name in ("distance_transform", "mask_morphology", "fill_holes", "mask_boundary", "mask_boundary_agreement"):
        assert name in stain2stain_amd.__all__ and getattr(stain2stain_amd, name) is getattr(morphology, name)
    assert "morphology.hip" in _native.SOURCES
    declared = _native.declared_symbols()
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in declared and hasattr(lib, sym), sym
    assert morphology.FAR == 2 ** 31 - 1 and morphology.MAX_SIDE == 32767 and morphology.SEGMENT == 64
    assert morphology.PACK_WIDTH == 512
    assert morphology.MAX_SIDE ** 2 * 2 < 2 ** 31


# ---- status codes of the entry points: returned before any HIP call ---------------------------------------------------
def test_entry_points_return_status_codes():
    from stain2stain_amd import _native
    lib = _native.lib()
    X = 4096                                      # a non-null pointer that is never dereferenced: every call below fails first
    words = lib.s2s_morph_words
    # bits 2, carries 2 words per column and segment, g half a word per pixel; the agreement adds 16 + 2048 words per sample
    # and two lists of H W
    assert words(1, 64, 64, 0) == 4 * 64 + 64 * 64 // 2 and words(3, 65, 7, 0) == 3 * 2 * 7 * 4 + (3 * 65 * 7 + 1) // 2
    assert words(2, 10, 10, 1) == 2 * 2064 + 2 * 10 * 4 + 100 + 2 * 2 * 100
    assert words(0, 8, 8, 0) == -1 and words(1, 0, 8, 0) == -1 and words(1, 8, -1, 0) == -1 and words(65536, 8, 8, 0) == -1
    assert words(1, 32768, 8, 0) == -1 and words(1, 8, 32768, 1) == -1 and words(1, 32767, 32767, 1) > 0
    fw = lib.s2s_morph_fill_holes_words
    assert fw(1, 32768, 8) == -1 and fw(0, 8, 8) == -1 and fw(2, 10, 10) == 2 * 68 + 2 * 2 + 200 + 50 + lib.s2s_objects_words(2, 10, 10)

    def edt(mask=X, pitch=64, img=64 * 32, B=1, H=32, W=64, fg=0, md2=7, scratch=X, out=X):
        return lib.s2s_morph_edt(mask, pitch, img, B, H, W, fg, md2, scratch, out, None)

    def thr(mask=X, pitch=64, img=64 * 32, B=1, H=32, W=64, erode=0, r2=7, scratch=X, out=X):
        return lib.s2s_morph_threshold(mask, pitch, img, B, H, W, erode, r2, scratch, out, None)

    def bnd(mask=X, pitch=64, img=64 * 32, B=1, H=32, W=64, out=X):
        return lib.s2s_morph_boundary(mask, pitch, img, B, H, W, out, None)

    def holes(mask=X, pitch=64, img=64 * 32, B=1, H=32, W=64, conn=4, scratch=X, out=X):
        return lib.s2s_morph_fill_holes(mask, pitch, img, B, H, W, conn, scratch, out, None)

    for f in (edt, thr, holes):
        assert f(mask=0) == -5 and f(scratch=0) == -5 and f(out=0) == -5
    assert bnd(mask=0) == -5 and bnd(out=0) == -5
    for f in (edt, thr, bnd, holes):
        assert f(B=0) == -1 and f(B=65536) == -1 and f(H=0) == -1 and f(W=-1) == -1 and f(pitch=63) == -1
        assert f(B=2, img=64 * 31) == -1 and f(H=32768) == -1 and f(W=32768, pitch=32768) == -1
    assert edt(md2=-1) == -1 and edt(fg=2) == -1 and thr(r2=-1) == -1 and thr(r2=2 ** 31 - 1) == -1 and thr(erode=2) == -1
    assert holes(conn=6) == -1 and holes(conn=0) == -1

    def agree(p=X, pp=64, pi=64 * 32, t=X, tp=64, ti=64 * 32, B=1, H=32, W=64, tol2=4, q=95, scratch=X):
        return lib.s2s_morph_boundary_agreement(p, pp, pi, t, tp, ti, B, H, W, tol2, q, scratch, None)

    assert agree(p=0) == -5 and agree(t=0) == -5 and agree(scratch=0) == -5
    assert agree(B=0) == -1 and agree(H=32768) == -1 and agree(W=0) == -1 and agree(pp=63) == -1 and agree(tp=63) == -1
    assert agree(B=2, ti=64 * 31) == -1 and agree(tol2=-1) == -1 and agree(q=0) == -1 and agree(q=101) == -1

    def fin(**kw):
        a = dict(scratch=X, B=1, H=32, W=64, **{k: X for k in "abcdefghijk"})
        a.update(kw)
        return lib.s2s_morph_boundary_finalize(a["scratch"], a["B"], a["H"], a["W"], *[a[k] for k in "abcdefghijk"], None)

    for k in ("scratch", *"abcdefghijk"):
        assert fin(**{k: 0}) == -5, k
    assert fin(B=0) == -1 and fin(H=32768) == -1 and fin(W=0) == -1 and fin(B=65536) == -1


# ---- argument checks that need no GPU ---------------------------------------------------------------------------------
def test_wrappers_reject_before_the_gpu():
    from stain2stain_amd import (distance_transform, fill_holes, mask_boundary, mask_boundary_agreement, mask_morphology)
    m = torch.zeros((2, 16, 16), dtype=torch.uint8)
    calls = [distance_transform, lambda x: mask_morphology(x, "close", 2), fill_holes, mask_boundary,
             lambda x: mask_boundary_agreement(x, x)]
    for f in calls:
        with pytest.raises(TypeError):
            f(m.numpy())
        for bad in (m.float(), m.int(), m[0, 0], m[None], torch.zeros((0, 4, 4), dtype=torch.bool),
                    torch.zeros((2, 0, 4), dtype=torch.bool), torch.zeros((1, 1), dtype=torch.bool).expand(32768, 4),
                    torch.zeros((1, 1), dtype=torch.bool).expand(4, 32768)):
            with pytest.raises(ValueError):
                f(bad)
    for kw in ({"to": "edge"}, {"max_dist": -1}, {"max_dist": float("nan")}, {"max_dist": float("inf")}):
        with pytest.raises(ValueError):
            distance_transform(m, **kw)
    for op, r in (("shrink", 2), ("close", -1), ("open", float("nan")), ("dilate", float("inf"))):
        with pytest.raises(ValueError):
            mask_morphology(m, op, r)
    with pytest.raises(TypeError):
        mask_morphology(m, "close", None)
    for conn in (0, 6):
        with pytest.raises(ValueError):
            fill_holes(m, connectivity=conn)
    with pytest.raises(TypeError):
        fill_holes(m, connectivity=4.0)
    for kw in ({"percentile": 0}, {"percentile": 101}, {"tolerance": -0.5}, {"tolerance": float("nan")}):
        with pytest.raises(ValueError):
            mask_boundary_agreement(m, m, **kw)
    with pytest.raises(TypeError):
        mask_boundary_agreement(m, m, percentile=95.0)
    for other in (m[:, :15], m[0], m[:1]):
        with pytest.raises(ValueError):
            mask_boundary_agreement(m, other)
    with pytest.raises(TypeError):
        mask_boundary_agreement(m, None)


def test_trainer_evaluate_signature():
    import inspect
    from stain2stain_amd import MultiTaskTrainer
    assert inspect.signature(MultiTaskTrainer.evaluate).parameters["boundary"].default is None
