"""Splitting touching objects (stain2stain_amd/split.py, csrc/split.hip) without a GPU: the exports, the
status codes of the two entry points (returned before any HIP call), the wrappers' argument checks, and the numpy
restatement (tests/split_ref.py) on its own: the part counts of simple shapes, the three properties that follow from the
definition, and its squared distances against scipy's float transform."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import morphology_ref as MR
import objects_ref as O
import split_ref as S

NECKS = (0.5, 0.75, 0.9)


def _count(m, connectivity=8, neck=0.75, **kw):
    return int(S.split(m, connectivity=connectivity, neck=neck, **kw)["count"])


# ---- the boundary -------------------------------------------------------------------------------------------------------
def test_exports():
    import stain2stain_amd
    from stain2stain_amd import _native, split
    for name in ("split_objects", "stain_object_split", "label_agreement"):
        assert name in stain2stain_amd.__all__ and getattr(stain2stain_amd, name) is getattr(split, name), name
    assert "split.hip" in _native.SOURCES
    declared = _native.declared_symbols()
    lib = _native.lib()
    for sym in ("s2s_split_words", "s2s_split_label"):
        assert sym in declared and hasattr(lib, sym), sym
    assert split.TILE == (32, 64) and split.NECK_ONE == 1024


def test_entry_points_return_status_codes():
    from stain2stain_amd import _native
    lib = _native.lib()
    X = 4096                                      # a non-null pointer that is never dereferenced: every call below fails first
    words = lib.s2s_split_words
    assert words(1, 32, 64) == 4 * 32 * 64 + 2 and words(3, 33, 65) == 3 * (4 * 33 * 65 + 3)
    assert words(0, 8, 8) == -1 and words(1, 0, 8) == -1 and words(1, 8, -1) == -1 and words(65536, 8, 8) == -1
    assert words(1, 32768, 8) == -1 and words(1, 8, 32768) == -1 and words(65535, 32767, 32767) > 0

    def label(d2=X, B=1, H=32, W=64, conn=8, neck_q=768, core2=0, min_area=1, M=0, scratch=X, labels=X, count=X, basins=X,
              kept=X, largest=X, hist=X, ta=0, tb=0, ts=0):
        return lib.s2s_split_label(d2, B, H, W, conn, neck_q, core2, min_area, M, scratch, labels, count, basins, kept,
                                   largest, hist, ta, tb, ts, None)

    for name in ("d2", "scratch", "labels", "count", "basins", "kept", "largest", "hist"):
        assert label(**{name: 0}) == -5, name
    assert label(M=4) == -5 and label(M=4, ta=X, tb=X) == -5 and label(M=4, ta=X, ts=X) == -5 and label(M=4, tb=X, ts=X) == -5
    assert label(B=0) == -1 and label(B=65536) == -1 and label(H=0) == -1 and label(W=-1) == -1
    assert label(H=32768) == -1 and label(W=32768) == -1
    assert label(conn=6) == -1 and label(conn=0) == -1
    assert label(neck_q=-1) == -1 and label(neck_q=1025) == -1 and label(core2=-1) == -1
    assert label(min_area=0) == -1 and label(M=-1) == -1 and label(B=65535, M=65536, ta=X, tb=X, ts=X) == -1
    assert label(scratch=X + 4) == -2                                      # the 64-bit slots come first in the scratch


def test_wrappers_reject_before_any_gpu_work():
    from stain2stain_amd import label_agreement, split_objects, stain_object_split
    m = torch.zeros((2, 16, 16), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        split_objects(m)
    with pytest.raises(RuntimeError, match="GPU"):
        split_objects(m[0] > 0, d2=torch.zeros((16, 16), dtype=torch.int32))
    with pytest.raises(TypeError):
        split_objects(m.numpy())
    for bad in (m.float(), m.int(), m[0, 0], m[None], torch.zeros((0, 4, 4), dtype=torch.bool)):
        with pytest.raises(ValueError):
            split_objects(bad)
    for kw in ({"neck": -0.01}, {"neck": 1.01}, {"neck": float("nan")}, {"min_core": -1.0}, {"min_core": float("inf")},
               {"connectivity": 6}, {"min_area": 0}, {"max_objects": 0}, {"d2": torch.zeros((2, 16, 16), dtype=torch.int64)},
               {"d2": torch.zeros((2, 16, 15), dtype=torch.int32)}, {"d2": torch.zeros((16, 16), dtype=torch.int32)}):
        with pytest.raises(ValueError):
            split_objects(m, **kw)
    for kw in ({"neck": "wide"}, {"min_core": None}, {"d2": np.zeros((2, 16, 16), np.int32)}, {"min_area": 1.5}):
        with pytest.raises(TypeError):
            split_objects(m, **kw)
    with pytest.raises(ValueError, match="32767"):
        split_objects(torch.zeros((1, 1), dtype=torch.bool).expand(2, 32768))

    u = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        stain_object_split(u)
    with pytest.raises(TypeError):
        stain_object_split(u.numpy())
    for kw in ({"neck": 2}, {"neck": -1}, {"min_core": -0.5}, {"stain": 3}, {"stains": "he"}, {"thresholds": (0.1, 0.2)},
               {"white": 0}, {"black": 256}, {"connectivity": 5}, {"min_area": 0}, {"max_objects": 0}, {"mpp": 0.0}):
        with pytest.raises(ValueError):
            stain_object_split(u, **kw)
    with pytest.raises(ValueError):
        stain_object_split(torch.zeros((2, 16, 16, 4), dtype=torch.uint8))

    lab, cnt = torch.zeros((2, 8, 8), dtype=torch.int32), torch.zeros((2,), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        label_agreement(lab, cnt, lab, cnt)
    with pytest.raises(TypeError):
        label_agreement(lab.numpy(), cnt, lab, cnt)
    for args in ((lab.long(), cnt, lab, cnt), (lab, cnt.long(), lab, cnt), (lab, cnt[:1], lab, cnt), (lab, cnt, lab[:, :7], cnt),
                 (lab, cnt, lab[0], cnt[0]), (lab[0, 0], cnt, lab[0, 0], cnt)):
        with pytest.raises(ValueError):
            label_agreement(*args)


# ---- the restatement on its own -------------------------------------------------------------------------------------------
def test_whole_shapes_stay_whole():
    shapes = {"disc": S.disc(64, 64, 32, 32, 20), "rectangle": S.rectangle(), "ellipse": S.ellipse(),
              "rotated rectangle": S.rotated_rectangle(), "foreground": np.ones((16, 16), np.uint8)}
    for name, m in shapes.items():
        assert O.label(m, 8)[1] == 1, name
        assert [_count(m, 8, n) for n in NECKS] == [1, 1, 1], name
    assert np.all(MR.d2(shapes["foreground"]) == S.FAR) and int(S.split(shapes["foreground"])["basins"]) == 1


def test_touching_discs_are_split_at_their_neck():
    apart, close = S.disc_pair(18), S.disc_pair(10)
    assert O.label(apart, 8)[1] == 1 and O.label(close, 8)[1] == 1
    assert _count(apart, neck=0.75) == 2 and _count(apart, neck=0.5) == 1
    assert [_count(close, neck=n) for n in NECKS] == [1, 1, 1]
    three = S.three_discs()
    assert O.label(three, 8)[1] == 1 and _count(three) == 3
    # neck = 0 joins every basin to its best higher neighbour only: the two lower discs both go to the highest key
    assert _count(three, neck=0.0) == 1 and int(S.split(three)["basins"]) == 3
    # ... so neck = 0 is not label_components: a small disc between two large ones joins one of them, and the two tops,
    # which touch only through it, stay apart
    dumbbell = MR.discs(40, 80, [(20, 22, 12), (20, 40, 6), (20, 58, 12)])
    assert O.label(dumbbell, 8)[1] == 1 and int(S.split(dumbbell)["basins"]) == 3
    assert [_count(dumbbell, neck=n) for n in (0.0, 0.5)] == [2, 3]


def test_smoothed_noise_counts_rise_with_the_neck():
    m = S.smoothed_noise()
    assert m.shape == (96, 96) and O.label(m, 8)[1] == 15
    assert [_count(m, 8, n) for n in NECKS] == [27, 30, 35]
    # min_core only adds links and min_area only drops parts; this field has one basin of core radius <= 3 that is cut off
    assert _count(m, 8, 0.75, min_core=2.0, min_area=5) <= 30 and _count(m, 8, 0.75, min_core=3.0) == 29


def test_four_connectivity_over_segments_a_diagonal_ridge():
    m = S.rotated_rectangle()
    assert _count(m, 4, 0.9) == 12 and _count(m, 8, 0.9) == 1


def _property_masks():
    yield "noise", S.smoothed_noise()
    yield "pair", S.disc_pair(18)
    yield "three", S.three_discs()
    yield "rotated", S.rotated_rectangle()
    yield "serpentine", O.serpentine(21, 13)
    yield "checkerboard", O.checkerboard(9, 11)
    for name, m in MR.patterns(33, 65, seed=5):
        yield name, m


@pytest.mark.parametrize("connectivity", [4, 8])
def test_parts_are_connected_lie_in_one_component_and_cover_the_mask(connectivity):
    for name, m in _property_masks():
        components = O.label(m, connectivity)[1]
        prev = None
        for neck in (0.0, 0.5, 0.75, 0.9, 1.0):
            r = S.split(m, connectivity=connectivity, neck=neck)
            S.check_properties(m, r["labels"], connectivity)
            assert components <= r["count"] <= r["basins"], (name, neck)
            assert prev is None or r["count"] >= prev, (name, neck)          # a higher neck only removes links
            prev = int(r["count"])
            # numbered by first raster pixel
            first = [int(np.flatnonzero(r["labels"].ravel() == k)[0]) for k in range(1, prev + 1)]
            assert first == sorted(first), (name, neck)
    # one basin per pixel where no two foreground pixels are 4-neighbours
    cb = O.checkerboard(9, 11)
    assert int(S.split(cb, connectivity=4)["basins"]) == int(cb.sum()) == _count(cb, 4)


def test_min_area_filter_and_table():
    m = S.smoothed_noise()
    full = S.split(m, max_objects=64)
    small = S.split(m, min_area=40, max_objects=4)
    areas = full["area"][:int(full["count"])]
    assert small["count"] == (areas >= 40).sum() and small["kept_pixels"] == areas[areas >= 40].sum()
    assert np.array_equal(small["area"], areas[areas >= 40][:4]) and small["size_hist"].sum() == small["count"]
    assert np.array_equal(small["labels"] > 0, np.isin(full["labels"], 1 + np.flatnonzero(areas >= 40)))
    k = 3
    ys, xs = np.nonzero(full["labels"] == k)
    assert full["bbox"][k - 1].tolist() == [ys.min(), xs.min(), ys.max() + 1, xs.max() + 1]
    assert full["centroid"][k - 1, 0] == np.float32(ys.sum() / len(ys))


def test_squared_distances_are_those_of_scipy():
    for name, m in _property_masks():
        d2 = MR.d2(m)
        if m.all():
            assert np.all(d2 == S.FAR), name
            continue
        d = ndimage.distance_transform_edt(m)
        assert np.array_equal(d2, np.rint(d * d).astype(np.int32)), name
