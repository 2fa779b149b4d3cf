"""What of the dense region alignment can be checked without a GPU: the numpy restatement's own
properties, the input conditions the GPU end-to-end test rests on, and that bad arguments are refused on the host and by
the entry points before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import region_warp_ref as Wr
import registration_ref as R
import stain2stain_amd
from stain2stain_amd import clean_shift_field, register_region, warp_region


# ---- the restatement's own properties ------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,cell", [(70, 90, 32), (40, 100, 40), (33, 35, 33), (64, 64, 16)])
def test_constant_field_is_an_integer_shift_with_fill(H, W, cell):
    rng = np.random.default_rng(H)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = rng.integers(0, 5, (H, W), dtype=np.uint8)
    for dy, dx in ((0, 0), (3, -5), (-7, 2), (H, 0), (0, -W)):
        D = np.tile(np.array([16 * dy, 16 * dx], np.int32), (H // cell, W // cell, 1))
        ms = max(abs(dy), abs(dx), 1)
        assert np.array_equal(Wr.warp(img, D, cell, ms, 255), Wr.shifted(img, dy, dx, 255)), (dy, dx)
        assert np.array_equal(Wr.warp(mask, D, cell, ms, 9), Wr.shifted(mask, dy, dx, 9)), (dy, dx)


def test_axis_weights_clamp_to_the_nearest_node():
    g0, g1, w = Wr.axis(70, 32, 2)                             # nodes at pixel centres 15.5 and 47.5, 6 ragged rows
    assert g0.tolist() == [0] * 70 and g1.tolist() == [1] * 70
    assert w[:16].tolist() == [0] * 16 and w[16] == 1 and w[47] == 63 and w[48:].tolist() == [64] * 22
    g0, g1, w = Wr.axis(96, 32, 3)
    assert g0[47] == 0 and w[47] == 63 and g0[48] == 1 and w[48] == 1 and g0[95] == 1 and w[95] == 64
    for n, cell in ((40, 40), (33, 33), (79, 40)):              # one node: no weights at all
        assert all(not a.any() for a in Wr.axis(n, cell, 1))


def test_single_row_single_column_and_single_node_grids():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (40, 100, 3), dtype=np.uint8)
    D = np.array([[[16, 0], [48, 0]]], np.int32)               # Gy = 1: dy runs from 1 to 3 pixels along x only
    d = Wr.dense(D, 40, 100, 40)
    assert (d[:, :, 1] == 0).all() and (d == d[:1]).all()
    assert d[0, :20, 0].tolist() == [16] * 20 and d[0, 60:, 0].tolist() == [48] * 40 and d[0, 40, 0] == 32
    assert np.array_equal(Wr.dense(D.transpose(1, 0, 2), 100, 40, 40), d.transpose(1, 0, 2))
    one = Wr.dense(np.array([[[-35, 21]]], np.int32), 33, 35, 33)
    assert (one == [-35, 21]).all()
    out = Wr.warp(img[:33, :35], np.array([[[-35, 21]]], np.int32), 33)
    assert out.shape == (33, 35, 3) and out.dtype == np.uint8


def test_displacement_is_clamped_and_rounds_half_up():
    D = np.array([[[10 ** 9, -10 ** 9], [-2 ** 31, 2 ** 31 - 1]]], np.int32)
    d = Wr.dense(D, 8, 16, 8, max_shift=3)
    assert d.min() == -48 and d.max() == 48 and (np.abs(d[:, :4]) == 48).all()
    D = np.array([[[0, 0], [1, -1]]], np.int32)                # weights 0, 1/4, 3/4, 1 of the second node
    d = Wr.dense(D, 2, 4, 2)
    assert d[0, :, 0].tolist() == [0, 0, 1, 1] and d[0, :, 1].tolist() == [0, 0, -1, -1]
    D = np.array([[[0, 0], [2, -2]]], np.int32)                # exactly halfway: 1/2 -> 1, -1/2 -> 0
    assert Wr.dense(D, 2, 4, 2)[0, :, 0].tolist() == [0, 1, 2, 2] and Wr.dense(D, 2, 4, 2)[0, 1, 1] == 0


def test_single_corner_fills_in_32_iterations():
    shift = np.zeros((17, 33, 2), np.int32)
    shift[0, 0] = (3, -4)
    rel = np.zeros((17, 33), np.uint8)
    rel[0, 0] = 1
    field, kept, stats = Wr.clean(shift, rel)
    assert stats.tolist() == [1, 32] and kept.sum() == 1 and kept[0, 0] == 1
    assert (field == [48, -64]).all()


def _outlier_case():
    rng = np.random.default_rng(11)
    shift = rng.integers(-2, 3, (5, 6, 2)).astype(np.int32)
    shift[2, 3] = (30, 30)
    return shift, np.ones((5, 6), np.uint8)


def test_planted_outlier_is_rejected_and_filled():
    shift, rel = _outlier_case()
    field, kept, stats = Wr.clean(shift, rel, max_dev=4)
    assert kept[2, 3] == 0 and kept.sum() == 29 and stats.tolist() == [29, 1]
    nb = np.array([16 * shift[y, x] for y in (1, 2, 3) for x in (2, 3, 4) if (y, x) != (2, 3)], np.int64)
    assert field[2, 3].tolist() == ((2 * nb.sum(0) + 8) // 16).tolist() and np.abs(field[2, 3]).max() <= 32
    keep = kept.astype(bool)
    assert np.array_equal(field[keep], 16 * shift[keep])


def test_no_reliable_cell_gives_zeros_and_no_iteration():
    shift, _ = _outlier_case()
    field, kept, stats = Wr.clean(shift, np.zeros((5, 6), np.uint8))
    assert not field.any() and not kept.any() and stats.tolist() == [0, 0]
    field, kept, stats = Wr.clean(np.full((5, 6, 2), 65, np.int32), np.ones((5, 6), np.uint8))    # beyond max_shift
    assert not field.any() and not kept.any() and stats.tolist() == [0, 0]


def test_lower_median_and_isolated_cells():
    shift = np.zeros((1, 7, 2), np.int32)                      # one row: at most 2 neighbours, nothing is judged
    shift[0, 3] = (40, 40)
    field, kept, stats = Wr.clean(shift, np.ones((1, 7), np.uint8))
    assert kept.all() and stats.tolist() == [7, 0] and field[0, 3].tolist() == [640, 640]
    shift = np.zeros((2, 3, 2), np.int32)                      # cell (0, 0) has 3 neighbours 0, 0, 6: lower median 0
    shift[1, 1] = (6, 6)
    field, kept, stats = Wr.clean(shift, np.ones((2, 3), np.uint8), max_dev=2)
    assert kept[0, 0] == 1 and kept[1, 1] == 0
    assert Wr.reliable([[1, 1, 0, 1]], [[0.9, 0.4, 0.9, 0.9]], [[0.2, 0.2, 0.2, 0.01]],
                       [[[1, 1]] * 4]).tolist() == [[1, 0, 0, 0]]


# ---- the input conditions of the GPU end-to-end test --------------------------------------------------------------------
def test_glass_pair_registers_on_five_cells():
    src, tgt = Wr.glass_pair()
    shifts, valid = np.zeros((2, 3, 2), np.int32), np.zeros((2, 3), np.int32)
    score, margin = np.zeros((2, 3)), np.zeros((2, 3))
    for gy in range(2):
        cells = [np.stack([img[gy * 64:(gy + 1) * 64, gx * 64:(gx + 1) * 64] for gx in range(3)]) for img in (src, tgt)]
        out = R.register(cells[0], cells[1], radius=6)
        shifts[gy], valid[gy], score[gy], margin[gy] = out["shift"], out["valid"], out["score"], out["margin"]
        for gx in range(3):
            if (gy, gx) != (1, 1):
                gap = R.runner_up_gap(out["scores"][gx], 6)
                print(f"cell ({gy}, {gx}): score {out['score'][gx]:.4f}, margin {out['margin'][gx]:.4f}, gap {gap:.2e}")
                assert gap > 1e-3 and out["margin"][gx] > 0.05
    assert valid.tolist() == [[1, 1, 1], [1, 0, 1]]
    ok = valid.astype(bool)
    assert (shifts[ok] == [3, -5]).all()
    rel = Wr.reliable(valid, score, margin, shifts)
    assert rel.tolist() == valid.tolist()
    field, kept, stats = Wr.clean(shifts, rel)
    assert (field == [48, -80]).all() and stats.tolist() == [5, 1] and kept.tolist() == valid.tolist()
    assert np.array_equal(Wr.warp(tgt, field, 64), Wr.shifted(tgt, 3, -5, 255))


# ---- the boundary ------------------------------------------------------------------------------------------------------------
def test_names_are_exported_and_the_source_is_built():
    from stain2stain_amd import _native
    for name in ("clean_shift_field", "warp_region", "register_region"):
        assert name in stain2stain_amd.__all__ and callable(getattr(stain2stain_amd, name))
    assert "warp.hip" in _native.SOURCES
    assert {"s2s_warp_region_u8", "s2s_field_clean"} <= set(_native.declared_symbols())
    from stain2stain_amd import warp
    assert (warp.SUB, warp.MAX_SHIFT, warp.MAX_CELLS, warp.MAX_CELL) == (Wr.SUB, Wr.MAX_SHIFT, Wr.MAX_CELLS, Wr.MAX_CELL)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from stain2stain_amd import _native
    lib = _native.lib()
    ok = ctypes.c_void_p(4096)

    def warp(src=ok, field=ok, out=ok, src_pitch=300, src_row0=0, src_rows=70, Gy=2, Gx=3, cell=32, max_shift=8, H=70,
             W=100, C=3, fill=255, row0=0, rows=70, out_pitch=300):
        return lib.s2s_warp_region_u8(src, src_pitch, src_row0, src_rows, field, Gy, Gx, cell, max_shift, H, W, C, fill,
                                      row0, rows, out, out_pitch, None)

    assert warp(src=None) == -5 and warp(field=None) == -5 and warp(out=None) == -5
    # the rows present do not cover the band and its halo of max_shift + 1 rows
    assert warp(src_row0=1) == -1 and warp(src_rows=69) == -1
    assert warp(row0=20, rows=10, src_row0=12, src_rows=58) == -1           # needs rows from 11
    assert warp(row0=20, rows=10, src_row0=11, src_rows=27) == -1           # needs rows up to 39
    assert warp(row0=60, rows=11) == -1 and warp(rows=0) == -1 and warp(row0=-1) == -1
    # the grid
    assert warp(Gy=3) == -1 and warp(Gx=2) == -1 and warp(cell=0) == -1 and warp(cell=-32) == -1
    assert warp(H=40000, W=40000, cell=(1 << 14) + 1, Gy=2, Gx=2, src_rows=40000, rows=40000, src_pitch=120000,
                out_pitch=120000) == -1
    assert warp(H=257, W=256, cell=1, Gy=257, Gx=256, src_rows=257, rows=257, src_pitch=768, out_pitch=768) == -1
    assert warp(max_shift=-1) == -1 and warp(max_shift=1025) == -1
    # pitches, channels, fill
    assert warp(src_pitch=299) == -1 and warp(out_pitch=299) == -1 and warp(C=2) == -1 and warp(fill=256) == -1
    assert warp(C=1, src_pitch=99) == -1

    def clean(shift=ok, rel=ok, field=ok, kept=ok, stats=ok, work=ok, Gy=5, Gx=6, max_dev=2, max_shift=64):
        return lib.s2s_field_clean(shift, rel, Gy, Gx, max_dev, max_shift, field, kept, stats, work, None)

    for k in ("shift", "rel", "field", "kept", "stats", "work"):
        assert clean(**{k: None}) == -5, k
    assert clean(Gy=0) == -1 and clean(Gx=0) == -1 and clean(Gy=257, Gx=256) == -1
    assert clean(max_shift=1025) == -1 and clean(max_shift=-1) == -1 and clean(max_dev=-1) == -1


def test_wrappers_raise_on_bad_arguments():
    """Everything here is refused before a device is needed (a host field or shift is refused as such last)."""
    img = torch.zeros((70, 100, 3), dtype=torch.uint8)
    field = torch.zeros((2, 3, 2), dtype=torch.int32)
    with pytest.raises(TypeError, match="region"):
        warp_region(None, field, 32)
    for bad in (img.float(), img[..., :2], img[None], img[:, ::2], img[:0]):
        with pytest.raises(ValueError, match="region|pixels"):
            warp_region(bad, field, 32)
    with pytest.raises(ValueError, match="pixels"):
        warp_region(img[:, :, 0], field, 32)                    # a mask whose pixels are 3 bytes apart
    with pytest.raises(TypeError, match="field"):
        warp_region(img, None, 32)
    for bad in (field.long(), field[:1], field[..., :1], torch.zeros((3, 2, 2), dtype=torch.int32)):
        with pytest.raises(ValueError, match="field"):
            warp_region(img, bad, 32)
    for cell in (0, -1, 71, 1 << 15):
        with pytest.raises(ValueError, match="cell"):
            warp_region(img, field, cell)
    with pytest.raises(ValueError, match="max_shift"):
        warp_region(img, field, 32, max_shift=1025)
    with pytest.raises(ValueError, match="fill"):
        warp_region(img, field, 32, fill=-1)
    with pytest.raises(ValueError, match="band_rows"):
        warp_region(img, field, 32, band_rows=0)
    with pytest.raises(ValueError, match="GPU"):
        warp_region(img, field, 32)                             # a host field: there is no CPU path

    shift = torch.zeros((5, 6, 2), dtype=torch.int32)
    with pytest.raises(TypeError, match="shift"):
        clean_shift_field(None)
    for bad in (shift.long(), shift[..., :1], shift[0], shift[:0]):
        with pytest.raises(ValueError, match="shift"):
            clean_shift_field(bad)
    with pytest.raises(ValueError, match="no 'score'"):
        clean_shift_field({"shift": shift, "valid": shift[..., 0]})
    for bad in (torch.ones((5, 5), dtype=torch.uint8), torch.ones((5, 6))):
        with pytest.raises(ValueError, match="reliable"):
            clean_shift_field(shift, reliable=bad)
    with pytest.raises(ValueError, match="max_dev"):
        clean_shift_field(shift, max_dev=-1)
    with pytest.raises(ValueError, match="max_shift"):
        clean_shift_field(shift, max_shift=-1)
    with pytest.raises(ValueError, match="at most"):
        clean_shift_field(torch.zeros((257, 256, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="GPU"):
        clean_shift_field(shift)

    with pytest.raises(ValueError, match="mask"):
        register_region(img, img, 32, masks=[torch.zeros((70, 99), dtype=torch.uint8)])
    with pytest.raises(ValueError, match="RGB"):
        register_region(img, img[:, :, 0].contiguous(), 32)
    with pytest.raises(ValueError, match="fill"):
        register_region(img, img, 32, mask_fill=300)
