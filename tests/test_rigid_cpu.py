"""What of the rigid pre-alignment can be checked without a GPU: the properties of the definition on the
numpy restatement of tests/rigid_ref.py, the conditions the GPU tests rest on (the planted pairs are recovered with a
clear lead), the host helpers, and that bad arguments are refused on the host and by the entry points before any launch.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import region_warp_ref as Wr
import rigid_ref as G
import stain2stain_amd
from stain2stain_amd import (align_regions, register_rigid, rigid_transform, rigid_warp, rotation_table,
                             structure_overview)

ONE = 1 << 24
SHAPES = [(33, 33), (20, 31), (70, 90), (40, 100)]


def _inputs(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)


# ---- the four identities of the definition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_identity_shift_and_flip(H, W):
    img, mask = _inputs(H, W)
    for arr in (img, mask):
        assert np.array_equal(G.warp(arr, (ONE, 0, 0, 0, H - 1, W - 1)), arr)
        assert np.array_equal(G.warp(arr, (ONE, 0, 0, 0, H - 1, W - 1), nearest=arr.ndim == 3), arr)
        assert np.array_equal(G.warp(arr, (-ONE, 0, 0, 0, H - 1, W - 1)), arr[::-1, ::-1])
        for dy, dx in ((3, -5), (-7, 2), (H, 0), (0, -W), (1, 1)):
            for centre in ((H - 1, W - 1), (0, 0), (-77, 4 * W)):            # a pure shift ignores its centre
                got = G.warp(arr, (ONE, 0, 16 * dy, 16 * dx) + centre, fill=9)
                assert np.array_equal(got, Wr.shifted(arr, dy, dx, 9)), (dy, dx, centre)


@pytest.mark.parametrize("N", [33, 20])
def test_quarter_turn_of_a_square(N):
    img, mask = _inputs(N, N)
    for arr in (img, mask):
        assert np.array_equal(G.warp(arr, (0, ONE, 0, 0, N - 1, N - 1)), np.rot90(arr, -1))
        assert np.array_equal(G.warp(arr, (0, -ONE, 0, 0, N - 1, N - 1)), np.rot90(arr, 1))


@pytest.mark.parametrize("H,W,cell", [(70, 90, 32), (40, 100, 40), (33, 35, 33)])
def test_identity_transform_with_a_field_is_warp_region(H, W, cell):
    img, mask = _inputs(H, W)
    rng = np.random.default_rng(cell)
    D = rng.integers(-200, 201, (H // cell, W // cell, 2)).astype(np.int32)
    T = (ONE, 0, 0, 0, H - 1, W - 1)
    assert np.array_equal(G.warp(img, T, D, cell, 8), Wr.warp(img, D, cell, 8, 255))
    assert np.array_equal(G.warp(mask, T, D, cell, 8, fill=0), Wr.warp(mask, D, cell, 8, 0))


def test_clamps_hold_the_six_numbers():
    big = 1 << 62
    assert G.clamped((big, -big, big, -big, big, -big)) == (ONE, -ONE, 1 << 36, -(1 << 36), ONE, -ONE)
    img, _ = _inputs(20, 31)
    assert np.array_equal(G.warp(img, (big, 0, 0, 0, 19, 30)), img)          # c clamps to one: the identity
    assert (G.warp(img, (ONE, 0, big, 0, 19, 30), fill=7) == 7).all()       # 2^32 pixels away: all fill
    sy, sx = G.positions((big, big, big, big, big, big), (1 << 20) - 1, 0)
    assert max(abs(sy), abs(sx)) < 1 << 54


# ---- the inset ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,max_angle", [(96, 96, 6), (40, 100, 3), (33, 20, 10)])
def test_inset_keeps_fill_out_of_every_crop(h, w, max_angle):
    angles = [float(k) for k in range(-max_angle, max_angle + 1)]
    Tk = G.overview_transforms(rotation_table(angles).tolist(), h, w)
    m = G.inset(Tk, h, w)
    assert m >= 1 and G.inset_ok(Tk, h, w, m) and not G.inset_ok(Tk, h, w, m - 1)
    ones = np.ones((h, w), np.uint8)
    for T in Tk:                                               # 1 inside, 0 for a tap outside: any fill shows as < 1
        bk = G.warp(ones, T, nearest=False, fill=0)
        assert (bk[m:h - m, m:w - m] == 1).all()
    from stain2stain_amd import rigid
    assert rigid._inset(Tk, h, w) == m


# ---- the host helpers ------------------------------------------------------------------------------------------------------
def test_rotation_table_and_rigid_transform():
    t = rotation_table([0, 90, -90, 180, -180, 270, 360]).tolist()
    assert t == [[ONE, 0], [0, ONE], [0, -ONE], [-ONE, 0], [-ONE, 0], [0, -ONE], [ONE, 0]]
    angles = np.linspace(-179.0, 179.0, 359 * 2 - 1)
    got = rotation_table(angles.tolist()).numpy()
    want = np.stack([np.rint(np.cos(np.radians(angles)) * ONE), np.rint(np.sin(np.radians(angles)) * ONE)], 1)
    assert got.dtype == np.int64 and np.abs(got - want).max() <= 1
    T = rigid_transform(90.0, (1.5, -3), shape=(100, 80))
    assert T.dtype == torch.int64 and T.tolist() == [0, ONE, 24, -48, 99, 79]
    assert rigid_transform(0.0, center=(10.5, 4.0)).tolist() == [ONE, 0, 0, 0, 21, 8]
    with pytest.raises(ValueError, match="shape"):
        rigid_transform(1.0)
    with pytest.raises(ValueError, match="finite"):
        rotation_table([float("nan")])


# ---- the conditions of the GPU search tests ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _found(n):
    angle, shift = G.PLANTS[n]
    src, tgt = G.planted(rotation_table([angle])[0].tolist(), shift)
    return G.register(src, tgt, rotation_table(G.SEARCH_ANGLES).tolist(), G.SEARCH_ANGLES, **G.SEARCH)


@pytest.mark.parametrize("n", range(len(G.PLANTS)))
def test_planted_pair_is_recovered(n):
    angle, shift = G.PLANTS[n]
    out = _found(n)
    sc = np.sort(out["scores"])[::-1]
    T = out["transform"]
    print(f"plant {angle} {shift}: angle {out['angle']}, t ({T[2] / 16}, {T[3] / 16}), score {out['score']:.4f}, "
          f"gap {sc[0] - sc[1]:.4f}, inset {out['inset']}")
    assert out["valid"] == 1 and out["angle_index"] == G.SEARCH_ANGLES.index(angle) and out["angle"] == angle
    ds = G.SEARCH["ds"]
    assert abs(T[2] / 16 - shift[0]) <= ds and abs(T[3] / 16 - shift[1]) <= ds
    assert sc[0] - sc[1] > 1e-3 and out["score"] == sc[0]
    assert T[4] == 191 and T[5] == 191 and out["inset"] >= 1


def test_flat_source_is_invalid_and_the_identity():
    _, tgt = G.base_pair()
    flat = np.full_like(tgt, 255)
    out = G.register(flat, tgt, rotation_table(G.SEARCH_ANGLES).tolist(), G.SEARCH_ANGLES, **G.SEARCH)
    assert out["valid"] == 0 and out["transform"].tolist() == [ONE, 0, 0, 0, 191, 191] and out["angle_index"] == -1


def test_align_chain_conditions():
    """What the GPU end-to-end test rests on: after the rigid stage every cell of the 64-pixel grid registers with a
    lead of more than 1e-3 and passes the cleaning, and the one resampling brings the target back onto the original."""
    src, tgt = G.planted(rotation_table([3.0])[0].tolist(), (6, -10))
    out = G.align(src, tgt, rotation_table(G.SEARCH_ANGLES).tolist(), G.SEARCH_ANGLES, 64, rigid=G.SEARCH, radius=6)
    m = out["measured"]
    print(f"cells: gap {m['gap'].min():.4f}..{m['gap'].max():.4f}, margin {m['margin'].min():.3f}, "
          f"score {m['score'].min():.3f}, shifts {np.unique(m['shift'].reshape(-1, 2), axis=0).tolist()}")
    assert (m["valid"] == 1).all() and (m["gap"] > 1e-3).all() and (m["margin"] > 0.05).all() and (m["score"] > 0.5).all()
    assert out["kept"].all() and out["stats"].tolist() == [9, 0] and np.abs(m["shift"]).max() <= 2
    original = G.base_pair()[1].astype(np.int64)
    err = lambda a: np.abs(a[24:-24, 24:-24].astype(np.int64) - original[24:-24, 24:-24]).mean()      # noqa: E731
    assert err(out["aligned"]) <= err(out["intermediate"]) < 0.25 * err(tgt)


# ---- the boundary --------------------------------------------------------------------------------------------------------------
def test_names_are_exported_and_the_source_is_built():
    from stain2stain_amd import _native
    for name in ("structure_overview", "rigid_warp", "register_rigid", "align_regions", "rotation_table",
                 "rigid_transform"):
        assert name in stain2stain_amd.__all__ and callable(getattr(stain2stain_amd, name))
    assert "rigid.hip" in _native.SOURCES
    assert {"s2s_structure_overview_u8", "s2s_rigid_warp_u8"} <= set(_native.declared_symbols())
    from stain2stain_amd import rigid
    assert (rigid.ONE,) + rigid._LIMITS == (G.ONE,) + G.LIMITS


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from stain2stain_amd import _native
    lib = _native.lib()
    ok = ctypes.c_void_p(4096)
    q = (ctypes.c_int * 256)(*range(256))
    w3 = (ctypes.c_int * 3)(100, -50, 25)

    def warp(src=ok, transform=ok, field=ok, out=ok, src_pitch=300, src_row0=0, src_rows=70, A=1, Gy=2, Gx=3, cell=32,
             max_shift=8, H=70, W=100, C=3, nearest=0, fill=255, row0=0, rows=70, out_pitch=300, out_img=21000):
        return lib.s2s_rigid_warp_u8(src, src_pitch, src_row0, src_rows, transform, A, field, Gy, Gx, cell, max_shift, H,
                                     W, C, nearest, fill, row0, rows, out, out_pitch, out_img, None)

    # the statuses of s2s_warp_region_u8: null pointers -5, shapes -1
    assert warp(src=None) == -5 and warp(transform=None) == -5 and warp(out=None) == -5
    assert warp(row0=60, rows=11) == -1 and warp(rows=0) == -1 and warp(row0=-1) == -1
    assert warp(src_row0=-1) == -1 and warp(src_rows=0) == -1 and warp(src_row0=1) == -1
    assert warp(Gy=3) == -1 and warp(Gx=2) == -1 and warp(cell=0) == -1 and warp(cell=-32) == -1
    assert warp(H=257, W=256, cell=1, Gy=257, Gx=256, src_rows=257, rows=257, src_pitch=768, out_pitch=768) == -1
    assert warp(max_shift=-1) == -1 and warp(max_shift=1025) == -1
    assert warp(src_pitch=299) == -1 and warp(out_pitch=299) == -1 and warp(C=2) == -1 and warp(fill=256) == -1
    assert warp(C=1, src_pitch=99) == -1 and warp(nearest=2) == -1
    assert warp(A=0) == -1 and warp(A=65536) == -1 and warp(A=2, out_img=20999) == -1
    assert warp(H=(1 << 20) + 1, src_rows=70) == -1 and warp(W=(1 << 20) + 1, src_pitch=1 << 23, out_pitch=1 << 23) == -1

    def over(img=ok, qt=q, w=w3, out=ok, pitch=300, H=70, W=100, ds=16):
        return lib.s2s_structure_overview_u8(img, pitch, H, W, qt, w, ds, out, None)

    assert over(img=None) == -5 and over(qt=None) == -5 and over(w=None) == -5 and over(out=None) == -5
    assert over(ds=0) == -1 and over(ds=3) == -1 and over(ds=128) == -1 and over(ds=-4) == -1
    assert over(H=15) == -1 and over(W=15, pitch=45) == -1 and over(pitch=299) == -1
    assert over(w=(ctypes.c_int * 3)(1 << 30, 1 << 30, 1 << 30)) == -1
    assert over(qt=(ctypes.c_int * 256)(*([-1] + [0] * 255))) == -1


def test_wrappers_raise_on_bad_arguments():
    """Everything here is refused before a device is needed."""
    img = torch.zeros((70, 100, 3), dtype=torch.uint8)
    T = rigid_transform(1.0, shape=(70, 100))
    for ds in (0, 3, 128, -2):
        with pytest.raises(ValueError, match="power of two"):
            structure_overview(img, ds)
        with pytest.raises(ValueError, match="power of two"):
            register_rigid(img, img, downsample=ds)
    with pytest.raises(ValueError, match="smaller than one"):
        structure_overview(img[:40], 64)
    with pytest.raises(ValueError, match="smaller than one"):
        register_rigid(img[:40], img[:40], downsample=64)
    with pytest.raises(ValueError, match="band_rows"):
        structure_overview(img, 16, band_rows=0)
    with pytest.raises(TypeError, match="region"):
        structure_overview(None)
    with pytest.raises(ValueError, match="region|pixels"):
        structure_overview(img[:, :, 0])
    with pytest.raises(ValueError, match="differ in shape"):
        register_rigid(img, img[:, :90])
    with pytest.raises(ValueError, match="raise downsample or lower radius"):
        register_rigid(img, img, downsample=2, radius=32)       # 35 x 50 maps cannot hold radius 32
    with pytest.raises(ValueError, match="raise downsample or lower radius"):
        register_rigid(img, img, downsample=1, radius=33)
    with pytest.raises(ValueError, match="angle"):
        register_rigid(img, img, angles=[])
    with pytest.raises(ValueError, match="angle_step"):
        register_rigid(img, img, angle_step=0.0)
    with pytest.raises(TypeError, match="transform"):
        rigid_warp(img, [1, 0, 0, 0, 0, 0])
    for bad in (T.to(torch.int32), T.double(), T[:5], T[None, None], torch.zeros((0, 6), dtype=torch.int64)):
        with pytest.raises(ValueError, match="transform"):
            rigid_warp(img, bad)
    field = torch.zeros((2, 3, 2), dtype=torch.int32)
    with pytest.raises(ValueError, match="cell"):
        rigid_warp(img, T, field=field)
    with pytest.raises(ValueError, match="field"):
        rigid_warp(img, T, field=field[:1], cell=32)
    with pytest.raises(ValueError, match="no field"):
        rigid_warp(img, T[None], field=field, cell=32)
    with pytest.raises(ValueError, match="GPU region"):
        rigid_warp(img, T[None].repeat(3, 1))
    with pytest.raises(ValueError, match="max_shift"):
        rigid_warp(img, T, max_shift=1025)
    with pytest.raises(ValueError, match="fill"):
        rigid_warp(img, T, fill=256)
    with pytest.raises(ValueError, match="band_rows"):
        rigid_warp(img, T, band_rows=0)
    with pytest.raises(ValueError, match="GPU"):
        rigid_warp(img, T, field=field, cell=32)                # a host field: there is no CPU path
    with pytest.raises(ValueError, match="mask"):
        align_regions(img, img, 32, masks=[torch.zeros((70, 99), dtype=torch.uint8)])
    with pytest.raises(ValueError, match="RGB"):
        align_regions(img, img[:, :, 0].contiguous(), 32)
    with pytest.raises(ValueError, match="fill"):
        align_regions(img, img, 32, mask_fill=300)
