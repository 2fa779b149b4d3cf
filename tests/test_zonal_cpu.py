"""Zonal stain quantification (stain2stain_amd/zonal.py, csrc/zonal.hip) without a GPU: the restatement
of tests/zonal_ref.py against brute-force Python loops and against the restatement of 3.17, the arg-max and band rules on
hand-made tables, the boundary (exports, the status codes of the new entry points, returned before any HIP call) and the
argument checks the wrappers make before they touch the device."""
import ctypes

import numpy as np
import pytest
import torch

import stain_quant_ref as R
import zonal_ref as Zr

THR = (0.2, 0.2, 0.2)


def _m32(stains="hdab"):
    from stain2stain_amd.stain_quant import unmix_matrix
    return unmix_matrix(stains).numpy()


def _stained(B, H, W, seed, plaque=0.15):
    rng = np.random.default_rng(seed)
    conc = np.zeros((B, H, W, 3))
    conc[..., 0] = rng.uniform(0.05, 0.5, size=(B, H, W))
    conc[..., 1] = np.where(rng.random((B, H, W)) < plaque, rng.uniform(0.1, 1.2, size=(B, H, W)), 0.02)
    img = R.synthesise(conc, "hdab").astype(np.int32) + rng.integers(-3, 4, size=(B, H, W, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    glass = rng.random((B, H, W)) < 0.2
    img[glass] = rng.integers(225, 256, size=(int(glass.sum()), 3), dtype=np.uint8)
    return img


# ---- the boundary ----------------------------------------------------------------------------------------------------
SYMBOLS = {"s2s_zonal_u8", "s2s_zonal_f32", "s2s_zonal_pair_u8", "s2s_zonal_pair_f32", "s2s_zonal_finalize",
           "s2s_zonal_object_overlap", "s2s_zonal_object_assign", "s2s_zonal_object_density", "s2s_zonal_bands"}
EXPORTS = ("stain_zonal", "stain_zonal_agreement", "region_stain_zonal", "region_stain_zonal_agreement", "object_zones",
           "stain_zonal_objects", "distance_zones")


def test_exports_sources_and_symbols():
    import os
    import re
    import stain2stain_amd
    from stain2stain_amd import _native, zonal
    for name in EXPORTS:
        assert name in stain2stain_amd.__all__ and getattr(stain2stain_amd, name) is getattr(zonal, name), name
    assert "zonal.hip" in _native.SOURCES
    assert SYMBOLS <= set(_native.declared_symbols())
    lib = _native.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    text = open(os.path.join(_native.CSRC, "zonal.hip")).read()
    assert not re.search(r"getenv", text)
    assert zonal.MAX_ZONES == 256 and zonal.MAX_EDGES == 126 and zonal.FAR == Zr.FAR == 2 ** 31 - 1


# ---- the restatement against loops -----------------------------------------------------------------------------------
def test_restatement_equals_brute_force_loops():
    m32 = _m32()
    H, W, Z = 9, 11, 4
    a, b = _stained(2, H, W, 1), _stained(2, H, W, 2)
    rng = np.random.default_rng(3)
    zones = rng.integers(0, 6, size=(2, H, W)).astype(np.uint8)          # bytes 4 and 5 are no zone
    zones[0, 0, 0] = 255
    tab, unz = Zr.table(a, zones, Z, m32, THR)
    ptab, punz = Zr.pair_table(a, b, zones, Z, m32, THR, stain=1)
    thr32 = np.asarray(THR, np.float32)
    od = R.od_table32()
    for n in range(2):
        want = [[0] * 8 for _ in range(Z)]
        wantp = [[0] * 6 for _ in range(Z)]
        nun = 0
        for y in range(H):
            for x in range(W):
                z = int(zones[n, y, x])
                if z >= Z:
                    nun += 1
                    continue

                def pixel(img):
                    r, g, bl = (int(v) for v in img[n, y, x])
                    t = min(r, g, bl) < 220 and max(r, g, bl) >= 0
                    c = [np.float32(np.float32(od[r] * m32[0][k]) + np.float32(od[g] * m32[1][k])) +
                         np.float32(od[bl] * m32[2][k]) for k in range(3)]
                    return t, c

                t, c = pixel(a)
                want[z][0] += 1
                want[z][1] += int(t)
                for k in range(3):
                    want[z][2 + k] += int(t and c[k] > thr32[k])
                    if t:
                        q = np.float32(max(c[k], np.float32(0))) * np.float32(1024)
                        want[z][5 + k] += min(int(np.rint(q)), 4095)
                tb, cb = pixel(b)
                pa, pb = bool(t and c[1] > thr32[1]), bool(tb and cb[1] > thr32[1])
                for k, v in enumerate((1, t, tb, pa and pb, pa and not pb, pb and not pa)):
                    wantp[z][k] += int(v)
        assert tab[n].tolist() == want and int(unz[n]) == nun, n
        assert ptab[n].tolist() == wantp and int(punz[n]) == nun, n
    assert unz.sum() > 0 and tab[..., 2:5].sum() > 0 and tab[..., 5:8].sum() > 0
    pooled, pun = Zr.table(a, zones, Z, m32, THR, pool=True)
    assert np.array_equal(pooled[0], tab.sum(0)) and pun[0] == unz.sum()
    # derived values: plain Python float arithmetic on the integers
    d = Zr.derived(tab, unz)
    for n in range(2):
        for z in range(Z):
            px, ts = int(tab[n, z, 0]), int(tab[n, z, 1])
            assert d["tissue_frac"][n, z] == float(ts) / float(max(px, 1))
            assert d["area_frac"][n, z] == float(px) / float(H * W)
            for k in range(3):
                assert d["burden"][n, z, k] == float(int(tab[n, z, 2 + k])) / float(max(ts, 1))
                assert d["mean_conc"][n, z, k] == (float(int(tab[n, z, 5 + k])) / float(max(ts, 1))) / 1024.0
    pd = Zr.pair_derived(np.array([[0, 0, 0, 0, 0, 0], [10, 8, 9, 2, 1, 3]]))
    assert pd["dice"].tolist() == [1.0, 4.0 / 8.0] and pd["iou"].tolist() == [1.0, 2.0 / 6.0]
    assert pd["burden_pred"].tolist() == [0.0, 3.0 / 8.0] and pd["burden_target"].tolist() == [0.0, 5.0 / 9.0]
    assert pd["burden_abs_err"][1] == abs(3.0 / 8.0 - 5.0 / 9.0)


def test_zones_sum_to_the_quantification_of_3_17():
    m32 = _m32()
    img = _stained(3, 24, 31, 5)
    zones = np.random.default_rng(6).integers(0, 7, size=(3, 24, 31)).astype(np.uint8)
    for white, black in ((220, 0), (256, 40)):
        tab, unz = Zr.table(img, zones, 7, m32, THR, white, black)
        ref = R.quantify32(img, m32, THR, white, black)
        assert (unz == 0).all()
        assert np.array_equal(tab[..., 1].sum(1), ref["tissue"]) and np.array_equal(tab[..., 2:5].sum(1), ref["positive"])
        assert np.array_equal(tab[..., 0].sum(1), np.full(3, 24 * 31))
    one, _ = Zr.table(img, np.zeros_like(zones), 1, m32, THR)
    ref = R.quantify32(img, m32, THR)
    assert np.array_equal(one[:, 0, 1], ref["tissue"]) and np.array_equal(one[:, 0, 2:5], ref["positive"])
    assert np.array_equal(Zr.derived(one, np.zeros(3, np.int64))["burden"][:, 0], ref["burden"])
    # mean_conc is the mean of the rounded grid values: within half a grid step of mean_od (no clamp is hit here)
    mc = Zr.derived(one, np.zeros(3, np.int64))["mean_conc"][:, 0]
    assert np.abs(mc - ref["mean_od"]).max() <= 0.5 / 1024 + 1e-6


# ---- the arg-max ------------------------------------------------------------------------------------------------------
def test_argmax_tie_rule_and_the_minus_one_cases():
    ov = np.zeros((1, 6, 4), np.int32)
    ov[0, 0] = [0, 5, 5, 1]            # a tie: the smaller zone
    ov[0, 1] = [0, 0, 0, 0]            # no zoned pixel
    ov[0, 2] = [1, 2, 3, 4]            # the last zone
    ov[0, 3] = [7, 0, 0, 7]            # a tie between the first and the last
    ov[0, 4] = [0, 0, 9, 0]            # at count: not an object
    area = np.array([[12, 3, 10, 14, 9, 0]], np.int32)
    zone, zpix, objects, opix = Zr.assign(ov, area, np.array([4], np.int32))
    assert zone[0].tolist() == [1, -1, 3, 0, -1, -1] and zpix[0].tolist() == [5, 0, 4, 7, 0, 0]
    assert objects[0].tolist() == [1, 1, 0, 1] and opix[0].tolist() == [14, 12, 0, 10]
    zone, _, objects, _ = Zr.assign(ov, area, np.array([9], np.int32))         # count beyond M: every row is live
    assert zone[0].tolist() == [1, -1, 3, 0, 2, -1] and objects[0].tolist() == [1, 1, 1, 1]
    zone, _, objects, _ = Zr.assign(ov, area, np.array([0], np.int32))
    assert (zone == -1).all() and (objects == 0).all()
    # overlap itself: labels above M are not tabulated but counted in count; unzoned pixels count towards the area only
    labels = np.array([[[1, 1, 2, 0], [1, 3, 2, 2]]], np.int32)
    zones = np.array([[[0, 1, 1, 0], [255, 0, 2, 2]]], np.uint8)
    o = Zr.object_zones(labels, zones, 2, 2)
    assert o["count"].tolist() == [3] and o["area"].tolist() == [[3, 3]]
    assert o["overlap"].tolist() == [[[1, 1], [0, 1]]] and o["zone"].tolist() == [[0, 1]]
    assert o["zone_pixels"].tolist() == [[1, 1]] and o["object_pixels"].tolist() == [[3, 3]]


# ---- distance bands ---------------------------------------------------------------------------------------------------
def test_squared_edges_and_the_band_rule():
    from stain2stain_amd.zonal import squared_edges
    assert Zr.squared_edges([2.5]) == [6] and squared_edges([2.5]) == (6,)
    assert Zr.squared_edges([0, 1, 1.5, 3, 46340.9]) == [0, 1, 2, 9, 2147479012]
    assert squared_edges([0, 1, 1.5, 3, 46340.9]) == (0, 1, 2, 9, 2147479012)
    assert squared_edges([0.1, 0.2]) == (0, 0)                            # ascending edges, equal E: an empty band
    for bad in ([], [1, 1], [2, 1], [-1], [float("nan")], [float("inf")], [46341], list(range(127)), 3, ["x"]):
        with pytest.raises(ValueError):
            squared_edges(bad)
    E = [1, 6]
    d_bg = np.array([[0, 0, 1, 2, 6, 7, Zr.FAR]], np.int32)
    d_fg = np.array([[1, 7, 0, 0, 0, 0, 0]], np.int32)
    assert Zr.bands(d_bg, d_fg, E).tolist() == [[3, 5, 0, 1, 1, 2, 2]]
    assert Zr.bands(d_bg, d_fg, E, "inside").tolist() == [[255, 255, 0, 1, 1, 2, 2]]
    assert Zr.bands(d_bg, d_fg, E, "outside").tolist() == [[3, 5, 255, 255, 255, 255, 255]]
    far = np.full((1, 3), Zr.FAR, np.int32)
    assert Zr.bands(np.zeros((1, 3), np.int32), far, E).tolist() == [[5, 5, 5]]     # an empty mask: the outermost band
    mask = np.zeros((1, 7, 9), bool)
    mask[0, 1:6, 2:8] = True
    z, nz = Zr.distance_zones(mask, [1, 2.5])
    assert nz == 6 and z[0, 3, 4] == 2 and z[0, 1, 2] == 0 and z[0, 2, 3] == 1 and z[0, 0, 0] == 4 and z[0, 3, 0] == 4
    assert z[0, 0, 2] == 3


# ---- status codes of the entry points: returned before any HIP call ---------------------------------------------------
def test_entry_points_return_status_codes():
    from stain2stain_amd import _native
    lib = _native.lib()
    od, um = (ctypes.c_float * 256)(), (ctypes.c_float * 12)()
    X = 4096                                      # a non-null pointer that is never dereferenced: every call below fails first

    def u8(img=X, pitch=96, zones=X, zp=32, B=1, band_top=0, band_h=32, H=32, W=32, Z=4, od=od, um=um, white=220, black=0,
           pool=0, table=X, unz=X, stride=None, zs=None):
        return lib.s2s_zonal_u8(img, pitch, pitch * band_h if stride is None else stride, zones, zp,
                                zp * band_h if zs is None else zs, B, band_top, band_h, H, W, Z, od, um, white, black,
                                pool, 1, table, unz, None)

    assert u8(img=0) == -5 and u8(zones=0) == -5 and u8(table=0) == -5 and u8(unz=0) == -5 and u8(od=None) == -5
    assert u8(um=None) == -5
    assert u8(B=0) == -1 and u8(B=-2) == -1 and u8(B=65536) == -1 and u8(H=0) == -1 and u8(W=-1) == -1
    assert u8(Z=0) == -1 and u8(Z=257) == -1 and u8(Z=-3) == -1
    assert u8(pitch=95) == -1 and u8(zp=31) == -1 and u8(band_h=0) == -1 and u8(band_h=33) == -1
    assert u8(band_top=1) == -1 and u8(band_top=-1) == -1
    assert u8(B=2, stride=96 * 31) == -1 and u8(B=2, zs=32 * 31) == -1
    assert u8(white=0) == -1 and u8(white=257) == -1 and u8(black=256) == -1 and u8(black=-1) == -1
    assert u8(H=1 << 30, W=1 << 11, pitch=3 << 11, zp=1 << 11, band_h=1) == -1          # 2^41 pixels in one owner
    assert u8(H=1 << 20, W=1 << 10, pitch=3 << 10, zp=1 << 10, band_h=1, B=2048, pool=1, stride=3 << 10,
              zs=1 << 10) == -1                                                          # pooled: 2^41
    # 2^20 pixels or more per workgroup: one owner on the whole grid of 2048, and 2048 owners with one workgroup each
    assert u8(H=1 << 16, W=1 << 15, pitch=3 << 15, zp=1 << 15, band_h=1 << 16) == -1
    assert u8(H=1024, W=1024, pitch=3072, zp=1024, band_h=1024, B=2048) == -1

    def f32(img=X, zones=X, zp=8, B=1, H=8, W=8, Z=4, od=od, um=um, table=X, unz=X, white=220, zs=64):
        return lib.s2s_zonal_f32(img, zones, zp, zs, B, H, W, Z, od, um, white, 0, 0, 1, table, unz, None)

    assert f32(img=0) == -5 and f32(zones=0) == -5 and f32(table=0) == -5 and f32(unz=0) == -5 and f32(od=None) == -5
    assert f32(um=None) == -5
    assert f32(B=0) == -1 and f32(H=0) == -1 and f32(W=-3) == -1 and f32(Z=0) == -1 and f32(Z=300) == -1
    assert f32(white=300) == -1 and f32(zp=7) == -1 and f32(B=2, zs=63) == -1
    assert f32(B=2048, H=1024, W=1024, zp=1024, zs=1 << 20) == -1                        # 2^20 pixels per workgroup

    def p8(a=X, b=X, zones=X, pitch=96, pitch_b=96, zp=32, B=1, band_top=0, band_h=32, H=32, W=32, Z=4, od=od, um=um,
           stain=1, table=X, unz=X):
        return lib.s2s_zonal_pair_u8(a, pitch, pitch * band_h, b, pitch_b, pitch_b * band_h, zones, zp, zp * band_h, B,
                                     band_top, band_h, H, W, Z, od, um, 220, 0, stain, 0, 1, table, unz, None)

    assert p8(a=0) == -5 and p8(b=0) == -5 and p8(zones=0) == -5 and p8(table=0) == -5 and p8(unz=0) == -5
    assert p8(od=None) == -5
    assert p8(B=0) == -1 and p8(stain=3) == -1 and p8(stain=-1) == -1 and p8(Z=0) == -1 and p8(Z=257) == -1
    assert p8(pitch=95) == -1 and p8(pitch_b=95) == -1 and p8(zp=31) == -1 and p8(band_h=33) == -1 and p8(W=0) == -1
    assert p8(H=1 << 16, W=1 << 15, pitch=3 << 15, pitch_b=3 << 15, zp=1 << 15, band_h=1 << 16) == -1

    def pf(a=X, b=X, zones=X, B=1, H=8, W=8, Z=4, um=um, stain=1, table=X, unz=X, zp=8):
        return lib.s2s_zonal_pair_f32(a, b, zones, zp, zp * H, B, H, W, Z, od, um, 220, 0, stain, 0, 1, table, unz, None)

    assert pf(a=0) == -5 and pf(b=0) == -5 and pf(zones=0) == -5 and pf(table=0) == -5 and pf(unz=0) == -5
    assert pf(um=None) == -5
    assert pf(B=0) == -1 and pf(H=0) == -1 and pf(stain=5) == -1 and pf(Z=0) == -1 and pf(zp=7) == -1

    def fin(table=X, unz=X, owners=1, Z=4, paired=0, out=X):
        return lib.s2s_zonal_finalize(table, unz, owners, Z, paired, out, None)

    assert fin(table=0) == -5 and fin(out=0) == -5 and fin(unz=0) == -5 and fin(unz=0, paired=1, owners=0) == -1
    assert fin(owners=0) == -1 and fin(owners=-2) == -1 and fin(Z=0) == -1 and fin(Z=257) == -1

    def ov(labels=X, zones=X, zp=32, B=1, H=32, W=32, Z=4, M=16, overlap=X, area=X, count=X, zs=None):
        return lib.s2s_zonal_object_overlap(labels, zones, zp, zp * H if zs is None else zs, B, H, W, Z, M, overlap, area,
                                            count, None)

    assert ov(labels=0) == -5 and ov(zones=0) == -5 and ov(overlap=0) == -5 and ov(area=0) == -5 and ov(count=0) == -5
    assert ov(B=0) == -1 and ov(B=65536) == -1 and ov(H=0) == -1 and ov(W=32768, zp=32768) == -1 and ov(H=32768) == -1
    assert ov(Z=0) == -1 and ov(Z=257) == -1 and ov(M=0) == -1 and ov(M=-1) == -1 and ov(zp=31) == -1
    assert ov(B=2, zs=32 * 31) == -1
    assert ov(M=1 << 29, Z=4) == -1 and ov(B=8, M=1 << 20, Z=256) == -1                  # B M Z = 2^31

    def asg(overlap=X, area=X, count=X, B=1, Z=4, M=16, zone=X, zpix=X, objects=X, opix=X):
        return lib.s2s_zonal_object_assign(overlap, area, count, B, Z, M, zone, zpix, objects, opix, None)

    assert asg(overlap=0) == -5 and asg(area=0) == -5 and asg(count=0) == -5 and asg(zone=0) == -5 and asg(zpix=0) == -5
    assert asg(objects=0) == -5 and asg(opix=0) == -5
    assert asg(B=0) == -1 and asg(Z=0) == -1 and asg(Z=257) == -1 and asg(M=0) == -1 and asg(M=1 << 29) == -1

    one, zero, nan = (ctypes.c_double * 1)(2.5e-7), (ctypes.c_double * 1)(0.0), (ctypes.c_double * 1)(float("nan"))

    def den(objects=X, table=X, owners=1, Z=4, scale=one, out=X):
        return lib.s2s_zonal_object_density(objects, table, owners, Z, scale, out, None)

    assert den(objects=0) == -5 and den(table=0) == -5 and den(scale=None) == -5 and den(out=0) == -5
    assert den(owners=0) == -1 and den(Z=0) == -1 and den(Z=257) == -1 and den(scale=zero) == -1 and den(scale=nan) == -1

    def bd(bg=X, fg=X, B=1, H=8, W=8, E=(1, 6), n=None, side=0, out=X):
        arr = (ctypes.c_int * max(len(E), 1))(*E)
        return lib.s2s_zonal_bands(bg, fg, B, H, W, arr, len(E) if n is None else n, side, out, None)

    assert bd(bg=0) == -5 and bd(fg=0) == -5 and bd(out=0) == -5
    assert lib.s2s_zonal_bands(X, X, 1, 8, 8, None, 1, 0, X, None) == -5
    assert bd(B=0) == -1 and bd(H=0) == -1 and bd(W=32768) == -1 and bd(n=0) == -1 and bd(E=tuple(range(127))) == -1
    assert bd(side=3) == -1 and bd(side=-1) == -1
    assert bd(E=(6, 1)) == -1 and bd(E=(-1, 3)) == -1 and bd(E=(1, 2 ** 31 - 1)) == -1
    assert bd(bg=X + 4) == -2 and bd(fg=X + 8) == -2 and bd(out=X + 2) == -2


# ---- argument checks that need no GPU --------------------------------------------------------------------------------
def test_wrappers_reject():
    from stain2stain_amd import (distance_zones, object_zones, region_stain_zonal, region_stain_zonal_agreement,
                                 stain_zonal, stain_zonal_agreement, stain_zonal_objects)
    u = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    f = torch.zeros((2, 3, 16, 16))
    z = torch.zeros((2, 16, 16), dtype=torch.uint8)
    r = torch.zeros((40, 40, 3), dtype=torch.uint8)
    rz = torch.zeros((40, 40), dtype=torch.uint8)
    for fn in (stain_zonal, stain_zonal_objects):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(u, z, 4)                                                   # CPU tensors: there is no CPU path
        with pytest.raises(ValueError):
            fn(torch.zeros((2, 16, 16, 4), dtype=torch.uint8), z, 4)
        with pytest.raises(ValueError):
            fn(f.double(), z, 4)
        with pytest.raises(TypeError):
            fn(u.numpy(), z, 4)
        with pytest.raises(TypeError):
            fn(u, z.numpy(), 4)
        with pytest.raises(ValueError):
            fn(u, z.int(), 4)
        with pytest.raises(ValueError):
            fn(u, z[:, :15], 4)
        with pytest.raises(ValueError):
            fn(u, z, 0)
        with pytest.raises(ValueError):
            fn(u, z, 257)
        with pytest.raises(ValueError):
            fn(u, z, 4, stains="he")
        with pytest.raises(ValueError):
            fn(u, z, 4, white=0)
        with pytest.raises(ValueError):
            fn(u, z, 4, thresholds=(0.2, 0.2))
    with pytest.raises(RuntimeError, match="GPU"):
        stain_zonal(f, z.bool(), 4)
    with pytest.raises(TypeError):
        stain_zonal(u, z, 4, out=3)
    with pytest.raises(ValueError):
        stain_zonal_objects(u, z, 4, mpp=0.0)
    with pytest.raises(ValueError):
        stain_zonal_objects(u, z, 4, max_objects=0)
    with pytest.raises(ValueError):
        stain_zonal_objects(u, z, 4, connectivity=6)
    with pytest.raises(RuntimeError, match="GPU"):
        stain_zonal_agreement(u, u.clone(), z, 4)
    with pytest.raises(ValueError):
        stain_zonal_agreement(u, u[:, :15], z, 4)
    with pytest.raises(ValueError):
        stain_zonal_agreement(u, f, z, 4)
    with pytest.raises(ValueError):
        stain_zonal_agreement(u, u.clone(), z, 4, stain=3)
    with pytest.raises(TypeError):
        stain_zonal_agreement(u, None, z, 4)
    # regions
    for fn in (region_stain_zonal, lambda a, zz, Z, **kw: region_stain_zonal_agreement(a, a.clone(), zz, Z, **kw)):
        with pytest.raises(ValueError):
            fn(r.float(), rz, 4)
        with pytest.raises(ValueError):
            fn(r[:, ::2], rz[:, ::2], 4)
        with pytest.raises(ValueError):
            fn(r, rz, 4, band_rows=0)
        with pytest.raises(ValueError):
            fn(r, rz[:39], 4)
        with pytest.raises(ValueError):
            fn(r, rz[:, ::2], 4)
        with pytest.raises(ValueError):
            fn(r, rz.float(), 4)
        with pytest.raises(ValueError):
            fn(r, rz, 300)
        with pytest.raises(TypeError):
            fn(r, None, 4)
    with pytest.raises(TypeError):
        region_stain_zonal(None, rz, 4)
    with pytest.raises(ValueError):
        region_stain_zonal_agreement(r, r[:39], rz, 4)
    with pytest.raises(ValueError):
        region_stain_zonal_agreement(r, r.clone(), rz, 4, stain=-1)
    # objects
    lab = torch.zeros((2, 16, 16), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        object_zones(lab, z, 4)
    with pytest.raises(ValueError):
        object_zones(lab.long(), z, 4)
    with pytest.raises(TypeError):
        object_zones(None, z, 4)
    with pytest.raises(ValueError):
        object_zones(lab, z[0], 4)
    with pytest.raises(ValueError):
        object_zones(lab, z, 4, max_objects=0)
    with pytest.raises(ValueError):
        object_zones(lab, z, 256, max_objects=1 << 22)                    # 2 * 2^22 * 256 = 2^31
    with pytest.raises(ValueError):
        object_zones(lab, z, 0)
    # distance bands
    m = torch.zeros((16, 16), dtype=torch.bool)
    for bad in ([], [2, 1], [1, 1], [-1], [float("nan")], [46341], list(range(127))):
        with pytest.raises(ValueError):
            distance_zones(m, bad)
    with pytest.raises(ValueError):
        distance_zones(m, [1, 2], side="around")
    with pytest.raises(ValueError):
        distance_zones(m.float(), [1, 2])
    with pytest.raises(TypeError):
        distance_zones(None, [1, 2])
