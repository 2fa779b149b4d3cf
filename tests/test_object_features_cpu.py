"""Object morphometry without a GPU: the restatement of tests/object_features_ref.py against scipy.ndimage and against its
own brute-force form, the closed forms of rectangles, single pixels and diagonals, why the finalize forms its numerators
in 128 bits, the restatement's own error against an exact evaluation (what the GPU test's bounds rest on), the exports,
the status codes of the s2s_objfeat_* entry points (returned before any HIP call) and the argument checks the wrappers
make before they touch the device."""
import math

import numpy as np
import pytest
import torch
from scipy import ndimage

import morphology_ref as MR
import object_features_ref as F
import objects_ref as O

SMALL = [(1, 1), (1, 9), (5, 1), (23, 31), (33, 65)]
NEW_SYMBOLS = ["s2s_objfeat_shape", "s2s_objfeat_intensity_u8", "s2s_objfeat_intensity_f32", "s2s_objfeat_finalize"]
NEW_NAMES = ("object_features", "stain_object_features", "region_stain_object_features", "object_feature_summary")


def _cases(H, W):
    for name, m in MR.patterns(H, W, seed=H * W):
        yield name, m
    yield "serpentine", O.serpentine(H, W)
    yield "objects checkerboard", O.checkerboard(H, W)


# ---- the restatement against scipy and against itself -------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", SMALL)
def test_tables_equal_scipy_and_brute_force(H, W, connectivity):
    rng = np.random.default_rng(H * 100 + W)
    q = rng.integers(0, 4096, size=(H, W))
    for name, m in _cases(H, W):
        lab, n, area = O.label(m, connectivity)
        d2 = MR.d2(lab > 0)
        M = max(n, 1)
        t = F.tables(lab, M, d2, q)
        brute = F.tables_brute(lab, M, d2, q)
        for k in t:
            assert np.array_equal(t[k], brute[k]), (name, k)
            assert np.asarray(t[k]).dtype == F.DTYPES[k], (name, k)
        assert t["count"] == n
        if n == 0:
            continue
        idx = np.arange(1, n + 1)
        assert np.array_equal(t["area"][:n], area)
        assert np.array_equal(t["area"][:n], ndimage.sum_labels(np.ones_like(lab), lab, idx).astype(np.int64))
        yy, xx = np.mgrid[0:H, 0:W]
        for col, w in enumerate((yy, xx, yy * yy, xx * xx, yy * xx)):
            assert np.array_equal(t["moments"][:n, col], ndimage.sum_labels(w.astype(np.float64), lab, idx).astype(np.int64))
        assert np.array_equal(t["max_d2"][:n], ndimage.maximum(d2, lab, idx).astype(np.int32))
        assert np.array_equal(t["max_q"][:n], ndimage.maximum(q, lab, idx).astype(np.int32))
        assert np.array_equal(t["sum_q"][:n], ndimage.sum_labels(q.astype(np.float64), lab, idx).astype(np.int64))
        for r, sl in enumerate(ndimage.find_objects(lab)):
            assert tuple(t["bbox"][r]) == (sl[0].start, sl[1].start, sl[0].stop, sl[1].stop), (name, r)
        com = np.array(ndimage.center_of_mass(np.ones_like(lab), lab, idx))
        d = F.derived(t)
        assert np.allclose(com[:, 0], d["centroid_y"][:n], rtol=1e-13, atol=0)
        assert np.allclose(com[:, 1], d["centroid_x"][:n], rtol=1e-13, atol=0)
        # boundary of a single object is mask_boundary of that object alone; max_d2 is the maximum of the distance
        # transform of labels > 0 over the object
        for k in range(1, min(n, 6) + 1):
            assert t["boundary"][k - 1] == MR.boundary(lab == k).sum(), (name, k)
            assert t["max_d2"][k - 1] == MR.d2(lab > 0)[lab == k].max(), (name, k)


def test_count_above_the_table_and_untabulated_neighbours():
    lab = np.array([[1, 1, 3, 0], [2, 2, 3, 0], [0, 0, 0, 4]], np.int32)
    t = F.tables(lab, 2)
    assert t["count"] == 4 and t["area"].tolist() == [2, 2]
    assert t["edges"].tolist() == [6, 6] and t["boundary"].tolist() == [2, 2]      # label 3 is another label, not tabulated
    assert t["border"].tolist() == [1, 1] and t["bbox"].tolist() == [[0, 0, 1, 2], [1, 0, 2, 2]]
    # connectivity-4 objects that touch diagonally: the other object is not background for the distance
    m = np.zeros((6, 6), np.uint8)
    m[0:3, 0:3] = 1
    m[3:6, 3:6] = 1
    lab, n, _ = O.label(m, 4)
    assert n == 2
    t = F.tables(lab, 4, MR.d2(lab > 0))
    assert t["edges"].tolist()[:2] == [12, 12] and t["max_d2"].tolist()[:2] == [9, 9]
    lab8, n8, _ = O.label(m, 8)
    assert n8 == 1 and F.tables(lab8, 4)["edges"][0] == 24


# ---- closed forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(1, 1), (1, 7), (6, 1), (2, 2), (5, 5), (4, 9), (12, 3)])
def test_rectangles(a, b):
    lab = np.zeros((a + 4, b + 5), np.int32)
    lab[2:2 + a, 3:3 + b] = 1
    t = F.tables(lab, 1, MR.d2(lab > 0))
    assert t["edges"][0] == 2 * (a + b) and t["boundary"][0] == a * b - max(a - 2, 0) * max(b - 2, 0)
    assert t["border"][0] == 0 and tuple(t["bbox"][0]) == (2, 3, 2 + a, 3 + b)
    assert tuple(int(v) for v in (t["area"][0], *t["moments"][0])) == F.rectangle_sums(2, 3, a, b)
    d = F.derived(t)
    assert d["mu_yy"][0] == pytest.approx((a * a - 1) / 12, rel=1e-15) and d["mu_xx"][0] == pytest.approx((b * b - 1) / 12, rel=1e-15)
    assert d["mu_yx"][0] == 0
    if a == b:
        assert d["eccentricity"][0] == 0 and d["orientation"][0] == 0 and d["major_axis"][0] == d["minor_axis"][0]
    else:
        assert d["orientation"][0] == (0.0 if b > a else math.pi / 2)
        assert d["major_axis"][0] == pytest.approx(4 * math.sqrt((max(a, b) ** 2 - 1) / 12), rel=1e-15)
    if a == b == 1:
        assert all(d[k][0] == 0 for k in ("major_axis", "minor_axis", "eccentricity", "orientation", "mu_yy", "mu_xx"))
        assert d["compactness"][0] == pytest.approx(math.pi / 4) and d["inscribed_radius"][0] == 1
    assert d["inscribed_radius"][0] == pytest.approx((min(a, b) + 1) // 2)
    assert d["equivalent_diameter"][0] == pytest.approx(math.sqrt(4 * a * b / math.pi), rel=1e-15)
    assert d["centroid_y"][0] == 2 + (a - 1) / 2 and d["centroid_x"][0] == 3 + (b - 1) / 2


def test_diagonal_line_disc_and_whole_image():
    for n in (2, 7, 40):
        t = F.tables(np.eye(n, dtype=np.int32), 1)
        d = F.derived(t)
        assert d["l2"][0] == 0.0 and d["minor_axis"][0] == 0.0 and d["eccentricity"][0] == 1.0
        assert d["orientation"][0] == math.pi / 4
        anti = F.derived(F.tables(np.eye(n, dtype=np.int32)[:, ::-1], 1))
        assert anti["orientation"][0] == -math.pi / 4 and anti["l2"][0] == 0.0
    disc = MR.discs(101, 101, [(50, 50, 40)]).astype(np.int32)
    d = F.derived(F.tables(disc, 1, MR.d2(disc > 0)))
    assert 0.58 < d["compactness"][0] < 0.64            # the crack length of a disc is 8 r, not 2 pi r: pi^2 / 16 = 0.617
    assert d["eccentricity"][0] == 0 and abs(d["major_axis"][0] - 80) < 1.5 and abs(d["inscribed_radius"][0] - 41) <= 1
    full = np.ones((7, 9), np.int32)
    t = F.tables(full, 3, MR.d2(full > 0))
    assert t["edges"][0] == 2 * (7 + 9) and t["border"][0] == 1 and t["max_d2"][0] == F.FAR and t["area"][1] == 0
    assert F.derived(t)["inscribed_radius"][0] == math.inf
    empty = F.tables(np.zeros((4, 5), np.int32), 3)
    assert empty["count"] == 0 and all(np.all(empty[k] == 0) for k in F.INT_KEYS)


def test_why_the_numerators_are_formed_in_128_bits():
    """A 3000 x 3100 object with its far corner at (32766, 32766): A * sum(y^2) and (sum y)^2 are near 2^76, beyond int64,
    and agree in their leading digits, so the float64 form of their difference is off by hundreds of ulp while the exact
    integer, converted once, is right to the last place; an int64 product wraps."""
    a, b = 3000, 3100
    A, sy, sx, syy, sxx, syx = F.rectangle_sums(32767 - a, 32767 - b, a, b)
    assert syy < 2 ** 61 and sxx < 2 ** 61 and syx < 2 ** 61 and A < 2 ** 31
    exact = A * syy - sy * sy
    assert exact == A * A * (a * a - 1) // 12 and A * syy > 2 ** 64
    naive = float(A) * float(syy) - float(sy) * float(sy)
    assert naive != float(exact)
    assert abs(naive - float(exact)) > 64 * np.spacing(float(exact))          # not a rounding error in the last place
    d = F.derived_row(A, sy, sx, syy, sxx, syx, 2 * (a + b))
    assert d["mu_yy"] == pytest.approx((a * a - 1) / 12, rel=4e-16) and d["mu_xx"] == pytest.approx((b * b - 1) / 12, rel=4e-16)
    assert d["mu_yx"] == 0.0 and d["orientation"] == 0.0
    with np.errstate(over="ignore"):
        assert A * syy != int(np.int64(A) * np.int64(syy))


# ---- the restatement's own error: what the GPU test's bounds rest on ----------------------------------------------------
def test_restatement_error_is_what_the_gpu_bounds_rest_on():
    """tests/test_object_features_gpu.py gives the device four times the largest error of the float64 restatement against
    the exact evaluation, never less than 2 ulp.  The errors are measured here over that file's whole pattern set (a
    random q image per shape for std_conc); its MEASURED constants must be these values (rounded up in the third digit),
    BOUND must follow from them, and the share of objects whose orientation is not compared must stay below one in ten."""
    import test_object_features_gpu as G           # the constants live next to the assertions that use them
    worst = {}
    skipped = total = 0
    for H, W in G.SHAPES:
        q = np.random.default_rng(H + W).integers(0, 4096, size=(H, W))
        for conn in (4, 8):
            for name, lab in G.labelled(H, W, conn):
                t = F.tables(lab, G.M_TABLE, MR.d2(lab > 0), q)
                for k, v in F.restatement_errors(t).items():
                    worst[k] = max(worst.get(k, 0.0), v)
                d = F.derived(t)
                n = min(int(t["count"]), G.M_TABLE)
                skipped += int(F.isotropic(d["l1"][:n], d["l2"][:n]).sum())
                total += n
    print("restatement errors:", worst, "orientation skipped", skipped, "of", total)
    assert sorted(worst) == sorted(G.MEASURED)
    for k, v in worst.items():
        assert 0.98 * G.MEASURED[k] <= v <= G.MEASURED[k], (k, v, G.MEASURED[k])
    assert total == G.OBJECTS_MEASURED and skipped == G.ORIENTATION_SKIPPED and skipped * 10 <= total
    for k, v in G.MEASURED.items():
        assert G.BOUND[k] == max(4 * v, G.FLOOR[k]), k


# ---- exports ----------------------------------------------------------------------------------------------------------
def test_exports():
    import stain2stain_amd
    import importlib
    from stain2stain_amd import _native
    object_features = importlib.import_module("stain2stain_amd.object_features")     # (the package attribute is the function)
    for name in NEW_NAMES:
        assert name in stain2stain_amd.__all__ and getattr(stain2stain_amd, name) is getattr(object_features, name), name
    assert "object_features.hip" in _native.SOURCES
    declared = _native.declared_symbols()
    _native.build()
    lib = _native.lib()
    for sym in NEW_SYMBOLS:
        assert sym in declared and hasattr(lib, sym), sym
    assert object_features.TILE == (64, 64) and object_features.LDS_SLOTS == 64 and object_features.N_DERIVED == 15
    assert object_features.MAX_SIDE == 32767 and object_features.FAR == 2 ** 31 - 1
    src = open(_native.CSRC + "/object_features.hip").read()
    assert "getenv" not in src and "atomicAdd(float" not in src.replace(" ", "")


# ---- status codes of the entry points: returned before any HIP call ---------------------------------------------------
def test_entry_points_return_status_codes():
    from stain2stain_amd import _native
    lib = _native.lib()
    X = 4096                                      # a non-null pointer that is never dereferenced: every call below fails first

    def shape(**kw):
        a = dict(labels=X, d2=0, B=1, H=32, W=64, M=4, count=X, area=X, bbox=X, moments=X, edges=X, boundary=X, border=X,
                 max_d2=0)
        a.update(kw)
        return lib.s2s_objfeat_shape(*a.values(), None)

    for k in ("labels", "count", "area", "bbox", "moments", "edges", "boundary", "border"):
        assert shape(**{k: 0}) == -5, k
    assert shape(d2=X) == -5                                        # a distance map needs its table
    for bad in ({"M": 0}, {"M": -3}, {"H": 32768}, {"W": 32768}, {"H": 0}, {"W": -1}, {"B": 0}, {"B": 65536},
                {"B": 65535, "M": 2 ** 16}):
        assert shape(**bad) == -1, bad
        assert shape(d2=X, max_d2=X, **bad) == -1, bad

    od, un = (np.zeros(256, np.float32), np.zeros(12, np.float32))
    odp, unp = od.ctypes.data, un.ctypes.data

    def u8(**kw):
        a = dict(labels=X, img=X, pitch=192, stride=192 * 32, B=1, top=0, band=32, H=32, W=64, M=4, od=odp, un=unp, stain=1,
                 sq=X, sq2=X, mq=X)
        a.update(kw)
        return lib.s2s_objfeat_intensity_u8(*a.values(), None)

    def f32(**kw):
        a = dict(labels=X, img=X, B=1, H=32, W=64, M=4, od=odp, un=unp, stain=1, sq=X, sq2=X, mq=X)
        a.update(kw)
        return lib.s2s_objfeat_intensity_f32(*a.values(), None)

    for f in (u8, f32):
        for k in ("labels", "img", "od", "un", "sq", "sq2", "mq"):
            assert f(**{k: 0}) == -5, k
        for bad in ({"M": 0}, {"H": 32768}, {"W": 32768}, {"B": 0}, {"B": 65536}, {"stain": 3}, {"stain": -1}):
            assert f(**bad) == -1, bad
    assert u8(pitch=191) == -1 and u8(top=-1) == -1 and u8(band=0) == -1 and u8(top=1) == -1 and u8(top=16, band=17) == -1
    assert u8(B=2, stride=192 * 31) == -1

    def fin(**kw):
        a = dict(count=X, area=X, moments=X, edges=X, sq=0, sq2=0, mq=0, md2=0, B=1, M=4, out=X)
        a.update(kw)
        return lib.s2s_objfeat_finalize(*a.values(), None)

    for k in ("count", "area", "moments", "edges", "out"):
        assert fin(**{k: 0}) == -5, k
    assert fin(sq=X) == -5 and fin(sq=X, sq2=X) == -5
    assert fin(M=0) == -1 and fin(B=0) == -1 and fin(B=65536) == -1 and fin(B=65535, M=2 ** 16) == -1


# ---- argument checks that need no GPU ---------------------------------------------------------------------------------
def test_wrappers_reject_before_the_gpu():
    from stain2stain_amd import (object_feature_summary, object_features, region_stain_object_features,
                                 stain_object_features)
    lab = torch.zeros((2, 16, 16), dtype=torch.int32)
    with pytest.raises(TypeError):
        object_features(lab.numpy())
    for bad in (lab.long(), lab.float(), lab.to(torch.uint8), lab[0, 0], lab[None], torch.zeros((0, 4, 4), dtype=torch.int32),
                torch.zeros((2, 0, 4), dtype=torch.int32), torch.zeros((1, 1), dtype=torch.int32).expand(32768, 4),
                torch.zeros((1, 1), dtype=torch.int32).expand(4, 32768)):
        with pytest.raises(ValueError):
            object_features(bad)
    for M in (0, -1):
        with pytest.raises(ValueError):
            object_features(lab, max_objects=M)
    with pytest.raises(TypeError):
        object_features(lab, max_objects=2.5)
    with pytest.raises(ValueError):
        object_features(lab, mpp=0)
    u8 = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(TypeError):
        object_features(lab, image=u8.numpy())
    for img in (u8[:, :15], u8[:1], u8.float(), torch.zeros((2, 3, 16, 15)), u8.to(torch.int16), u8[0]):
        with pytest.raises(ValueError):
            object_features(lab, image=img)
    with pytest.raises(ValueError):
        object_features(lab, image=u8, stain=3)
    with pytest.raises(ValueError):
        object_features(lab, image=u8, stains="nope")
    # everything valid but on the host: there is no CPU path
    for call in (lambda: object_features(lab), lambda: object_features(lab[0], image=u8[0]),
                 lambda: stain_object_features(u8), lambda: stain_object_features(torch.zeros((2, 3, 16, 16)))):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    for kw in ({"max_objects": 0}, {"connectivity": 6}, {"min_area": 0}, {"stain": 5}, {"white": 0}, {"mpp": -1.0}):
        with pytest.raises(ValueError):
            stain_object_features(u8, **kw)
        with pytest.raises(ValueError):
            region_stain_object_features(u8[0], **kw)
    with pytest.raises(ValueError):
        stain_object_features(torch.zeros((1, 2, 32768, 3), dtype=torch.uint8))
    with pytest.raises(TypeError):
        region_stain_object_features(u8[0].numpy())
    with pytest.raises(ValueError):
        region_stain_object_features(u8)
    with pytest.raises(ValueError):
        region_stain_object_features(u8[0], band_rows=8)
    with pytest.raises(TypeError):
        object_feature_summary(lab)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            region_stain_object_features(u8[0])


def test_summary_runs_on_any_device():
    """object_feature_summary is plain torch: on a host table it gives what numpy gives."""
    from stain2stain_amd import object_feature_summary
    area = torch.tensor([[5, 9, 2, 0], [0, 0, 0, 0], [4, 4, 7, 1]])
    f = {"count": torch.tensor([3, 0, 9], dtype=torch.int32), "area": area,
         "border": torch.tensor([[0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]], dtype=torch.int32),
         "eccentricity": torch.tensor([[0.5, 0.9, 0.1, 0.0], [0.0] * 4, [0.2, 0.4, 0.6, 0.8]], dtype=torch.float64),
         "compactness": torch.ones((3, 4), dtype=torch.float64)}
    s = object_feature_summary(f, exclude_border=True)
    assert s["objects"].tolist() == [2, 0, 3] and s["valid"].tolist() == [1, 0, 1]
    assert s["median_area"].tolist() == [2.0, 0.0, 4.0]
    assert s["eccentricity_mean"].tolist() == pytest.approx([0.3, 0.0, 0.4])
    assert s["eccentricity_area_mean"].tolist() == pytest.approx([(0.5 * 5 + 0.1 * 2) / 7, 0.0, (0.8 + 1.6 + 4.2) / 15])
    s = object_feature_summary(f, exclude_border=False)
    assert s["objects"].tolist() == [3, 0, 4] and s["median_area"].tolist() == [5.0, 0.0, 4.0]
    assert "mean_conc_mean" not in s and s["compactness_mean"].tolist() == [1.0, 0.0, 1.0]
    one = object_feature_summary({k: v[0] for k, v in f.items()})
    assert one["objects"].dim() == 0 and int(one["objects"]) == 2
