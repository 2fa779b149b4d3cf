"""The object morphometry kernels (csrc/object_features.hip) against the numpy restatement of tests/object_features_ref.py,
on poisoned memory (every ``torch.empty`` and every ``ops._workspace`` slab starts as 0xFF, as in
tests/test_morphology_gpu.py).

Every integer output is compared with ``array_equal``.  Of the derived fp64 values, those that are one or two correctly
rounded divisions of exact integers (centroid, the central moments, mean_conc, max_conc) are bit-equal to the
restatement.  The device evaluates the other values by the same expression and differs from the restatement only by its
``sqrt`` and ``atan2``, so it gets four times the restatement's OWN largest error against an exact (mpmath, 60 digits)
evaluation over the patterns of this file (every pattern of ``labelled`` at every shape of SHAPES and both
connectivities, the first M_TABLE objects each: OBJECTS_MEASURED = 1856 objects), and never less than 2 ulp; the factor
follows the Dormand-Prince kernel tests.  MEASURED holds those errors (tests/test_object_features_cpu.py measures them
again and checks that BOUND follows from them): axis lengths in ulp(major_axis); equivalent_diameter, std_conc and
inscribed_radius in their own ulp; eccentricity, orientation and compactness absolutely.  The minor axis of a long thin
object is 4 sqrt(l2) with l2 = (t - root) / 2 a difference of nearly equal numbers, which is why the restatement itself
is 52 ulp(major_axis) off on the 3 x 1025 foreground.  The orientation of an isotropic multi-pixel object (l1 - l2 <=
1e-9 l1, l1 > 0) is undefined and not compared: ORIENTATION_SKIPPED = 8 of the 1856 objects.  A single pixel (l1 = 0)
has orientation 0 by definition and IS compared; leaving those out as well, as the bare rule l1 - l2 <= 1e-9 l1 would,
skips 882 of the 1856, far beyond one in ten.

The shape pass's workgroup owns a TILE = 64 x 64 tile, a wave 64 columns of 16 rows; the shapes are the smallest that
cross a wave's 64 columns, a tile, a row wider than one workgroup, and several tiles per object."""
import numpy as np
import pytest
import torch

import morphology_ref as MR
import object_features_ref as F
import objects_ref as O
import stain_quant_ref as SQ

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1), (1, 9), (5, 1), (33, 65), (97, 131), (3, 1025), (300, 520)]
M_TABLE = 48
THR = (0.2, 0.15, 0.1)

# the float64 restatement against the exact evaluation (see the module docstring), measured on the CPU
MEASURED = {"major_axis": 0.923, "minor_axis": 52.3, "equivalent_diameter": 0.707, "std_conc": 0.76,
            "inscribed_radius": 0.5, "eccentricity": 6.29e-16, "orientation": 1.28e-16, "compactness": 9.32e-17}
OBJECTS_MEASURED, ORIENTATION_SKIPPED = 1856, 8
# the floor of 2 ulp: of the value itself (major_axis for both axes; 1.0 for the three absolute ones, whose values lie
# in [0, 1], (-pi/2, pi/2] and (0, 1])
FLOOR = {"major_axis": 2.0, "minor_axis": 2.0, "equivalent_diameter": 2.0, "std_conc": 2.0, "inscribed_radius": 2.0,
         "eccentricity": 2 * 2.0 ** -52, "orientation": 2 * 2.0 ** -52, "compactness": 2 * 2.0 ** -52}
BOUND = {k: max(4 * v, FLOOR[k]) for k, v in MEASURED.items()}


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    from stain2stain_amd import ops
    import torch.utils.deterministic as tud
    prev_det, prev_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    prev_fill = tud.fill_uninitialized_memory
    orig = ops._workspace

    def poisoned(device, numel, tag):
        buf = orig(device, numel, tag)
        buf.view(torch.uint8).fill_(255)
        return buf

    torch.use_deterministic_algorithms(True, warn_only=True)
    tud.fill_uninitialized_memory = True
    try:
        for buf in ops._WORKSPACE.values():
            buf.view(torch.uint8).fill_(255)
        monkeypatch.setattr(ops, "_workspace", poisoned)
        yield orig
    finally:
        torch.use_deterministic_algorithms(prev_det, warn_only=prev_warn)
        tud.fill_uninitialized_memory = prev_fill


def labelled(H, W, connectivity):
    """(name, labels int32 [H, W]) of every pattern: morphology_ref.patterns plus the serpentine and checkerboard of
    objects_ref, labelled by objects_ref.label."""
    for name, m in MR.patterns(H, W, seed=3 * H + W):
        yield name, O.label(m, connectivity)[0]
    yield "serpentine", O.label(O.serpentine(H, W), connectivity)[0]
    yield "objects checkerboard", O.label(O.checkerboard(H, W), connectivity)[0]


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same_ints(got, ref, names, keys):
    for k in keys:
        assert got[k].dtype == F.DTYPES[k] and got[k].shape == ref[k].shape, (k, got[k].dtype, got[k].shape)
        bad = [n for n, g, w in zip(names, got[k], ref[k]) if not np.array_equal(g, w)]
        assert not bad, (k, bad)


def _check_derived(got, ref_tables, names, stats=None):
    """got: numpy dict [B, M, ...]; ref_tables: the restatement's integer tables [B, M, ...]."""
    B = ref_tables["area"].shape[0]
    for n in range(B):
        t = {k: v[n] for k, v in ref_tables.items()}
        d = F.derived(t)
        rows = min(int(t["count"]), t["area"].shape[0])
        pairs = {"centroid_y": got["centroid"][n, :, 0], "centroid_x": got["centroid"][n, :, 1]}
        pairs.update({k: got[k][n] for k in F.DERIVED[2:] if k in got})
        for k in F.EXACT_KEYS:
            if k in pairs:
                assert np.array_equal(pairs[k], d[k]), (names[n], k)
        for k, g in pairs.items():
            assert np.all(g[rows:] == 0), (names[n], k)
        ulp_major = np.spacing(np.where(d["major_axis"] > 0, d["major_axis"], 1.0))
        for k in ("major_axis", "minor_axis"):
            err = np.abs(pairs[k] - d[k]) / ulp_major
            assert np.all(err <= BOUND[k]), (names[n], k, float(err.max()))
        for k in ("equivalent_diameter", "std_conc", "inscribed_radius"):
            if k not in pairs:
                continue
            fin = np.isfinite(d[k])
            assert np.array_equal(np.isinf(pairs[k]), ~fin), (names[n], k)
            err = np.abs(pairs[k][fin] - d[k][fin]) / np.spacing(np.where(d[k][fin] > 0, d[k][fin], 1.0))
            assert np.all(err <= BOUND[k]), (names[n], k, float(err.max(initial=0)))
        for k in ("eccentricity", "compactness"):
            err = np.abs(pairs[k] - d[k])
            assert np.all(err <= BOUND[k]), (names[n], k, float(err.max()))
        skip = F.isotropic(d["l1"], d["l2"])
        err = np.abs(pairs["orientation"] - d["orientation"])[~skip]
        assert np.all(err <= BOUND["orientation"]), (names[n], "orientation", float(err.max(initial=0)))
        if stats is not None:
            stats[0] += int(skip[:rows].sum())
            stats[1] += rows


# ---- the integer tables and the derived values, every pattern -----------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", SHAPES)
def test_every_pattern(H, W, connectivity):
    from stain2stain_amd import object_features
    names, labs = zip(*labelled(H, W, connectivity))
    labs = np.stack(labs)
    d2 = MR.d2_batch(labs > 0)
    ref = F.batch(labs, M_TABLE, d2)
    got = _np(object_features(_gpu(labs), max_objects=M_TABLE))
    assert sorted(got) == sorted(["count", *F.INT_KEYS, "max_d2", "centroid", *F.DERIVED[2:11], "inscribed_radius"])
    _same_ints(got, ref, names, ("count", *F.INT_KEYS, "max_d2"))
    stats = [0, 0]
    _check_derived(got, ref, names, stats)
    assert (ref["count"] > M_TABLE).any() or H * W < 2 * M_TABLE           # the large shapes also exercise count > M
    # the named cases
    i_bg, i_fg = names.index("background"), names.index("foreground")
    assert got["count"][i_bg] == 0 and all(np.all(got[k][i_bg] == 0) for k in got)
    assert got["count"][i_fg] == 1 and got["border"][i_fg, 0] == 1 and got["max_d2"][i_fg, 0] == F.FAR
    assert got["edges"][i_fg, 0] == 2 * (H + W) and got["area"][i_fg, 0] == H * W and np.isinf(got["inscribed_radius"][i_fg, 0])
    # without the thickness pass: the same table, no thickness keys
    thin = _np(object_features(_gpu(labs), max_objects=M_TABLE, thickness=False))
    assert "max_d2" not in thin and "inscribed_radius" not in thin
    for k in thin:
        assert np.array_equal(thin[k], got[k]), k


def test_count_above_the_table_and_untabulated_neighbours():
    from stain2stain_amd import object_features
    lab = O.label(O.bernoulli((150, 200), 0.59, 59), 4)[0]
    n = int(lab.max())
    assert n > 400
    for M in (1, 7, n - 1, n, n + 5):
        got = _np(object_features(_gpu(lab), max_objects=M))
        ref = F.tables(lab, M, MR.d2(lab > 0))
        assert got["count"] == n
        for k in (*F.INT_KEYS, "max_d2"):
            assert np.array_equal(got[k], ref[k]), (M, k)
    # rows beyond the table are never written: a neighbour numbered above M still counts as another label
    small = np.array([[1, 1, 3, 0], [2, 2, 3, 0], [0, 0, 0, 4]], np.int32)
    got = _np(object_features(_gpu(small), max_objects=2, thickness=False))
    assert got["count"] == 4 and got["edges"].tolist() == [6, 6] and got["boundary"].tolist() == [2, 2]


def test_more_labels_in_a_tile_than_the_lds_table_holds():
    from stain2stain_amd import object_features
    from stain2stain_amd.object_features import LDS_SLOTS, TILE
    # isolated pixels on a grid of pitch 2: (TILE_H / 2) * (TILE_W / 2) labels per tile, sixteen times the table, in raster
    # order, so neighbouring labels hash to neighbouring slots; and 3 x 3 blocks of LDS_SLOTS + 9 labels in one tile
    H, W = TILE[0] + 7, 2 * TILE[1] + 5
    m = np.zeros((H, W), np.uint8)
    m[::2, ::2] = 1
    lab = O.label(m, 8)[0]
    per_tile = len(np.unique(lab[:TILE[0], :TILE[1]])) - 1
    assert per_tile > 4 * LDS_SLOTS
    blocks = np.zeros((H, W), np.uint8)
    for i in range(LDS_SLOTS + 9):
        y, x = 4 * (i // 14), 4 * (i % 14)
        blocks[y:y + 3, x:x + 3] = 1
    lab2 = O.label(blocks, 4)[0]
    assert lab2.max() == LDS_SLOTS + 9 and lab2[:TILE[0], :TILE[1]].max() == LDS_SLOTS + 9
    labs = np.stack([lab, lab2])
    M = int(labs.max())
    got = _np(object_features(_gpu(labs), max_objects=M))
    ref = F.batch(labs, M, MR.d2_batch(labs > 0))
    _same_ints(got, ref, ("grid", "blocks"), ("count", *F.INT_KEYS, "max_d2"))
    _check_derived(got, ref, ("grid", "blocks"))


def test_diagonal_contact_batch_isolation_and_no_batch_dimension():
    from stain2stain_amd import object_features
    m = np.zeros((70, 90), np.uint8)
    m[0:30, 0:30] = 1
    m[30:66, 30:90] = 1                                     # touches the first block at one corner only
    lab4, lab8 = O.label(m, 4)[0], O.label(m, 8)[0]
    assert lab4.max() == 2 and lab8.max() == 1
    rng = O.bernoulli((70, 90), 0.45, 7)
    labs = np.stack([lab4, lab8, O.label(rng, 8)[0], np.zeros((70, 90), np.int32)])
    whole = object_features(_gpu(labs), max_objects=40)
    ref = F.batch(labs, 40, MR.d2_batch(labs > 0))
    _same_ints(_np(whole), ref, ("conn4", "conn8", "random", "empty"), ("count", *F.INT_KEYS, "max_d2"))
    # with connectivity 4 the diagonal neighbour is another object, not background: the distance sees one body
    assert ref["max_d2"][0, 0] == ref["max_d2"][1, 0] or ref["max_d2"][0, 1] == ref["max_d2"][1, 0]
    for n in range(4):
        alone = object_features(_gpu(labs[n:n + 1]), max_objects=40)
        single = object_features(_gpu(labs[n]), max_objects=40)
        for k, v in whole.items():
            assert torch.equal(alone[k][0], v[n]), (n, k)                 # bit-equal alone and inside a batch
            assert single[k].shape == v.shape[1:] and torch.equal(single[k], v[n]), (n, k)
    view = torch.zeros((4, 75, 99), dtype=torch.int32, device=DEV)[:, 2:72, 3:93]
    view.copy_(_gpu(labs))
    assert not view.is_contiguous()
    for k, v in object_features(view, max_objects=40).items():
        assert torch.equal(v, whole[k]), k


# ---- intensity ----------------------------------------------------------------------------------------------------------
def _plaques(B, H, W, seed, discs=14):
    """uint8 [B, H, W, 3]: haematoxylin background, DAB discs of mixed sizes, speckle and noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    conc = np.zeros((B, H, W, 3))
    conc[..., 0] = rng.uniform(0.05, 0.5, size=(B, H, W))
    conc[..., 1] = np.where(rng.random((B, H, W)) < 0.03, rng.uniform(0.3, 1.0, size=(B, H, W)), 0.02)
    for n in range(B):
        for _ in range(discs):
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1.5, 9.0)
            conc[n, ..., 1][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.uniform(0.5, 4.5)     # some beyond the grid's 4
    img = SQ.synthesise(conc, "hdab").astype(np.int32) + rng.integers(-3, 4, size=(B, H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _network(u8, seed):
    rng = np.random.default_rng(seed)
    lv = u8.astype(np.float64).transpose(0, 3, 1, 2) + rng.random(u8.transpose(0, 3, 1, 2).shape) * 0.98
    return np.ascontiguousarray((lv / 127.5 - 1.0).astype(np.float32))


TILES = _plaques(3, 97, 263, 17)
TILES[:, 5, 5] = (0, 0, 255)                      # a haematoxylin concentration beyond 4: q stops at 4095


def _m32():
    from stain2stain_amd.stain_quant import unmix_matrix
    return unmix_matrix("hdab").numpy()


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_intensity_and_the_one_call_form(kind):
    from stain2stain_amd import object_features, stain_object_features, stain_objects
    if kind == "u8":
        inp, u8 = _gpu(TILES), TILES
    else:
        x = _network(TILES, 23)
        inp, u8 = _gpu(x), SQ.nchw_to_u8(x)
    names = [f"sample {n}" for n in range(len(u8))]
    for stain, conn, M in ((1, 8, 40), (0, 4, 9)):
        objs = stain_objects(inp, stain=stain, thresholds=THR, connectivity=conn, mpp=0.5, return_labels=True)
        labs = objs["labels"].cpu().numpy()
        pos = SQ.positive32(u8, _m32(), THR)[..., stain].astype(np.uint8)
        assert np.array_equal(labs, np.stack([O.label(p, conn)[0] for p in pos]))
        q = F.quantise(u8, _m32(), stain)
        ref = F.batch(labs, M, MR.d2_batch(labs > 0), q)
        f = object_features(objs["labels"], max_objects=M, image=inp, stain=stain, mpp=0.5)
        got = _np(f)
        _same_ints(got, ref, names, ("count", *F.INT_KEYS, "max_d2", *F.Q_KEYS))
        _check_derived(got, ref, names)
        assert ref["max_q"].max() == (4095 if stain == 0 else ref["max_q"].max()) > 1024 and (ref["sum_q"] > 0).any()
        assert np.array_equal(got["area_um2"], ref["area"].astype(np.float64) * 0.25)
        for k in ("equivalent_diameter", "major_axis", "minor_axis", "inscribed_radius"):
            assert np.array_equal(got[k + "_um"], got[k] * 0.5), k
        one = stain_object_features(inp, max_objects=M, stain=stain, thresholds=THR, connectivity=conn, mpp=0.5,
                                    return_labels=True)
        assert sorted(one) == sorted({*f, *objs})
        for k, v in one.items():
            want = f[k] if k in f else objs[k]
            assert v.dtype == want.dtype and torch.equal(v, want), (kind, stain, k)
    # a batch of one image against a [H, W] label image; the intensity keys are absent without an image
    lab0 = objs["labels"][0]
    img0 = inp[0]
    a, b = object_features(lab0, 9, image=img0, stain=0), object_features(objs["labels"][:1], 9, image=inp[:1], stain=0)
    for k in a:
        assert torch.equal(a[k], b[k][0]), k
    assert not {"sum_q", "mean_conc", "std_conc", "max_conc"} & set(object_features(lab0, 9))


def test_u8_crop_view():
    from stain2stain_amd import object_features, stain_objects
    B, H, W, _ = TILES.shape
    big = torch.full((B, H + 5, W + 6, 3), 77, dtype=torch.uint8, device=DEV)
    view = big[:, 2:2 + H, 3:3 + W]
    view.copy_(torch.from_numpy(TILES))
    labels = stain_objects(view, thresholds=THR, return_labels=True)["labels"]
    a = object_features(labels, 30, image=view)
    b = object_features(labels, 30, image=_gpu(TILES))
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- whole regions ----------------------------------------------------------------------------------------------------
def test_region_bands_host_and_gpu():
    from stain2stain_amd import region_stain_object_features
    H, W = 200, 300
    region = _plaques(1, H, W, 29, discs=40)[0]
    for top in (10, 42, 90, 138, 186):                                        # an object across every seam of 16 and 48 rows
        region[top:top + 12, 100 + top:130 + top] = SQ.synthesise([0.1, 1.0, 0.0], "hdab")
    M = 64
    pos = SQ.positive32(region, _m32(), THR)[..., 1].astype(np.uint8)
    lab = O.label(pos, 8, 4)[0]
    for top in (10, 42, 90, 138, 186):
        blk = lab[top:top + 12, 100 + top:130 + top]
        assert blk.min() > 0 and (blk == blk[0, 0]).all()
    ref = F.tables(lab, M, MR.d2(lab > 0), F.quantise(region, _m32(), 1))
    ref_b = {k: v[None] for k, v in ref.items()}
    host = torch.from_numpy(region)
    padded = torch.zeros((H, W + 3, 3), dtype=torch.uint8, device=DEV)
    view = padded[:, 1:1 + W]
    view.copy_(host)
    first = None
    for band_rows in (16, 48, None):
        for src, name in ((host, "host"), (host.to(DEV), "gpu"), (view, "gpu view")):
            got = region_stain_object_features(src, max_objects=M, band_rows=band_rows, thresholds=THR, min_area=4,
                                               mpp=0.5, return_labels=True)
            assert all(v.is_cuda for v in got.values()) and got["count"].dim() == 0 and got["area"].shape == (M,)
            if first is None:
                first = got
                g = _np(got)
                assert np.array_equal(g["labels"], lab)
                for k in ("count", *F.INT_KEYS, "max_d2", *F.Q_KEYS):
                    assert g[k].dtype == F.DTYPES[k] and np.array_equal(g[k], ref[k]), k
                _check_derived({k: v[None] for k, v in g.items()}, ref_b, ["region"])
                assert int(g["count"]) > 20
            for k, v in got.items():
                assert torch.equal(v, first[k]), (name, band_rows, k)         # bit-equal for every banding and source


# ---- the summary --------------------------------------------------------------------------------------------------------
def _summary_ref(f, exclude_border):
    """numpy on the returned table, one sample."""
    M = f["area"].shape[0]
    keep = (np.arange(M) < int(f["count"])) & (f["area"] > 0)
    if exclude_border:
        keep &= f["border"] == 0
    n = int(keep.sum())
    out = {"objects": n, "valid": int(n > 0), "median_area": 0.0}
    w = f["area"][keep].astype(np.float64)
    for name in ("eccentricity", "compactness", "mean_conc", "inscribed_radius"):
        if name in f:
            v = f[name][keep]
            out[name + "_mean"] = float(v.sum() / n) if n else 0.0
            out[name + "_area_mean"] = float((v * w).sum() / w.sum()) if n else 0.0
    if n:
        out["median_area"] = float(np.sort(f["area"][keep])[(n + 1) // 2 - 1])
    return out


def test_object_feature_summary():
    from stain2stain_amd import object_feature_summary, stain_object_features
    img = np.concatenate([TILES, np.full((1, *TILES.shape[1:]), 255, np.uint8)])           # the last sample is empty glass
    f = stain_object_features(_gpu(img), max_objects=40, thresholds=THR, min_area=3)
    fn = _np(f)
    assert fn["count"][-1] == 0 and (fn["count"][:-1] > 5).all() and fn["border"].any()
    for exclude in (True, False):
        s = _np(object_feature_summary(f, exclude_border=exclude))
        assert s["objects"].dtype == np.int64 and s["valid"].dtype == np.int32
        for n in range(len(img)):
            ref = _summary_ref({k: v[n] for k, v in fn.items()}, exclude)
            assert sorted(ref) == sorted(s)
            for k, want in ref.items():
                got = s[k][n]
                if np.isinf(want):
                    assert np.isinf(got), (exclude, n, k)
                else:
                    assert got == pytest.approx(want, rel=1e-12, abs=0), (exclude, n, k, got, want)
        assert s["valid"][-1] == 0 and all(s[k][-1] == 0 for k in s)
    a, b = object_feature_summary(f, True), object_feature_summary(f, False)
    assert (a["objects"] < b["objects"]).any()
    one = object_feature_summary({k: v[0] for k, v in f.items()})
    assert one["objects"].dim() == 0 and torch.equal(one["median_area"], a["median_area"][0])


# ---- no hidden synchronisation ----------------------------------------------------------------------------------------
def test_does_not_synchronise():
    from stain2stain_amd import object_feature_summary, object_features, stain_object_features
    inp = _gpu(TILES)
    f = stain_object_features(inp, max_objects=16, thresholds=THR, return_labels=True)      # the workspaces exist from here on
    labels = f["labels"]
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = object_features(labels, 16, image=inp, mpp=0.5)
        b = stain_object_features(inp, max_objects=16, thresholds=THR, mpp=0.5)
        c = object_feature_summary(b)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(a["sum_q"], b["sum_q"]) and int(c["objects"].sum()) > 0
