"""The object-analysis kernels (csrc/objects.hip, the mask kernels of csrc/stain_quant.hip) against the scipy restatement of
tests/objects_ref.py, on poisoned memory (every ``torch.empty`` and every ``ops._workspace`` slab starts as 0xFF, as in
tests/test_stain_quant_gpu.py).

Every comparison is exact (``array_equal``): labels, counts, areas, boxes and histograms are integers, and the centroid,
the burden, the density and the agreement ratios are each one correctly rounded division of exact integers, compared bit
for bit with the same expression in numpy.

The local pass labels tiles of T_h x T_w = 32 x 64 pixels; the numbering scan works in chunks of 1024 raster indices, 256
chunks per step of its one workgroup: 512 x 512 = 256 chunks is the smallest square that fills a step, 520 x 520 = 265
chunks needs a second one."""
import numpy as np
import pytest
import torch

import objects_ref as O
import stain_quant_ref as R
from stain2stain_amd import (label_components, region_stain_objects, stain_object_agreement, stain_objects,
                             stain_quantify)
from stain2stain_amd.objects import TILE
from stain2stain_amd.stain_quant import unmix_matrix

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_H, T_W = TILE
THR = (0.2, 0.15, 0.1)
TABLE = ("area", "bbox", "centroid")
DTYPES = {"labels": np.int32, "count": np.int32, "kept_pixels": np.int64, "largest": np.int32, "size_hist": np.int64,
          "area": np.int32, "bbox": np.int32, "centroid": np.float32}


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


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same(got, ref, what):
    """Every key of ``ref`` bit for bit, and no key beyond it."""
    got = _np(got)
    assert sorted(got) == sorted(ref), what
    for k, want in ref.items():
        want = np.asarray(want)
        assert got[k].dtype == DTYPES[k] and got[k].shape == want.shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want), (what, k)


def _check(masks, connectivity, min_area=1, max_objects=None, what=""):
    """label_components of a [B, H, W] numpy mask against the reference; returns the GPU result."""
    got = label_components(torch.from_numpy(masks).to(DEV), connectivity=connectivity, min_area=min_area,
                           max_objects=max_objects)
    _same(got, O.batch(masks, connectivity, min_area, max_objects), f"{what} conn {connectivity} min_area {min_area}")
    return got


# ---- shapes and patterns ----------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 9), (5, 1), (T_H - 1, T_W + 1), (2 * T_H + 1, 2 * T_W + 3), (97, 131)]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_empty_full_random_serpentine(H, W, connectivity):
    empty, full = np.zeros((1, H, W), np.uint8), np.ones((1, H, W), np.uint8)
    got = _check(empty, connectivity, max_objects=3, what="empty")
    assert int(got["count"][0]) == 0 and int(got["labels"].abs().max()) == 0
    got = _check(full, connectivity, max_objects=3, what="full")
    assert int(got["count"][0]) == 1 and int(got["largest"][0]) == H * W
    assert got["bbox"][0, 0].tolist() == [0, 0, H, W]
    _check(np.stack([O.bernoulli((H, W), p, 7 * H + W + i) for i, p in enumerate((0.3, 0.5, 0.7))]), connectivity,
           max_objects=16, what=f"random {H}x{W}")
    snake = O.serpentine(H, W)[None]
    got = _check(snake, connectivity, max_objects=2, what=f"serpentine {H}x{W}")
    assert int(got["count"][0]) == 1


@pytest.mark.parametrize("connectivity", [4, 8])
def test_serpentine_crosses_every_seam(connectivity):
    for H, W in ((97, 131), (200, 70)):
        got = _check(O.serpentine(H, W)[None], connectivity, max_objects=2, what=f"serpentine {H}x{W}")
        assert int(got["count"][0]) == 1 and int(got["largest"][0]) == int(O.serpentine(H, W).sum())


def test_checkerboard_one_object_or_all_singletons():
    board = O.checkerboard(65, 67)[None]
    assert int(_check(board, 8, max_objects=4, what="checkerboard")["count"][0]) == 1
    got = _check(board, 4, max_objects=2178, what="checkerboard")
    assert int(got["count"][0]) == 2178 and int(got["largest"][0]) == 1 and int(got["size_hist"][0, 0]) == 2178
    # the numbers run along the raster: object k is the k-th foreground pixel
    assert torch.equal(got["labels"][0][torch.from_numpy(board[0]).to(DEV) > 0],
                       torch.arange(1, 2179, dtype=torch.int32, device=DEV))


def test_diagonals_pass_through_tile_corners():
    for d in O.diagonals(130):
        assert int(_check(d[None], 8, max_objects=2, what="diagonal")["count"][0]) == 1
        assert int(_check(d[None], 4, max_objects=130, what="diagonal")["count"][0]) == 130


BERNOULLI = {8: O.bernoulli((3, 150, 200), 0.41, 41), 4: O.bernoulli((3, 150, 200), 0.59, 59)}


@pytest.mark.parametrize("connectivity", [4, 8])
def test_bernoulli_near_percolation(connectivity):
    masks = BERNOULLI[connectivity]
    got = _check(masks, connectivity, max_objects=64, what="percolation")
    n = got["count"].cpu().numpy()
    print(f"conn {connectivity}: counts {n.tolist()}, largest {got['largest'].tolist()}, "
          f"bins used {(got['size_hist'] > 0).sum(1).tolist()}")
    assert (n > 100).all()
    _check(O.bernoulli((2, 150, 200), 0.5, 50 + connectivity), connectivity, max_objects=8, what="p = 0.5")


@pytest.mark.parametrize("H,W", [(512, 512), (520, 520)])
def test_numbering_scan_spans_many_chunks(H, W):
    got = _check(O.bernoulli((1, H, W), 0.41, H), 8, max_objects=32, what=f"{H}x{W}")
    assert int(got["count"][0]) > 1024


# ---- batches, views ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
def test_batch_isolation(connectivity):
    H, W = 40, 70
    m = np.zeros((2, H, W), np.uint8)
    m[0, H - 1] = 1
    m[1, 0] = 1
    got = _check(m, connectivity, max_objects=2, what="two rows")
    assert got["count"].tolist() == [1, 1] and got["bbox"][:, 0].tolist() == [[H - 1, 0, H, W], [0, 0, 1, W]]
    masks = torch.from_numpy(BERNOULLI[connectivity]).to(DEV)
    whole = label_components(masks, connectivity=connectivity, max_objects=16, min_area=2)
    for n in range(masks.shape[0]):
        alone = label_components(masks[n:n + 1], connectivity=connectivity, max_objects=16, min_area=2)
        for k in whole:
            assert torch.equal(whole[k][n:n + 1], alone[k]), (n, k)
        flat = label_components(masks[n], connectivity=connectivity, max_objects=16, min_area=2)
        for k in whole:
            assert torch.equal(whole[k][n], flat[k]), (n, k)


def test_bool_uint8_and_strided_views():
    rng = np.random.default_rng(3)
    m = (rng.random((2, 70, 90)) < 0.45)
    ref = O.batch(m.astype(np.uint8), 8, 1, 8)
    _same(label_components(torch.from_numpy(m).to(DEV), max_objects=8), ref, "bool")
    u8 = torch.from_numpy(m.astype(np.uint8) * rng.integers(1, 256, size=m.shape).astype(np.uint8)).to(DEV)
    _same(label_components(u8, max_objects=8), ref, "uint8, any nonzero value")
    big = torch.ones((2, 77, 101), dtype=torch.uint8, device=DEV)            # foreground all round the crop
    crop = big[:, 4:74, 5:95]
    crop.copy_(torch.from_numpy(m))
    assert not crop.is_contiguous()
    _same(label_components(crop, max_objects=8), ref, "row-strided crop")
    _same(label_components(crop.bool()[:, :, :], max_objects=8), ref, "bool copy of the crop")
    cols = torch.from_numpy(m).to(DEV).transpose(1, 2)                       # columns not contiguous: copied
    _same(label_components(cols, max_objects=8), O.batch(m.transpose(0, 2, 1).astype(np.uint8), 8, 1, 8), "transposed")


# ---- the filter and the table -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("min_area", [2, 8, 64])
def test_min_area_filters_then_renumbers(connectivity, min_area):
    got = _check(BERNOULLI[connectivity], connectivity, min_area=min_area, max_objects=32, what="filter")
    assert (got["count"] > 0).all()
    labels, kept = got["labels"], got["kept_pixels"]
    assert torch.equal((labels > 0).sum((1, 2)), kept)


def test_min_area_larger_than_every_object():
    masks = BERNOULLI[8]
    got = _check(masks, 8, min_area=150 * 200 + 1, max_objects=4, what="nothing kept")
    for k in ("labels", "count", "kept_pixels", "largest", "size_hist", "area", "bbox", "centroid"):
        assert int(got[k].abs().max()) == 0, k


def test_table_above_equal_and_below_the_count():
    masks = BERNOULLI[8][:1]
    n = int(O.batch(masks, 8)["count"][0])
    full = _check(masks, 8, max_objects=n + 5, what="table above")
    assert int(full["area"][0, n - 1]) > 0 and int(full["area"][0, n:].abs().max()) == 0
    _check(masks, 8, max_objects=n, what="table equal")
    cut = _check(masks, 8, max_objects=7, what="table below")
    assert int(cut["count"][0]) == n and torch.equal(cut["labels"], full["labels"])
    for k in TABLE:
        assert torch.equal(cut[k], full[k][:, :7]), k
    none = label_components(torch.from_numpy(masks).to(DEV))
    assert sorted(none) == ["count", "kept_pixels", "labels", "largest", "size_hist"]


# ---- state ------------------------------------------------------------------------------------------------------------
def test_stale_workspace_and_determinism(poison, monkeypatch):
    from stain2stain_amd import ops
    big, small = O.bernoulli((1, 512, 512), 0.41, 5), O.bernoulli((1, 97, 131), 0.45, 6)
    _check(big, 8, max_objects=16, what="big")
    # from here on the workspace keeps what the big call left in it (no poison between the calls)
    monkeypatch.setattr(ops, "_workspace", poison)
    first = _check(small, 8, max_objects=16, what="small after big")
    again = label_components(torch.from_numpy(small).to(DEV), max_objects=16)
    for k in first:
        assert torch.equal(first[k], again[k]), k
    for conn in (4, 8):
        a = label_components(torch.from_numpy(BERNOULLI[conn]).to(DEV), connectivity=conn, min_area=3, max_objects=40)
        b = label_components(torch.from_numpy(BERNOULLI[conn]).to(DEV), connectivity=conn, min_area=3, max_objects=40)
        for k in a:
            assert torch.equal(a[k], b[k]), (conn, k)


# ---- stained tiles ----------------------------------------------------------------------------------------------------
def _plaques(B, H, W, seed, discs=14):
    """uint8 [B, H, W, 3]: haematoxylin background, DAB discs of mixed sizes, speckle, glass patches and noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    conc = np.zeros((B, H, W, 3))
    conc[..., 0] = rng.uniform(0.05, 0.5, size=(B, H, W))
    conc[..., 1] = np.where(rng.random((B, H, W)) < 0.03, rng.uniform(0.3, 1.0, size=(B, H, W)), 0.02)
    for n in range(B):
        for _ in range(discs):
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1.5, 9.0)
            conc[n, ..., 1][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.uniform(0.5, 1.2)
    img = R.synthesise(conc, "hdab").astype(np.int32) + rng.integers(-3, 4, size=(B, H, W, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    glass = rng.random((B, H // 8 + 1, W // 8 + 1)) < 0.15
    glass = np.repeat(np.repeat(glass, 8, 1), 8, 2)[:, :H, :W]
    img[glass] = rng.integers(225, 256, size=(int(glass.sum()), 3), dtype=np.uint8)
    return img


def _network(u8, seed):
    """uint8 [B, H, W, 3] -> fp32 [B, 3, H, W] in the network's range with a sub-level jitter."""
    rng = np.random.default_rng(seed)
    lv = u8.astype(np.float64).transpose(0, 3, 1, 2) + rng.random(u8.transpose(0, 3, 1, 2).shape) * 0.98
    return np.ascontiguousarray((lv / 127.5 - 1.0).astype(np.float32))


def _stain_ref(u8, stain, connectivity, min_area, max_objects, mpp=None, white=220, black=0):
    """What stain_objects returns for uint8 [B, H, W, 3], from the two restatements."""
    m32 = unmix_matrix("hdab").numpy()
    pos = R.positive32(u8, m32, THR, white, black)[..., stain].astype(np.uint8)
    c = O.batch(pos, connectivity, min_area, max_objects)
    tissue = R.tissue(u8, white, black).sum(axis=(1, 2)).astype(np.int64)
    ref = {"count": c["count"], "tissue": tissue, "positive": c["kept_pixels"], "largest": c["largest"],
           "size_hist": c["size_hist"], "labels": c["labels"],
           "burden": (c["kept_pixels"].astype(np.float64) / np.maximum(tissue, 1).astype(np.float64)).astype(np.float32)}
    if max_objects is not None:
        ref.update({k: c[k] for k in TABLE})
    if mpp is not None:
        mm2 = tissue.astype(np.float64) * (mpp * mpp * 1e-6)
        ref["per_mm2"] = np.where(tissue > 0, c["count"].astype(np.float64) / np.where(tissue > 0, mm2, 1.0), 0.0)
    return ref


STAIN_DTYPES = dict(DTYPES, tissue=np.int64, positive=np.int64, burden=np.float32, per_mm2=np.float64)
TILES = _plaques(2, 96, 160, 17)


def _same_stain(got, ref, what):
    got = _np(got)
    assert sorted(got) == sorted(ref), (what, sorted(got), sorted(ref))
    for k, want in ref.items():
        assert got[k].dtype == STAIN_DTYPES[k] and got[k].shape == np.asarray(want).shape, (what, k)
        assert np.array_equal(got[k], want), (what, k)


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_stain_objects(kind):
    if kind == "u8":
        inp, u8 = torch.from_numpy(TILES).to(DEV), TILES
    else:
        x = _network(TILES, 23)
        inp, u8 = torch.from_numpy(x).to(DEV), R.nchw_to_u8(x)
    q = stain_quantify(inp, thresholds=THR)
    for stain, conn in ((1, 8), (0, 4)):
        got = stain_objects(inp, stain=stain, thresholds=THR, connectivity=conn, max_objects=24, mpp=0.5,
                            return_labels=True)
        _same_stain(got, _stain_ref(u8, stain, conn, 1, 24, mpp=0.5), f"{kind} stain {stain}")
        assert torch.equal(got["positive"], q["positive"][:, stain]) and torch.equal(got["tissue"], q["tissue"])
        assert torch.equal(got["burden"], q["burden"][:, stain])
    assert (stain_objects(inp, thresholds=THR)["count"] > 5).all()
    got = stain_objects(inp, thresholds=THR, min_area=12, white=256, black=30, mpp=0.2528)
    ref = _stain_ref(u8, 1, 8, 12, None, mpp=0.2528, white=256, black=30)
    del ref["labels"]
    _same_stain(got, ref, f"{kind} filtered")
    assert (got["count"] > 0).all() and (got["positive"] < q["positive"][:, 1]).all()


def test_stain_objects_crop_view_and_no_tissue():
    B, H, W, _ = TILES.shape
    big = torch.full((B, H + 5, W + 6, 3), 77, dtype=torch.uint8, device=DEV)
    view = big[:, 2:2 + H, 3:3 + W]
    view.copy_(torch.from_numpy(TILES))
    ref = _stain_ref(TILES, 1, 8, 1, None)
    _same_stain(stain_objects(view, thresholds=THR, return_labels=True), ref, "crop view")
    glass = torch.full((1, 33, 47, 3), 255, dtype=torch.uint8, device=DEV)
    got = stain_objects(glass, mpp=0.5, max_objects=2)
    for k, v in got.items():
        assert float(v.double().abs().max()) == 0.0, k


def test_stain_object_agreement():
    m32 = unmix_matrix("hdab").numpy()
    target = TILES
    pred = np.roll(TILES, (3, -5), axis=(1, 2)).copy()                         # the same plaques, shifted
    pred[:, :40, :60] = R.synthesise([0.3, 0.0, 0.0], "hdab")                  # and some of them missed
    for min_area, conn in ((1, 8), (6, 4)):
        got = _np(stain_object_agreement(torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV), thresholds=THR,
                                         connectivity=conn, min_area=min_area))
        pa = R.positive32(pred, m32, THR)[..., 1]
        pb = R.positive32(target, m32, THR)[..., 1]
        for n in range(pred.shape[0]):
            la, na, _ = O.label(pa[n], conn, min_area)
            lb, nb, _ = O.label(pb[n], conn, min_area)
            ref = O.agreement(la, na, lb, nb)
            assert sorted(got) == sorted(ref)
            for k, want in ref.items():
                assert got[k].dtype == want.dtype and got[k][n] == want, (min_area, n, k, got[k][n], want)
            print(f"min_area {min_area} sample {n}: " + ", ".join(f"{k} {got[k][n]}" for k in ref))
        assert (got["recall"] < 1).all() and (got["recall"] > 0).all()
    same = _np(stain_object_agreement(torch.from_numpy(target).to(DEV), torch.from_numpy(target).to(DEV), thresholds=THR))
    assert (same["recall"] == 1).all() and (same["precision"] == 1).all() and (same["f1"] == 1).all()
    assert (same["count_abs_err"] == 0).all()


def test_stain_object_agreement_empty_conventions():
    blank = np.broadcast_to(R.synthesise([0.3, 0.0, 0.0], "hdab"), (1, 40, 50, 3)).copy()
    brown = blank.copy()
    brown[0, 10:20, 10:20] = R.synthesise([0.1, 1.0, 0.0], "hdab")
    a = torch.from_numpy(np.concatenate([blank, blank, brown, brown])).to(DEV)
    b = torch.from_numpy(np.concatenate([blank, brown, blank, brown])).to(DEV)
    got = _np(stain_object_agreement(a, b))
    assert got["count_pred"].tolist() == [0, 0, 1, 1] and got["count_target"].tolist() == [0, 1, 0, 1]
    assert got["count_abs_err"].tolist() == [0, 1, 1, 0]
    assert got["recall"].tolist() == [1, 0, 0, 1] and got["precision"].tolist() == [1, 0, 0, 1]
    assert got["f1"].tolist() == [1, 0, 0, 1]


# ---- whole regions ----------------------------------------------------------------------------------------------------
def test_region_stain_objects_bands_host_and_gpu():
    H, W = 300, 517
    region = _plaques(1, H, W, 29, discs=60)[0]
    region[40:56, 100:130] = R.synthesise([0.1, 1.0, 0.0], "hdab")            # spans the seams at rows 48 (and 16 k)
    ref = _stain_ref(region[None], 1, 8, 4, 48, mpp=0.5)
    ref = {k: v[0] for k, v in ref.items()}
    seam = ref["labels"][40:56, 100:130]
    assert seam.min() > 0 and (seam == seam[0, 0]).all()
    host = torch.from_numpy(region)
    padded = torch.zeros((H, W + 3, 3), dtype=torch.uint8, device=DEV)
    view = padded[:, 1:1 + W]
    view.copy_(host)
    for band_rows in (None, 16, 48):
        for src, name in ((host, "host"), (host.to(DEV), "gpu"), (view, "gpu view")):
            got = region_stain_objects(src, band_rows=band_rows, thresholds=THR, min_area=4, max_objects=48, mpp=0.5,
                                       return_labels=True)
            assert all(v.is_cuda for v in got.values())
            _same_stain(got, ref, f"{name} band_rows {band_rows}")
    small = region_stain_objects(host.to(DEV), thresholds=THR)
    assert sorted(small) == ["burden", "count", "largest", "positive", "size_hist", "tissue"] and small["count"].dim() == 0


# ---- no hidden synchronisation ----------------------------------------------------------------------------------------
def test_stain_objects_does_not_synchronise():
    inp = torch.from_numpy(TILES).to(DEV)
    pair = inp.flip(1).contiguous()
    mask = torch.from_numpy(BERNOULLI[8]).to(DEV)
    stain_objects(inp, thresholds=THR, max_objects=8, mpp=0.5)                 # the workspace exists from here on
    stain_object_agreement(inp, pair, thresholds=THR)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = stain_objects(inp, thresholds=THR, max_objects=8, mpp=0.5, return_labels=True)
        b = stain_object_agreement(inp, pair, thresholds=THR)
        c = label_components(mask, min_area=2, max_objects=8)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert int(a["count"].sum()) > 0 and float(b["f1"].sum()) >= 0 and int(c["count"].sum()) > 0
