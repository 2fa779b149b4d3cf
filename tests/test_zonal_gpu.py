"""The zonal kernels (csrc/zonal.hip) against the numpy / Python-integer restatement of tests/zonal_ref.py, on poisoned
memory (every ``torch.empty`` and every ``ops._workspace`` slab starts as NaN / 0xFF, as in
tests/test_stain_calibrate_gpu.py).

Tolerances.  Tables, unzoned counts, overlaps, zones and bands are integers; the derived values are
doubles formed from those integers by the operations the header spells out, which the restatement repeats: everything is
compared for equality.  The one exception is the cross-check of the paired Dice / IoU at Z = 1 against the fp32 values of
``stain_agreement``: one fp32 rounding of the same quotient, 2^-23 relative (the bound of 3.17 and 3.33)."""
import numpy as np
import pytest
import torch

import stain_quant_ref as R
import zonal_ref as Zr
from stain2stain_amd import (distance_zones, label_components, object_zones, region_stain_zonal,
                             region_stain_zonal_agreement, stain_agreement, stain_objects, stain_quantify, stain_zonal,
                             stain_zonal_agreement, stain_zonal_objects)
from stain2stain_amd.stain_quant import unmix_matrix

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = 2.0 ** -23
THR = (0.2, 0.2, 0.2)


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
        yield
    finally:
        torch.use_deterministic_algorithms(prev_det, warn_only=prev_warn)
        tud.fill_uninitialized_memory = prev_fill


def _stained(B, H, W, seed, plaque=0.08):
    """uint8 [B, H, W, 3]: haematoxylin background with DAB blobs, glass patches, black specks and noise."""
    rng = np.random.default_rng(seed)
    conc = np.zeros((B, H, W, 3))
    conc[..., 0] = rng.uniform(0.05, 0.5, size=(B, H, W))
    conc[..., 1] = np.where(rng.random((B, H, W)) < plaque, rng.uniform(0.1, 1.2, size=(B, H, W)), 0.02)
    img = R.synthesise(conc, "hdab").astype(np.int32) + rng.integers(-3, 4, size=(B, H, W, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    glass = rng.random((B, H, W)) < 0.2
    img[glass] = rng.integers(225, 256, size=(int(glass.sum()), 3), dtype=np.uint8)
    img[rng.random((B, H, W)) < 0.01] = 0
    return img


def _pair(B, H, W, seed):
    a, b = _stained(B, H, W, seed), _stained(B, H, W, seed + 1000, plaque=0.12)
    b[:, : H // 2] = a[:, : H // 2]                                        # the masks overlap
    return a, b


def _network(u8, seed):
    """uint8 [B, H, W, 3] -> fp32 [B, 3, H, W] in the network's range with a sub-level jitter (the quantiser has work)."""
    rng = np.random.default_rng(seed)
    lv = u8.astype(np.float64).transpose(0, 3, 1, 2) + rng.random(u8.transpose(0, 3, 1, 2).shape) * 0.98
    return np.ascontiguousarray((lv / 127.5 - 1.0).astype(np.float32))


def _crop_view(arr, fill=77):
    """[B, H, W(, 3)] as a crop view of a larger GPU array: odd row pitch, unaligned base."""
    B, H, W = arr.shape[:3]
    big = torch.full((B, H + 5, W + 6) + arr.shape[3:], fill, dtype=torch.uint8, device=DEV)
    view = big[:, 2:2 + H, 3:3 + W]
    view.copy_(torch.from_numpy(arr))
    return view


def _m32(stains="hdab"):
    return unmix_matrix(stains).numpy()


def _same(got, want, what):
    """Equality of a device tensor and the restatement's array, dtype included."""
    got, want = got.cpu().numpy(), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), what


def _no_nan(d):
    for k, v in d.items():
        if isinstance(v, torch.Tensor) and v.is_floating_point():
            assert not torch.isnan(v).any(), k


def _check_single(z, tab, unz, what):
    _same(z["counts"], tab, what + " counts")
    _same(z["unzoned"], unz, what + " unzoned")
    for k, v in Zr.derived(tab, unz).items():
        _same(z[k], v, f"{what} {k}")
    assert torch.equal(z["pixels"], z["counts"][..., 0]) and torch.equal(z["sum_q"], z["counts"][..., 5:8])
    assert torch.equal(z["tissue"], z["counts"][..., 1]) and torch.equal(z["positive"], z["counts"][..., 2:5])
    _no_nan(z)


def _check_paired(z, tab, unz, what):
    _same(z["counts"], tab, what + " counts")
    _same(z["unzoned"], unz, what + " unzoned")
    for k, v in Zr.pair_derived(tab).items():
        _same(z[k], v, f"{what} {k}")
    _no_nan(z)


def _patterns(B, H, W, seed):
    """(name, zone bytes [B, H, W], Z)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    full = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B, H, W)).astype(np.uint8))
    mixed = rng.integers(0, 8, size=(B, H, W)).astype(np.uint8)
    mixed[rng.random((B, H, W)) < 0.05] = 255
    areas = full((xx // 32 + 2 * (yy // 16)) % 7)                          # large areas, bytes 5 and 6 are no zone
    return [("constant", full(np.full((H, W), 3)), 5),                     # the aggregated path
            ("columns", full(xx % 5), 5),                                  # every lane differs inside its quad
            ("blocks32", full((xx // 32 + yy // 32) % 3), 3),              # waves split in two, lanes uniform
            ("random256", rng.integers(0, 256, size=(B, H, W)).astype(np.uint8), 256),
            ("one", full(np.zeros((H, W))), 1),
            ("one of 256", full(np.full((H, W), 255)), 256),
            ("unzoned mixed", mixed, 5),
            ("unzoned areas", areas, 5),
            ("all unzoned", full(np.full((H, W), 200)), 5)]


CASES = [("u8", 1, 1, 1, False), ("u8", 2, 37, 53, True), ("u8", 2, 64, 64, False), ("u8", 2, 130, 1030, False),
         ("f32", 2, 37, 53, False), ("f32", 2, 64, 64, True)]


def _inputs(kind, B, H, W, crop, seed):
    """(GPU pair, the uint8 bytes the kernels see)."""
    a, b = _pair(B, H, W, seed)
    if kind == "f32":
        xa, xb = _network(a, 1), _network(b, 2)
        xa.reshape(-1)[:: 7] += 3.0                                        # out of range: the clamp has work
        xb.reshape(-1)[:: 11] -= 3.0
        return (torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV)), (R.nchw_to_u8(xa), R.nchw_to_u8(xb))
    if crop:
        return (_crop_view(a), _crop_view(b)), (a, b)
    return (torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)), (a, b)


# ---- 1. parity with the restatement: every shape, every zone pattern ---------------------------------------------------
@pytest.mark.parametrize("kind,B,H,W,crop", CASES)
def test_parity(kind, B, H, W, crop):
    m32 = _m32()
    (ga, gb), (a, b) = _inputs(kind, B, H, W, crop, 100 + H)
    cols, pcols = Zr.columns(a, m32, THR), Zr.pair_columns(a, b, m32, THR, stain=1)
    for name, zones, Z in _patterns(B, H, W, 7 + H):
        what = f"{kind} {B}x{H}x{W} {name}"
        gz = _crop_view(zones, 9) if crop else torch.from_numpy(zones).to(DEV)
        if crop and kind == "u8":
            assert gz.stride(1) % 4 != 0 and gz.data_ptr() % 4 != 0 and ga.stride(1) % 4 != 0
        tab, unz = Zr.tabulate(cols, zones, Z)
        z = stain_zonal(ga, gz, Z)
        _check_single(z, tab, unz, what)
        assert z["num_zones"] == Z and tuple(z["burden"].shape) == (B, Z, 3) and tuple(z["area_frac"].shape) == (B, Z)
        ptab, punz = Zr.tabulate(pcols, zones, Z)
        _check_paired(stain_zonal_agreement(ga, gb, gz, Z), ptab, punz, what + " paired")
        if name == "all unzoned":
            assert (z["counts"] == 0).all() and (z["unzoned"] == H * W).all() and (z["area_frac"] == 0).all()
        if name == "unzoned mixed":
            assert int(z["unzoned"].sum()) > 0 or H * W == 1
            tp, up = Zr.tabulate(cols, zones, Z, pool=True)
            _check_single(stain_zonal(ga, gz, Z, pool=True), tp, up, what + " pooled")
            tp, up = Zr.tabulate(pcols, zones, Z, pool=True)
            _check_paired(stain_zonal_agreement(ga, gb, gz, Z, pool=True), tp, up, what + " paired pooled")
    # a bool map is a byte map of zeros and ones; stain 0 of the pair
    zb = np.random.default_rng(3).random((B, H, W)) < 0.5
    tab, unz = Zr.tabulate(cols, zb.astype(np.uint8), 2)
    _check_single(stain_zonal(ga, torch.from_numpy(zb).to(DEV), 2), tab, unz, "bool map")
    ptab, punz = Zr.pair_table(a, b, zb.astype(np.uint8), 1, m32, THR, stain=0)
    _check_paired(stain_zonal_agreement(ga, gb, torch.from_numpy(zb).to(DEV), 1, stain=0), ptab, punz, "stain 0, Z 1")


# ---- 2. invariants against the existing kernels -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_zones_add_up_to_stain_quantify_and_agreement(kind):
    B, H, W = 3, 64, 80
    (ga, gb), _ = _inputs(kind, B, H, W, False, 31)
    q = stain_quantify(ga)
    for name, zones, Z in _patterns(B, H, W, 5):
        if name.startswith("unzoned") or name == "all unzoned":
            continue
        z = stain_zonal(ga, torch.from_numpy(zones).to(DEV), Z)
        assert torch.equal(z["tissue"].sum(1), q["tissue"]) and torch.equal(z["positive"].sum(1), q["positive"]), name
        assert (z["pixels"].sum(1) == H * W).all() and (z["unzoned"] == 0).all(), name
    one = torch.zeros((B, H, W), dtype=torch.uint8, device=DEV)
    z = stain_zonal(ga, one, 1)
    assert torch.equal(z["tissue"][:, 0], q["tissue"]) and torch.equal(z["positive"][:, 0], q["positive"])
    assert torch.equal(z["burden"][:, 0].float(), q["burden"])             # the same quotient, rounded to fp32 once
    assert (z["area_frac"] == 1).all()
    zp = stain_zonal_agreement(ga, gb, one, 1)
    ag = stain_agreement(ga, gb, stain=1)
    for k in ("dice", "iou"):
        want, got = zp[k][:, 0].cpu().numpy(), ag[k].cpu().numpy().astype(np.float64)
        err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
        err = np.where(want == 0, np.abs(got), err)
        print(f"{kind} {k}: max rel err {err.max():.3e} (tolerance {F32:.1e})")
        assert (err <= F32).all(), k


# ---- 3. batch independence, repeatability, accumulation, other arguments ------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_a_sample_does_not_see_its_batch_mates_runs_repeat_and_out_accumulates(kind):
    B, H, W, Z = 4, 64, 80, 5
    (ga, gb), (a, b) = _inputs(kind, B, H, W, False, 41)
    zones = dict((n, z) for n, z, _ in _patterns(B, H, W, 9))["unzoned mixed"]
    gz = torch.from_numpy(zones).to(DEV)
    keys = ("counts", "unzoned", "derived")
    z1, z2 = stain_zonal(ga, gz, Z), stain_zonal(ga, gz, Z)
    p1, p2 = stain_zonal_agreement(ga, gb, gz, Z), stain_zonal_agreement(ga, gb, gz, Z)
    assert all(torch.equal(z1[k], z2[k]) for k in keys) and all(torch.equal(p1[k], p2[k]) for k in keys)
    for n in (0, 3):
        zs = stain_zonal(ga[n:n + 1], gz[n:n + 1], Z)
        ps = stain_zonal_agreement(ga[n:n + 1], gb[n:n + 1], gz[n:n + 1], Z)
        assert all(torch.equal(zs[k][0], z1[k][n]) for k in keys), n
        assert all(torch.equal(ps[k][0], p1[k][n]) for k in keys), n
    # a dataset-level table: two half-batches added into one result equal the pooled whole
    whole = stain_zonal(ga, gz, Z, pool=True)
    acc = stain_zonal(ga[:2], gz[:2], Z, pool=True)
    assert stain_zonal(ga[2:], gz[2:], Z, pool=True, out=acc) is acc
    assert all(torch.equal(acc[k], whole[k]) for k in keys) and torch.equal(acc["burden"], whole["burden"])
    assert torch.equal(whole["counts"][0], z1["counts"].sum(0)) and int(whole["unzoned"][0]) == int(z1["unzoned"].sum())
    pw = stain_zonal_agreement(ga, gb, gz, Z, pool=True)
    pacc = stain_zonal_agreement(ga[:2], gb[:2], gz[:2], Z, pool=True)
    stain_zonal_agreement(ga[2:], gb[2:], gz[2:], Z, pool=True, out=pacc)
    assert all(torch.equal(pacc[k], pw[k]) for k in keys) and torch.equal(pacc["dice"], pw["dice"])
    with pytest.raises(ValueError):
        stain_zonal(ga, gz, Z, out=acc)                                    # four owners into one
    with pytest.raises(ValueError):
        stain_zonal(ga[:2], gz[:2], 4, pool=True, out=acc)                 # another number of zones
    with pytest.raises(ValueError):
        stain_zonal_agreement(ga[2:], gb[2:], gz[2:], Z, stain=0, pool=True, out=pacc)      # another stain
    with pytest.raises(TypeError):
        stain_zonal(ga[:2], gz[:2], Z, pool=True, out=pacc["counts"])
    # other tissue thresholds, other concentration thresholds, the other basis
    thr = (0.1, 0.35, 0.05)
    tab, unz = Zr.table(a, zones, Z, _m32(), thr, 256, 40)
    _check_single(stain_zonal(ga, gz, Z, thresholds=thr, white=256, black=40), tab, unz, "white 256 black 40")
    tab, unz = Zr.pair_table(a, b, zones, Z, _m32(), thr, 2, 200, 1)
    _check_paired(stain_zonal_agreement(ga, gb, gz, Z, stain=2, thresholds=thr, white=200, black=1), tab, unz, "pair 200 1")
    tab, unz = Zr.table(a, zones, Z, _m32("hed"), THR)
    _check_single(stain_zonal(ga, gz, Z, stains="hed"), tab, unz, "hed")
    tab, unz = Zr.pair_table(a, b, zones, Z, _m32("hed"), THR, 2)
    _check_paired(stain_zonal_agreement(ga, gb, gz, Z, stain=2, stains="hed"), tab, unz, "hed pair")


# ---- 4. regions -------------------------------------------------------------------------------------------------------
def test_regions_for_host_and_gpu_input_and_every_banding():
    H, W, Z = 301, 203, 6
    a, b = _pair(1, H, W, 51)
    m32 = _m32()
    yy, xx = np.mgrid[0:H, 0:W]
    zones = ((xx // 40 + yy // 25) % 8).astype(np.uint8)                   # bytes 6 and 7 are no zone
    zones[np.random.default_rng(2).random((H, W)) < 0.1] = 255
    ha, hb, hz = torch.from_numpy(a[0]), torch.from_numpy(b[0]), torch.from_numpy(zones)
    ga, gz = _crop_view(a)[0], _crop_view(zones[None], 9)[0]               # crop views: odd pitch, unaligned base
    gb = hb.to(DEV)
    keys = ("counts", "unzoned", "derived")
    base = stain_zonal(ga[None], gz[None], Z)
    _check_single(base, *Zr.table(a, zones[None], Z, m32, THR), "region bytes")
    pbase = stain_zonal_agreement(ga[None], gb[None], gz[None], Z)
    _check_paired(pbase, *Zr.pair_table(a, b, zones[None], Z, m32, THR), "region pair bytes")
    for img, zn in ((ga, gz), (ha, hz), (ga, hz), (ha, gz)):
        for band_rows in (16, 48, None):
            got = region_stain_zonal(img, zn, Z, band_rows=band_rows)
            assert all(torch.equal(got[k], base[k]) for k in keys), (img.is_cuda, zn.is_cuda, band_rows)
            if band_rows is not None:
                assert region_stain_zonal.last_stats["bands"] == -(-H // band_rows)
    for pa, pb, zn in ((ga, gb, gz), (ha, hb, hz), (ga, hb, hz), (ha, gb, gz)):
        for band_rows in (16, 48, None):
            got = region_stain_zonal_agreement(pa, pb, zn, Z, band_rows=band_rows)
            assert all(torch.equal(got[k], pbase[k]) for k in keys), (pa.is_cuda, pb.is_cuda, zn.is_cuda, band_rows)
    assert torch.equal(region_stain_zonal(ha, hz, Z, band_rows=1)["counts"], base["counts"])
    two = region_stain_zonal(ha, hz, Z, out=region_stain_zonal(ga, gz, Z))            # two regions of one slide
    assert torch.equal(two["counts"], 2 * base["counts"]) and torch.equal(two["unzoned"], 2 * base["unzoned"])
    assert torch.equal(two["burden"], base["burden"]) and torch.equal(two["area_frac"], base["area_frac"])


# ---- 5. objects by zone -----------------------------------------------------------------------------------------------
OBJECT_KEYS = ("zone", "zone_pixels", "area", "count", "objects", "object_pixels", "overlap")


def _check_objects(labels, zones, Z, M, what):
    got = object_zones(labels, torch.from_numpy(zones).to(DEV), Z, max_objects=M, return_overlap=True)
    ref = Zr.object_zones(labels.cpu().numpy(), zones, Z, M)
    assert sorted(got) == sorted(OBJECT_KEYS)
    for k in OBJECT_KEYS:
        _same(got[k], ref[k], f"{what} {k}")
    return got


def _designed():
    """Three samples of 40 x 64: designed objects; four objects in a corner; background only."""
    mask = np.zeros((3, 40, 64), bool)
    mask[0, 4:8, 10:16] = True          # object 1: 24 pixels, split 12 / 12 by the zone border at column 13
    mask[0, 12:15, 30:33] = True        # object 2: wholly without a zone
    mask[0, 20:26, 2:7] = True          # object 3: 30 pixels, 12 of them without a zone (byte 200), 18 in zone 1
    mask[0, 30:32, 40:50] = True        # object 4: zones 2 (6 pixels) and 3 (14 pixels)
    mask[0, 36:38, 60:64] = True        # object 5: at the image corner, zone 3
    mask[1, 0:2, 0:2] = mask[1, 0:2, 4:6] = mask[1, 4:6, 0:2] = mask[1, 4:6, 4:6] = True
    zones = np.zeros((3, 40, 64), np.uint8)
    zones[:, :, 13:] = 1
    zones[:, 10:18, 28:36] = 255
    zones[:, 20:26, 2:4] = 200
    zones[:, 20:26, 4:7] = 1
    zones[:, 28:, 43:] = 3
    zones[:, 28:, 36:43] = 2
    return mask, zones


def test_object_zones_on_designed_masks():
    mask, zones = _designed()
    lab = label_components(torch.from_numpy(mask).to(DEV))
    labels = lab["labels"]
    assert lab["count"].tolist() == [5, 4, 0]
    got = _check_objects(labels, zones, 4, 8, "designed")
    assert got["zone"][0].tolist() == [0, -1, 1, 3, 3, -1, -1, -1] and (got["zone"][2] == -1).all()
    assert got["zone_pixels"][0].tolist() == [12, 0, 18, 14, 8, 0, 0, 0]
    assert got["objects"][0].tolist() == [1, 1, 0, 2] and got["object_pixels"][0].tolist() == [24, 30, 0, 28]
    assert got["objects"][2].tolist() == [0, 0, 0, 0] and got["count"].tolist() == [5, 4, 0]
    _check_objects(labels, zones, 4, 3, "count > max_objects")
    one = _check_objects(labels, zones, 4, 1, "M = 1")
    assert one["zone"][:, 0].tolist() == [0, 0, -1] and one["count"].tolist() == [5, 4, 0]
    z1 = _check_objects(labels, np.minimum(zones, 1) * 255, 1, 8, "Z = 1")             # zone 0 left of column 13 only
    assert z1["zone"][0].tolist() == [0, -1, -1, -1, -1, -1, -1, -1]
    _check_objects(labels, zones, 256, 8, "Z = 256: 200 and 255 are zones")
    z256 = _check_objects(labels, zones, 255, 8, "Z = 255")
    assert z256["zone"][0].tolist() == [0, -1, 1, 3, 3, -1, -1, -1]
    # a single label image without a batch dimension, a strided zone view
    solo = object_zones(labels[0], _crop_view(zones, 9)[0], 4, max_objects=8)
    assert solo["zone"].tolist() == got["zone"][0].tolist() and tuple(solo["objects"].shape) == (4,)


def test_object_zones_on_many_small_objects():
    rng = np.random.default_rng(11)
    B, H, W = 2, 256, 256
    mask = np.zeros((B, H, W), bool)
    for n in range(B):
        for gy in range(0, H, 14):
            for gx in range(0, W, 14):
                if rng.random() < 0.93:
                    y, x = gy + rng.integers(0, 8), gx + rng.integers(0, 8)
                    mask[n, y:y + rng.integers(1, 6), x:x + rng.integers(1, 6)] = True
    yy, xx = np.mgrid[0:H, 0:W]
    zones = np.broadcast_to(((xx // 20) * 3 + yy // 50) % 12, (B, H, W)).astype(np.uint8).copy()
    zones[rng.random((B, H, W)) < 0.2] = 255
    lab = label_components(torch.from_numpy(mask).to(DEV))
    counts = lab["count"].tolist()
    print("objects per sample:", counts)
    assert all(250 <= c <= 400 for c in counts)
    got = _check_objects(lab["labels"], zones, 10, 512, "many")                         # bytes 10, 11 and 255: no zone
    assert int(got["objects"].sum()) + int((got["zone"] == -1).sum()) == 2 * 512
    _check_objects(lab["labels"], zones, 12, 256, "many, M below count")
    again = object_zones(lab["labels"], torch.from_numpy(zones).to(DEV), 10, max_objects=512)
    assert all(torch.equal(again[k], got[k]) for k in again)


def test_stain_zonal_objects():
    B, H, W, Z, M = 2, 96, 96, 4, 2048
    img = _stained(B, H, W, 71)
    yy, xx = np.mgrid[0:H, 0:W]
    zones = np.broadcast_to(xx // 24, (B, H, W)).astype(np.uint8).copy()
    zones[:, :20] = 255                                                    # objects up here have no zone
    g, gz = torch.from_numpy(img).to(DEV), torch.from_numpy(zones).to(DEV)
    mpp = 0.5
    s = stain_zonal_objects(g, gz, Z, min_area=2, max_objects=M, mpp=mpp)
    so = stain_objects(g, min_area=2, return_labels=True)
    z = stain_zonal(g, gz, Z)
    assert all(torch.equal(s[k], z[k]) for k in ("counts", "unzoned", "derived", "burden", "area_frac"))
    assert torch.equal(s["count"], so["count"]) and int(so["count"].max()) <= M and int(so["count"].min()) > 20
    ref = Zr.object_zones(so["labels"].cpu().numpy(), zones, Z, M)
    for k in ("objects", "object_pixels", "zone", "zone_pixels"):
        _same(s[k], ref[k], k)
    rows = torch.arange(M, device=DEV)[None] < so["count"][:, None]
    nowhere = ((s["zone"] == -1) & rows).sum(1)
    assert int(nowhere.min()) > 0
    assert torch.equal(s["objects"].sum(1) + nowhere, so["count"].long())
    _same(s["per_mm2"], Zr.per_mm2(ref["objects"], z["tissue"].cpu().numpy(), mpp), "per_mm2")
    glass = torch.full((1, 32, 32, 3), 255, dtype=torch.uint8, device=DEV)
    e = stain_zonal_objects(glass, torch.zeros((1, 32, 32), dtype=torch.uint8, device=DEV), 2, mpp=mpp)
    assert (e["per_mm2"] == 0).all() and (e["objects"] == 0).all() and (e["zone"] == -1).all() and "per_mm2" not in z
    _no_nan(e)


# ---- 6. distance bands ------------------------------------------------------------------------------------------------
def _shapes(H, W):
    """[4, H, W] bool: a disc, an L-shape, an empty and a full mask."""
    yy, xx = np.mgrid[0:H, 0:W]
    disc = (yy - H // 2) ** 2 + (xx - W // 3) ** 2 <= (min(H, W) // 3) ** 2
    ell = np.zeros((H, W), bool)
    ell[3:H - 4, 5:5 + W // 4] = True
    ell[H - 4 - H // 4:H - 4, 5:W - 6] = True
    return np.stack([disc, ell, np.zeros((H, W), bool), np.ones((H, W), bool)])


EDGES = {"n = 1, fractional": [2.5], "four": [0, 1, 2.5, 7.3], "n = 126": [0.37 * i for i in range(1, 127)]}


@pytest.mark.parametrize("H,W", [(37, 53), (64, 64)])
@pytest.mark.parametrize("edges", list(EDGES))
def test_distance_zones(H, W, edges):
    masks = _shapes(H, W)
    e = EDGES[edges]
    g = torch.from_numpy(masks).to(DEV)
    for side in ("both", "inside", "outside"):
        want, nz = Zr.distance_zones(masks, e, side)
        got, gnz = distance_zones(g, e, side=side)
        assert gnz == nz == 2 * len(e) + 2 and got.is_cuda
        _same(got, want, f"{edges} {side}")
    n = len(e)
    both = got = distance_zones(g, e)[0]
    assert (both[2] == 2 * n + 1).all() and (both[3] == n).all()            # FAR: the deepest band on either side
    assert int(both[0].max()) <= 2 * n + 1
    # a single uint8 mask, a strided view, a host mask: the same bytes
    want = Zr.distance_zones(masks[:1], e)[0][0]
    _same(distance_zones(g[0].to(torch.uint8) * 7, e)[0], want, "uint8 [H, W]")
    _same(distance_zones(_crop_view(masks.view(np.uint8), 0).view(torch.bool)[:1], e)[0], want[None], "crop view")
    host = distance_zones(torch.from_numpy(masks[0]), e)[0]
    assert not host.is_cuda and np.array_equal(host.numpy(), want)
    # the bands as a zone map of the zonal table
    img = _stained(4, H, W, 5)
    z = stain_zonal(torch.from_numpy(img).to(DEV), both, 2 * n + 2)
    tab, unz = Zr.table(img, both.cpu().numpy(), 2 * n + 2, _m32(), THR)
    _check_single(z, tab, unz, "bands as zones")
    assert (z["unzoned"] == 0).all()


# ---- 7. capture and replay --------------------------------------------------------------------------------------------
def test_zonal_calls_in_a_captured_graph():
    B, H, W, Z, M = 2, 64, 64, 5, 64
    a, a2 = _stained(B, H, W, 61), _stained(B, H, W, 62)
    pats = dict((n, z) for n, z, _ in _patterns(B, H, W, 3))
    zones, zones2 = pats["unzoned areas"], pats["unzoned mixed"]
    rng = np.random.default_rng(4)
    lab1 = (rng.integers(0, 40, size=(B, H // 4, W // 4)).repeat(4, 1).repeat(4, 2) * (rng.random((B, H, W)) < 0.7)).astype(np.int32)
    lab2 = (rng.integers(0, 90, size=(B, H // 2, W // 2)).repeat(2, 1).repeat(2, 2) * (rng.random((B, H, W)) < 0.5)).astype(np.int32)
    ga, gz, gl = torch.from_numpy(a).to(DEV), torch.from_numpy(zones).to(DEV), torch.from_numpy(lab1).to(DEV)
    eager_z, eager_o = stain_zonal(ga, gz, Z), object_zones(gl, gz, Z, max_objects=M, return_overlap=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                  # one stream, a plain chain of launches: no parallel branches
        out_z = stain_zonal(ga, gz, Z)
        out_o = object_zones(gl, gz, Z, max_objects=M, return_overlap=True)
    for v in (out_z["counts"], out_z["unzoned"], out_z["derived"], *out_o.values()):
        v.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out_z[k], eager_z[k]) for k in ("counts", "unzoned", "derived"))
    assert all(torch.equal(out_o[k], eager_o[k]) for k in eager_o)
    ga.copy_(torch.from_numpy(a2))                 # the graph reads its inputs at replay
    gz.copy_(torch.from_numpy(zones2))
    gl.copy_(torch.from_numpy(lab2))
    graph.replay()
    torch.cuda.synchronize()
    _check_single(out_z, *Zr.table(a2, zones2, Z, _m32(), THR), "replay")
    ref = Zr.object_zones(lab2, zones2, Z, M)
    assert int(ref["count"].max()) > M             # labels beyond the table
    for k in OBJECT_KEYS:
        _same(out_o[k], ref[k], f"replay {k}")
    del graph


# ---- 8. the class map of the multiclass mask head as the zone map (the README's example, end to end) -------------------
def test_class_map_of_the_mask_head_as_zones():
    from stain2stain_amd import (FlowMatchingDecoder, MultiTaskFlowMatchingModule, SegmentationDecoder, SharedEncoder,
                                 SolverConfig, multitask_sampler, render_classes, translate_region)
    torch.manual_seed(1984)
    enc = SharedEncoder(3, [16, 32], precision="fp32")
    fdec = FlowMatchingDecoder(32, [16], 3, 32, precision="fp32")
    sdec = SegmentationDecoder(32, [16], 3, precision="fp32")
    mod = MultiTaskFlowMatchingModule(enc, fdec, sdec, time_emb_dim=32, num_classes=3, solver=SolverConfig("euler")).to(DEV)
    region = torch.from_numpy(_stained(1, 72, 88, 81)[0]).to(DEV)
    with torch.no_grad():
        gen, probs = translate_region(region, multitask_sampler(mod, 2), tile=32, overlap=8, batch=4)
    assert tuple(probs.shape) == (72, 88, 3)
    zones = probs.argmax(-1).to(torch.uint8)
    r = region_stain_zonal(gen, zones, num_zones=probs.shape[-1])
    tab, unz = Zr.table(gen.cpu().numpy()[None], zones.cpu().numpy()[None], 3, _m32(), THR)
    _check_single(r, tab, unz, "class map")
    assert int(r["pixels"].sum()) == 72 * 88 and int(r["unzoned"][0]) == 0
    pic = render_classes(gen, zones)
    assert pic.dtype == torch.uint8 and tuple(pic.shape) == (72, 88, 3)
