"""The splitting kernels (csrc/split.hip) against the numpy restatement of tests/split_ref.py, on poisoned memory (every
``torch.empty`` and every ``ops._workspace`` slab starts as 0xFF, as in tests/test_object_features_gpu.py).

Everything the feature computes is an integer or one correctly rounded division of integers (the centroid), so every
comparison is ``array_equal``: labels, count, basins, kept_pixels, largest, size_hist and the tables.

The ascent pass's workgroup owns a TILE = 32 x 64 tile (rows x columns) and a wave one row of 64 columns; the other
passes take 256 consecutive raster indices or 256 columns of a row.  The shapes are the smallest that cross a wave's
columns, a tile and a row wider than one workgroup; ``test_peak_on_a_tile_corner_and_neck_on_a_tile_edge`` puts a peak on
the corner of four tiles and a neck on a tile edge."""
import numpy as np
import pytest
import torch

import morphology_ref as MR
import objects_ref as O
import split_ref as S
import stain_quant_ref as SQ

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1), (1, 9), (5, 1), (3, 5), (33, 65), (97, 131), (3, 1025)]
M_TABLE = 24
INT_KEYS = (*S.KEYS, *S.TABLE)
THR = (0.2, 0.15, 0.1)


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


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _fit(m, H, W):
    """A fixed-size pattern cut or zero-padded to H x W."""
    out = np.zeros((H, W), np.uint8)
    h, w = min(H, m.shape[0]), min(W, m.shape[1])
    out[:h, :w] = m[:h, :w]
    return out


def masks(H, W):
    """(name, mask) of every pattern at one shape."""
    yield from MR.patterns(H, W, seed=3 * H + W)
    yield "pair 18", _fit(S.disc_pair(18), H, W)
    yield "pair 10", _fit(S.disc_pair(10), H, W)
    yield "three discs", _fit(S.three_discs(), H, W)
    yield "rotated rectangle", _fit(S.rotated_rectangle(), H, W)
    yield "serpentine", O.serpentine(H, W)
    yield "objects checkerboard", O.checkerboard(H, W)
    yield "smoothed noise", _fit(S.smoothed_noise(), H, W)


_REF = {}


def _ref(names, ms, **kw):
    """The restatement of a batch, computed once per (patterns, arguments)."""
    key = (names, ms.shape, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = S.batch(ms, **kw)
    return _REF[key]


def _same(got, ref, names, keys=INT_KEYS):
    for k in keys:
        if k not in ref:
            continue
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (k, got[k].dtype, got[k].shape)
        bad = [n for n, g, w in zip(names, got[k], ref[k]) if not np.array_equal(g, w)]
        assert not bad, (k, bad)


# ---- every pattern at every shape -------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", SHAPES)
def test_every_pattern(H, W, connectivity):
    from stain2stain_amd import label_components, split_objects
    names, ms = zip(*masks(H, W))
    ms = np.stack(ms)
    ref = _ref(names, ms, connectivity=connectivity, max_objects=M_TABLE)
    res = split_objects(_gpu(ms), connectivity=connectivity, max_objects=M_TABLE)
    got = _np(res)
    assert sorted(got) == sorted([*INT_KEYS, "d2"])
    assert np.array_equal(got["d2"], MR.d2_batch(ms))
    _same(got, ref, names)
    # the properties that follow from the definition, on the GPU's own output
    comp = _np(label_components(_gpu(ms), connectivity=connectivity))
    assert (got["count"] >= comp["count"]).all() and (got["basins"] >= got["count"]).all()
    for n, name in enumerate(names):
        assert np.array_equal(got["labels"][n] > 0, ms[n] != 0), name
        if H * W <= 33 * 65:
            S.check_properties(ms[n], got["labels"][n], connectivity)
        else:                                               # one pass: a part never spans two components
            lab, c = got["labels"][n], comp["labels"][n]
            pairs = np.unique(np.stack([lab[lab > 0], c[lab > 0]]), axis=1)
            assert pairs.shape[1] == got["count"][n], name
    i_bg, i_fg = names.index("background"), names.index("foreground")
    assert got["count"][i_bg] == 0 and got["basins"][i_bg] == 0 and not got["labels"][i_bg].any()
    assert got["count"][i_fg] == 1 and got["basins"][i_fg] == 1 and (got["d2"][i_fg] == S.FAR).all()
    assert got["area"][i_fg, 0] == H * W and got["bbox"][i_fg, 0].tolist() == [0, 0, H, W]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("neck", [0.0, 0.5, 0.75, 0.9, 1.0])
def test_necks_cores_and_areas(neck, connectivity):
    from stain2stain_amd import split_objects
    H, W = 70, 90                                           # 3 x 2 tiles; the 64 x 64 patterns fit whole
    names, ms = zip(*masks(H, W))
    ms = np.stack(ms)
    dev = _gpu(ms)
    d2 = _gpu(MR.d2_batch(ms))
    for min_core, min_area in ((0.0, 1), (2.0, 1), (0.0, 5), (2.0, 5)):
        kw = dict(connectivity=connectivity, neck=neck, min_core=min_core, min_area=min_area)
        ref = _ref(names, ms, **kw)
        _same(_np(split_objects(dev, d2=d2, **kw)), ref, names, S.KEYS)
    if neck == 0.75:
        base = _ref(names, ms, connectivity=connectivity, neck=neck, min_core=0.0, min_area=1)["count"]
        assert (_ref(names, ms, connectivity=connectivity, neck=neck, min_core=2.0, min_area=1)["count"] < base).any()
        assert (_ref(names, ms, connectivity=connectivity, neck=neck, min_core=0.0, min_area=5)["count"] < base).any()


def test_the_counts_of_the_simple_shapes():
    from stain2stain_amd import label_components, split_objects
    pair, close, three, rot = S.disc_pair(18), S.disc_pair(10), S.three_discs(), S.rotated_rectangle()
    ms = _gpu(np.stack([pair, close, three, rot]))
    assert label_components(ms)["count"].tolist() == [1, 1, 1, 1]
    assert split_objects(ms, neck=0.75)["count"].tolist() == [2, 1, 3, 1]
    assert split_objects(ms, neck=0.5)["count"].tolist() == [1, 1, 3, 1]
    assert split_objects(ms, neck=0.9, connectivity=4)["count"].tolist()[3] == 12          # the documented over-segmentation
    noise = _gpu(S.smoothed_noise())
    assert label_components(noise)["count"].item() == 15
    assert [split_objects(noise, neck=n)["count"].item() for n in (0.5, 0.75, 0.9)] == [27, 30, 35]


def test_count_above_the_table():
    from stain2stain_amd import split_objects
    m = S.smoothed_noise()
    n = int(S.split(m)["count"])
    for M in (1, 7, n - 1, n, n + 5):
        got = _np(split_objects(_gpu(m), max_objects=M))
        ref = S.split(m, max_objects=M)
        assert got["count"] == n > 7
        for k in INT_KEYS:
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (M, k)


def test_peak_on_a_tile_corner_and_neck_on_a_tile_edge():
    from stain2stain_amd import split_objects
    from stain2stain_amd.split import TILE
    th, tw = TILE
    H, W = 2 * th + 9, 2 * tw + 11
    # a disc whose centre, its peak, is the first pixel of the fourth tile: its basin spans four tiles
    corner = S.disc(H, W, th, tw, 14)
    assert MR.d2(corner).argmax() == th * W + tw
    # two discs left and right of the seam between two tile columns: their parts meet between columns tw - 1 and tw
    edge = MR.discs(H, W, [(th + 6, tw - 9, 12), (th + 6, tw + 9, 12)])
    # ... and above and below the seam between two tile rows
    edge_rows = MR.discs(H, W, [(th - 9, 30, 12), (th + 9, 30, 12)])
    names = ("corner", "edge", "edge rows")
    ms = np.stack([corner, edge, edge_rows])
    for connectivity in (4, 8):
        for neck in (0.5, 0.75):
            ref = _ref(names, ms, connectivity=connectivity, neck=neck, max_objects=4)
            _same(_np(split_objects(_gpu(ms), connectivity=connectivity, neck=neck, max_objects=4)), ref, names)
    ref = _ref(names, ms, connectivity=8, neck=0.75, max_objects=4)
    assert ref["count"].tolist() == [1, 2, 2]
    assert ref["bbox"][1, :2, [1, 3]].T.tolist() == [[tw - 21, tw], [tw, tw + 22]]           # x0, x1 of the two parts
    assert ref["bbox"][2, :2, [0, 2]].T.tolist() == [[th - 21, th], [th, th + 22]]           # y0, y1


def test_long_chains():
    """A one-pixel-wide snake is nearly one plateau of d2 = 1, where the key is the raster index alone: the ascent runs
    along a full row, down the bend and back until the index stops rising, a chain of about two rows through every tile
    column."""
    from stain2stain_amd import split_objects
    for H, W in ((97, 131), (70, 200)):
        m = O.serpentine(H, W)
        for connectivity in (4, 8):
            root, _ = S.basins_of(MR.d2(m), connectivity)
            assert np.bincount(root[root >= 0]).max() >= 2 * W
            ref = S.split(m, connectivity=connectivity, max_objects=3)
            got = _np(split_objects(_gpu(m), connectivity=connectivity, max_objects=3))
            for k in INT_KEYS:
                assert np.array_equal(got[k], ref[k]), (H, W, connectivity, k)
            assert got["basins"] > got["count"] >= 1


# ---- batches and input forms ----------------------------------------------------------------------------------------------
def test_batch_isolation_and_no_batch_dimension():
    from stain2stain_amd import split_objects
    H, W = 97, 131
    ms = np.stack([_fit(S.smoothed_noise(), H, W), np.ones((H, W), np.uint8), MR.bernoulli((H, W), 0.7, 11)])
    whole = split_objects(_gpu(ms), max_objects=16)
    _same(_np(whole), _ref(("noise", "full", "bernoulli"), ms, max_objects=16), ("noise", "full", "bernoulli"))
    for n in range(3):
        alone = split_objects(_gpu(ms[n:n + 1]), max_objects=16)
        single = split_objects(_gpu(ms[n]), max_objects=16)
        for k, v in whole.items():
            assert torch.equal(alone[k][0], v[n]), (n, k)                 # bit-equal alone and inside a batch
            assert single[k].shape == v.shape[1:] and torch.equal(single[k], v[n]), (n, k)


def test_input_forms():
    from stain2stain_amd import distance_transform, split_objects
    H, W = 97, 131
    ms = np.stack([_fit(S.smoothed_noise(), H, W), _fit(S.disc_pair(18), H, W)])
    u8 = _gpu(ms)
    want = split_objects(u8, max_objects=8)
    big = torch.full((2, H + 5, W + 7), 1, dtype=torch.uint8, device=DEV)
    view = big[:, 2:2 + H, 3:3 + W]
    view.copy_(u8)
    assert not view.is_contiguous()
    forms = {"bool": split_objects(u8 > 0, max_objects=8), "values": split_objects(u8 * 200, max_objects=8),
             "view": split_objects(view, max_objects=8),
             "d2": split_objects(u8, max_objects=8, d2=distance_transform(u8))}
    for name, got in forms.items():
        assert sorted(got) == sorted(want)
        for k, v in want.items():
            assert got[k].dtype == v.dtype and torch.equal(got[k], v), (name, k)


# ---- the stain wrapper, the features of parts, the agreement of label images --------------------------------------------------
def _two_touching_positive_discs():
    """uint8 [1, 64, 64, 3]: haematoxylin tissue with the DAB-positive disc pair on it; (image, the pair's mask)."""
    pair = S.disc_pair(18)
    conc = np.zeros((1, 64, 64, 3))
    conc[..., 0] = 0.3
    conc[0, ..., 1] = np.where(pair > 0, 1.5, 0.0)
    return SQ.synthesise(conc, "hdab").astype(np.uint8), pair


def test_stain_object_split_and_the_features_of_the_parts():
    from stain2stain_amd import object_features, stain_object_split, stain_objects
    img, pair = _two_touching_positive_discs()
    inp = _gpu(img)
    whole = stain_objects(inp, thresholds=THR, mpp=0.5, return_labels=True)
    parts = stain_object_split(inp, thresholds=THR, mpp=0.5, max_objects=4, return_labels=True)
    assert np.array_equal(whole["labels"].cpu().numpy()[0] > 0, pair > 0)
    assert whole["count"].item() == 1 and parts["components"].item() == 1 and parts["count"].item() == 2
    assert sorted(parts) == sorted([*stain_objects(inp, thresholds=THR, mpp=0.5, max_objects=4, return_labels=True), "components"])
    for k in ("tissue", "positive", "burden"):
        assert torch.equal(parts[k], whole[k]), k
    assert parts["per_mm2"].item() == 2 * whole["per_mm2"].item()
    ref = S.split(pair, max_objects=4)
    assert np.array_equal(parts["labels"].cpu().numpy()[0], ref["labels"])
    for k in S.TABLE:
        assert np.array_equal(parts[k].cpu().numpy()[0], ref[k]), k
    f_whole = object_features(whole["labels"], max_objects=4)
    f_parts = object_features(parts["labels"], max_objects=4)
    assert f_whole["count"].item() == 1 and f_parts["count"].item() == 2
    assert f_parts["area"][0, :2].sum().item() == f_whole["area"][0, 0].item() == int(pair.sum())
    assert (f_parts["area"][0, :2] > 0).all() and f_parts["area"][0, 2:].sum().item() == 0


def test_label_agreement():
    from stain2stain_amd import label_agreement, split_objects, stain_object_agreement, stain_objects
    rng = np.random.default_rng(5)
    conc = np.zeros((2, 3, 60, 90, 3))
    conc[..., 0] = 0.3
    conc[..., 1] = np.where(rng.random((2, 3, 60, 90)) < 0.2, 1.5, 0.0)
    imgs = SQ.synthesise(conc, "hdab").astype(np.uint8)
    pred, target = _gpu(imgs[0]), _gpu(imgs[1])
    want = stain_object_agreement(pred, target, thresholds=THR, connectivity=4, min_area=2)
    a = stain_objects(pred, thresholds=THR, connectivity=4, min_area=2, return_labels=True)
    b = stain_objects(target, thresholds=THR, connectivity=4, min_area=2, return_labels=True)
    got = label_agreement(a["labels"], a["count"], b["labels"], b["count"])
    assert sorted(got) == sorted(want) and int(want["count_pred"].min()) > 5 and 0 < float(want["f1"].min()) < 1
    for k, v in want.items():
        assert got[k].dtype == v.dtype and torch.equal(got[k], v), k                   # bit for bit
    one = label_agreement(a["labels"][1], a["count"][1], b["labels"][1], b["count"][1])
    for k, v in want.items():
        assert one[k].dim() == 0 and torch.equal(one[k], v[1]), k
    # split labels: a prediction that covers both halves of the touching pair hits two target parts, not one component
    pair = S.disc_pair(18)
    blob = _gpu(S.rectangle(6, 40))
    assert (blob.cpu().numpy() & pair).any()
    for split, hits in ((False, 1), (True, 2)):
        from stain2stain_amd import label_components
        t = split_objects(_gpu(pair)) if split else label_components(_gpu(pair))
        p = label_components(blob)
        s = label_agreement(p["labels"], p["count"], t["labels"], t["count"])
        assert s["count_target"].item() == hits and s["recall"].item() == 1.0 and s["count_pred"].item() == 1
        assert s["count_abs_err"].item() == hits - 1


# ---- no hidden synchronisation ----------------------------------------------------------------------------------------
def test_does_not_synchronise():
    from stain2stain_amd import label_agreement, split_objects, stain_object_split
    img, pair = _two_touching_positive_discs()
    inp, m = _gpu(img), _gpu(pair)
    first = split_objects(m, max_objects=4)                                   # the workspaces exist from here on
    stain_object_split(inp, thresholds=THR, max_objects=4, mpp=0.5)
    label_agreement(first["labels"], first["count"], first["labels"], first["count"])
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = split_objects(m, max_objects=4)
        b = stain_object_split(inp, thresholds=THR, max_objects=4, mpp=0.5, return_labels=True)
        c = label_agreement(a["labels"], a["count"], b["labels"][0], b["count"][0])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.equal(a["labels"], b["labels"][0]) and a["count"].item() == 2 and c["f1"].item() == 1.0
