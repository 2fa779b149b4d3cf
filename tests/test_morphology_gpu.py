"""The morphology kernels (csrc/morphology.hip) against the numpy / scipy restatement of tests/morphology_ref.py, on poisoned
memory (every ``torch.empty`` and every ``ops._workspace`` slab starts as 0xFF, as in tests/test_objects_gpu.py).

Every integer output is compared with ``array_equal``.  The derived fp64 values are compared with numpy within 1 ulp: the
two divisions are correctly rounded on both sides, the device ``sqrt`` is allowed one ulp.

The column pass works in segments of SEGMENT = 64 rows; the row pass packs 1024 // W rows into a workgroup, so a row wider
than PACK_WIDTH = 512 pixels is alone in its workgroup and a row wider than 256 takes more than one pixel per thread."""
import numpy as np
import pytest
import torch

import morphology_ref as M
from stain2stain_amd import (distance_transform, fill_holes, mask_boundary, mask_boundary_agreement, mask_morphology)
from stain2stain_amd.morphology import FAR, PACK_WIDTH, SEGMENT

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1), (1, 9), (5, 1), (SEGMENT - 1, 65), (2 * SEGMENT + 1, 131), (97, 131), (300, 520), (3, PACK_WIDTH + 1),
          (3, 2 * PACK_WIDTH + 1)]
RADII = (0, 1, 1.5, 2, 5)


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


def _stack(H, W):
    names, masks = zip(*M.patterns(H, W, seed=3 * H + W))
    return names, np.stack(masks)


def _bad(got, want, names):
    return [n for n, g, w in zip(names, got, want) if not np.array_equal(g, w)]


def _ulp_close(got, want):
    return np.all(np.abs(got - want) <= np.spacing(np.abs(want)))


# ---- the distance transform -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_distance_transform_every_pattern(H, W):
    names, masks = _stack(H, W)                       # one batch: every pattern is a sample with its own content
    for to in ("background", "foreground"):
        got = distance_transform(_gpu(masks), to=to)
        assert got.dtype == torch.int32 and got.shape == masks.shape
        assert not _bad(got.cpu().numpy(), M.d2_batch(masks, to), names), to
    full = distance_transform(_gpu(masks[1:2]))
    assert int(full.min()) == FAR                     # all foreground: no background site
    c = distance_transform(_gpu(masks[2]), to="foreground")          # a single site in corner (0, 0), no batch dimension
    assert c.shape == (H, W) and int(c[H - 1, W - 1]) == (H - 1) ** 2 + (W - 1) ** 2


@pytest.mark.parametrize("H,W", [(97, 131), (3, PACK_WIDTH + 1)])
@pytest.mark.parametrize("max_dist", [0, 1, 4.5, 30])
def test_distance_transform_max_dist(H, W, max_dist):
    names, masks = _stack(H, W)
    for to in ("background", "foreground"):
        got = distance_transform(_gpu(masks), to=to, max_dist=max_dist).cpu().numpy()
        assert not _bad(got, M.d2_batch(masks, to, max_dist), names), to


def test_views_bool_and_host_masks():
    rng = np.random.default_rng(5)
    m = rng.random((3, 70, 90)) < 0.6
    want = M.d2_batch(m, "background")
    assert np.array_equal(distance_transform(_gpu(m)).cpu().numpy(), want)
    u8 = _gpu(m.astype(np.uint8) * rng.integers(1, 256, size=m.shape).astype(np.uint8))
    assert np.array_equal(distance_transform(u8).cpu().numpy(), want)
    big = torch.zeros((3, 77, 101), dtype=torch.uint8, device=DEV)              # background all round the crop
    crop = big[:, 4:74, 5:95]
    crop.copy_(_gpu(m))
    assert not crop.is_contiguous()
    assert np.array_equal(distance_transform(crop).cpu().numpy(), want)
    assert np.array_equal(mask_morphology(crop, "erode", 2).cpu().numpy(), np.stack([M.erode(x, 2) for x in m]))
    assert np.array_equal(mask_boundary(crop).cpu().numpy(), np.stack([M.boundary(x) for x in m]))
    assert np.array_equal(fill_holes(crop).cpu().numpy(), np.stack([M.fill_holes(x) for x in m]))
    cols = _gpu(m).transpose(1, 2)                                              # columns not contiguous: copied
    assert np.array_equal(distance_transform(cols).cpu().numpy(), M.d2_batch(m.transpose(0, 2, 1), "background"))
    host = torch.from_numpy(m)
    out = distance_transform(host)
    assert not out.is_cuda and np.array_equal(out.numpy(), want)
    closed = mask_morphology(host, "close", 1.5)
    assert closed.dtype == torch.bool and not closed.is_cuda
    assert np.array_equal(closed.numpy(), np.stack([M.morphology(x, "close", 1.5) for x in m]) > 0)
    # a sample's values do not depend on its batch mates
    whole = distance_transform(_gpu(m), to="foreground")
    for n in range(3):
        assert torch.equal(distance_transform(_gpu(m[n]), to="foreground"), whole[n])


# ---- disc morphology --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_morphology_against_the_reference(H, W):
    names, masks = _stack(H, W)
    g = _gpu(masks)
    big = H * W > 100000                                                        # (the reference takes its time there)
    for r in ((1.5, 5) if big else RADII) + (H + W,):                           # the last one is larger than the image
        for op in ("open", "close") if big else ("dilate", "erode", "open", "close"):
            got = mask_morphology(g, op, r)
            assert got.dtype == torch.uint8 and got.shape == masks.shape and int(got.max()) <= 1
            assert not _bad(got.cpu().numpy(), [M.morphology(m, op, r) for m in masks], names), (op, r)


@pytest.mark.parametrize("H,W", [(1, 9), (5, 1), (SEGMENT - 1, 65), (97, 131), (3, PACK_WIDTH + 1)])
def test_morphology_against_scipy(H, W):
    names, masks = _stack(H, W)
    g = _gpu(masks)
    for r in RADII:
        for op in ("dilate", "erode", "open", "close"):
            got = mask_morphology(g, op, r).cpu().numpy()
            assert not _bad(got, [M.scipy_morphology(m, op, r) for m in masks], names), (op, r)


# ---- hole filling -----------------------------------------------------------------------------------------------------
def test_fill_holes():
    H, W = 97, 131
    diag = np.ones((H, W), np.uint8)
    diag[40, 40] = diag[39, 39] = 0
    diag[:39, :39][np.eye(39, dtype=bool)] = 0                                  # reaches (0, 0) through diagonal steps only
    cases = {"ring": M.ring(H, W, 48, 65, 30, 12), "ring on the border": M.ring(H, W, 10, 65, 30, 12),
             "diagonal": diag, "nested": M.ring(H, W, 48, 65, 45, 38) | M.ring(H, W, 48, 65, 25, 10) | M.discs(H, W, [(48, 65, 4)]),
             "bernoulli": M.bernoulli((H, W), 0.6, 2), "empty": np.zeros((H, W), np.uint8), "full": np.ones((H, W), np.uint8)}
    names, masks = list(cases), np.stack(list(cases.values()))
    from scipy import ndimage
    for conn in (4, 8):
        got = fill_holes(_gpu(masks), connectivity=conn).cpu().numpy()
        assert not _bad(got, [M.fill_holes(m, conn) for m in masks], names), conn
        structure = None if conn == 4 else M.SQUARE
        assert not _bad(got, [ndimage.binary_fill_holes(m, structure).astype(np.uint8) for m in masks], names), conn
    f4, f8 = fill_holes(_gpu(diag), 4), fill_holes(_gpu(diag), 8)
    assert int(f4[40, 40]) == 1 and int(f8[40, 40]) == 0 and int(f4[0, 0]) == 0
    assert int(fill_holes(_gpu(cases["ring"]))[48, 65]) == 1 and int(fill_holes(_gpu(cases["ring on the border"]))[0, 65]) == 0
    for H, W in [(1, 1), (1, 9), (5, 1), (3, PACK_WIDTH + 1)]:
        m = M.bernoulli((2, H, W), 0.5, H + W)
        assert np.array_equal(fill_holes(_gpu(m)).cpu().numpy(), np.stack([M.fill_holes(x) for x in m]))


def test_mask_boundary():
    for H, W in SHAPES:
        names, masks = _stack(H, W)
        got = mask_boundary(_gpu(masks)).cpu().numpy()
        assert not _bad(got, [M.boundary(m) for m in masks], names), (H, W)
    assert mask_boundary(_gpu(np.ones((4, 4), bool))).dtype == torch.bool


# ---- boundary agreement -----------------------------------------------------------------------------------------------
DTYPES = dict({k: np.int64 for k in M.INT_KEYS}, max_d2=np.int32, pq_d2=np.int32, valid=np.int32,
              **{k: np.float64 for k in M.F64_KEYS})


def _agree(pred, target, what, **kw):
    got = {k: v.cpu().numpy() for k, v in mask_boundary_agreement(_gpu(pred), _gpu(target), **kw).items()}
    ref = M.agreement_batch(pred, target, **kw)
    assert sorted(got) == sorted(ref), what
    for k in M.INT_KEYS:
        assert got[k].dtype == DTYPES[k] and got[k].shape == ref[k].shape, (what, k)
        assert np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])
    for k in M.F64_KEYS:
        assert got[k].dtype == np.float64 and np.isfinite(got[k]).all(), (what, k)
        assert _ulp_close(got[k], ref[k]), (what, k, got[k], ref[k])
    return got


def _pairs(H, W):
    """pred / target [B, H, W]: identical, shifted by (3, 4), disc in disc, random pairs, both degenerate cases."""
    a = M.two_discs(H, W)
    z = np.zeros((H, W), np.uint8)
    small = M.discs(H, W, [(H * 0.5, W * 0.5, min(H, W) * 0.2)])
    large = M.discs(H, W, [(H * 0.5, W * 0.5, min(H, W) * 0.4)])
    r0, r1, r2 = (M.bernoulli((H, W), p, 11 + i) for i, p in enumerate((0.3, 0.7, 0.98)))
    blobs = M.scipy_dilate(M.bernoulli((H, W), 0.004, 21), 5)
    pred = [a, a, small, r0, r1, blobs, z, a, z, M.corners(H, W)[0]]
    target = [a, np.roll(a, (3, 4), axis=(0, 1)), large, r1, r2, np.roll(blobs, (-2, 5), axis=(0, 1)), z, z, a,
              M.corners(H, W)[3]]
    return np.stack(pred), np.stack(target)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (5, 1), (SEGMENT - 1, 65), (2 * SEGMENT + 1, 131), (97, 131),
                                 (300, 520), (3, 2 * PACK_WIDTH + 1)])
def test_agreement_pairs(H, W):
    pred, target = _pairs(H, W)
    got = _agree(pred, target, f"{H}x{W}")
    far = (H - 1) ** 2 + (W - 1) ** 2
    assert got["valid"][0] == 1 or got["boundary_pred"][0] == 0
    assert got["max_d2"][0] == 0 and got["sum_q8"][0] == 0 and got["surface_dice"][0] == 1          # identical masks
    assert got["valid"][6] == 0 and got["surface_dice"][6] == 1 and got["max_d2"][6] == 0           # both empty
    if pred[7].any():
        assert got["valid"][7] == 0 and got["valid"][8] == 0 and got["max_d2"][7] == far and got["pq_d2"][8] == far
    if min(H, W) > 1:
        assert got["max_d2"][9] == far and got["valid"][9] == 1                                     # corner to corner


@pytest.mark.parametrize("kw", [{"percentile": 100}, {"percentile": 1}, {"percentile": 50, "tolerance": 0},
                                {"tolerance": 4.5}, {"tolerance": 5, "percentile": 99}])
def test_agreement_arguments(kw):
    pred, target = _pairs(97, 131)
    got = _agree(pred, target, str(kw), **kw)
    if kw.get("percentile") == 100:
        assert np.array_equal(got["pq_d2"], got["max_d2"]) and np.array_equal(got["hd"], got["hausdorff"])
    if kw.get("tolerance") == 5:
        assert got["max_d2"][1] <= 25 and got["surface_dice"][1] == 1                               # the (3, 4) shift


def test_agreement_without_batch_dimension_views_and_determinism():
    pred, target = _pairs(97, 131)
    whole = mask_boundary_agreement(_gpu(pred), _gpu(target))
    again = mask_boundary_agreement(_gpu(pred), _gpu(target))
    for k in whole:
        assert torch.equal(whole[k], again[k]), k
    one = mask_boundary_agreement(_gpu(pred[5]) > 0, _gpu(target[5]) > 0)
    for k in whole:
        assert one[k].dim() == 0 and torch.equal(one[k], whole[k][5]), k
    big = torch.ones((10, 100, 140), dtype=torch.uint8, device=DEV)
    crop = big[:, 2:99, 3:134]
    crop.copy_(_gpu(pred))
    strided = mask_boundary_agreement(crop, _gpu(target))
    for k in whole:
        assert torch.equal(strided[k], whole[k]), k


def test_stale_workspace(poison, monkeypatch):
    from stain2stain_amd import ops
    pred, target = _pairs(300, 520)
    _agree(pred, target, "big")
    monkeypatch.setattr(ops, "_workspace", poison)            # from here on the workspace keeps what the big call left
    p, t = _pairs(97, 131)
    _agree(p, t, "small after big")
    names, masks = _stack(97, 131)
    assert not _bad(distance_transform(_gpu(masks)).cpu().numpy(), M.d2_batch(masks), names)
    assert not _bad(fill_holes(_gpu(masks)).cpu().numpy(), [M.fill_holes(m) for m in masks], names)


def test_no_host_synchronisation():
    pred, target = (_gpu(x) for x in _pairs(97, 131))
    calls = [lambda: distance_transform(pred, max_dist=9), lambda: mask_morphology(pred, "close", 3),
             lambda: fill_holes(pred), lambda: mask_boundary(pred), lambda: mask_boundary_agreement(pred, target)]
    for f in calls:                                           # the workspaces exist from here on
        f()
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = [f() for f in calls]
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert int(out[0].min()) == 0 and int(out[4]["valid"].sum()) > 0


# ---- the trainer ------------------------------------------------------------------------------------------------------
def _trainer(ncls=None):
    from stain2stain_amd import FlowMatchingDecoder, MultiTaskTrainer, SegmentationDecoder, SharedEncoder
    torch.manual_seed(1984)
    enc = SharedEncoder(3, [16, 32], precision="fp32")
    fdec = FlowMatchingDecoder(32, [16], 3, 32, precision="fp32")
    sdec = SegmentationDecoder(32, [16], ncls or 1, precision="fp32")
    nets = tuple(m.to(DEV).train() for m in (enc, fdec, sdec))
    return nets, MultiTaskTrainer(*nets, time_emb_dim=32, num_classes=ncls)


def test_trainer_evaluate_boundary():
    from stain2stain_amd import evaluation
    (enc, _, sdec), tr = _trainer()
    g = torch.Generator().manual_seed(7)
    x0 = (torch.rand(3, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    x1 = (torch.rand(3, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    t = torch.rand(3, generator=g).to(DEV)
    mask = torch.from_numpy(np.stack([M.two_discs(64, 64), M.discs(64, 64, [(30, 30, 12)]),
                                      np.zeros((64, 64), np.uint8)])[:, None]).float().to(DEV)
    old = tr.evaluate(x0, x1, mask, t)
    assert sorted(old) == sorted(["loss", "flow_loss", "seg_loss", "seg_dice", "seg_bce", "dice_coef", "iou"])
    kw = {"tolerance": 3, "percentile": 90}
    out = tr.evaluate(x0, x1, mask, t, boundary=kw)
    assert sorted(out) == sorted(list(old) + ["boundary/hd", "boundary/assd", "boundary/surface_dice"])
    for k in old:
        assert torch.equal(out[k], old[k]), k
    with torch.no_grad():
        logits = evaluation.mask_logits(enc, sdec, x0.float().contiguous())
    a = mask_boundary_agreement((logits > 0)[:, 0], (mask > 0)[:, 0], **kw)
    ref = M.agreement_batch((logits > 0)[:, 0].cpu().numpy(), (mask > 0)[:, 0].cpu().numpy(), **kw)
    for k in ("hd", "assd", "surface_dice"):
        assert torch.equal(out[f"boundary/{k}"], a[k].mean()), k
        assert _ulp_close(a[k].cpu().numpy(), ref[k]), k
    assert sorted(tr.evaluate(x0, x1, mask, t, boundary={})) == sorted(out)
    tr.close()
    _, mc = _trainer(4)
    with pytest.raises(ValueError, match="binary"):
        mc.evaluate(x0, x1, torch.zeros((3, 64, 64), dtype=torch.long, device=DEV), t, boundary={})
    mc.close()
