"""What of the paired tile registration can be checked without a GPU: the numpy restatement recovers the
planted shifts with a clear gap, the host arithmetic of the package equals the restatement, and arguments are refused
on the host before any launch."""
import ctypes
import random

import numpy as np
import pytest
import torch

import registration_ref as R
from stain2stain_amd import (overlap_boxes, register_pairs, sample_crop_params_within, shift_tiles, structure_map,
                             structure_weights)


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_recovers_the_planted_shifts(name):
    """The condition the GPU test rests on: each planted shift is the restatement's pick, and the best score leads the
    second best by more than 1e-3, so last-bit differences of sqrt and / cannot change the pick."""
    src, tgt, planted, kw = R.case(name)
    out = R.register(src, tgt, **kw)
    assert np.array_equal(out["shift"], planted) and out["valid"].all()
    Rl = (out["scores"].shape[1] - 1) // 2
    for s in range(3):
        gap = R.runner_up_gap(out["scores"][s], Rl)
        print(f"{name}[{s}]: score {out['score'][s]:.4f}, centre {out['score_center'][s]:.4f}, gap {gap:.2e}")
        assert gap > 1e-3
        assert out["score"][s] > 0.3 and out["margin"][s] >= gap


def test_restated_pick_is_a_total_order():
    scores = np.zeros((5, 5))
    scores[0, 4] = scores[4, 0] = scores[1, 2] = scores[2, 1] = 0.5      # d2 = 8, 8, 1, 1
    tsum = np.array([4, 10, 30])
    assert R.pick(tsum, scores, 2)[0] == (-1, 0)                         # nearest, then the smaller dy
    scores[2, 1] = 0.0
    scores[3, 2] = 0.5
    assert R.pick(tsum, scores, 2, 7, -3, 2)[0] == ((7 - 1) * 2, -3 * 2)
    assert R.pick(np.array([4, 10, 25]), scores, 2, 7, -3)[::4] == ((7, -3), 0)    # va = 0
    assert R.pick(np.zeros(3, np.int64), scores, 2, -2 ** 31, 2 ** 31 - 1, 4)[0] == (-2 ** 31, 2 ** 31 - 1)


def test_structure_weights_equal_the_restatement():
    assert structure_weights("hed").tolist() == [3000, -105, -961]
    assert structure_weights("hdab").tolist() == [1920, 1096, -1468]
    fitted = np.array([[0.5626, 0.7201, 0.4062], [0.2159, 0.8012, 0.5581]])
    for stains in ("hed", "hdab", fitted):
        for k in range(3):
            for gain in (100.0, 37.5):
                w = structure_weights(stains, k, gain)
                assert w.dtype == torch.int32 and not w.is_cuda
                assert w.tolist() == R.weights(stains, k, gain).tolist(), (k, gain)
    for bad in (0.0, -1.0, float("nan"), 1e9):
        with pytest.raises(ValueError, match="gain"):
            structure_weights("hed", 0, bad)
    with pytest.raises(ValueError, match="stain"):
        structure_weights("hed", 3)


def test_the_integer_table_is_the_one_of_stain_norm():
    from stain2stain_amd.stain_norm import q_table
    assert q_table().tolist() == R.q_table().tolist()


def test_sample_crop_params_within_stays_inside_its_boxes():
    boxes = torch.tensor([[0, 5, 70, 85], [2, 0, 68, 90], [3, 7, 64, 64]], dtype=torch.int32)
    seen = set()
    for seed in range(50):
        p = sample_crop_params_within(boxes, 64, random.Random(seed))
        assert p.dtype == torch.int32 and tuple(p.shape) == (3, 5)
        for (top, left, bh, bw), (t, l, hf, vf, tr) in zip(boxes.tolist(), p.tolist()):
            assert top <= t and t + 64 <= top + bh and left <= l and l + 64 <= left + bw
            assert {hf, vf, tr} <= {0, 1}
        assert p[2, :2].tolist() == [3, 7]
        seen.add(tuple(p[0].tolist()))
    assert len(seen) > 20
    a, b = (sample_crop_params_within(boxes, 64, random.Random(3)) for _ in range(2))
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="box 2"):
        sample_crop_params_within(boxes, 66, random.Random(0))
    with pytest.raises(ValueError, match="boxes"):
        sample_crop_params_within(boxes[:, :3], 8)
    with pytest.raises(ValueError, match="size"):
        sample_crop_params_within(boxes, 0)


def test_overlap_boxes_on_host_tensors():
    shift = torch.tensor([[0, 0], [3, -2], [-5, 7], [70, 1], [-70, -90], [2 ** 31 - 1, -2 ** 31]], dtype=torch.int32)
    got = overlap_boxes(shift, 70, 90)
    assert got.dtype == torch.int32 and tuple(got.shape) == (6, 4)
    for (dy, dx), (top, left, bh, bw) in zip(shift.tolist(), got.tolist()):
        ys = [y for y in range(70) if 0 <= y + dy < 70]
        xs = [x for x in range(90) if 0 <= x + dx < 90]
        assert (bh, bw) == (len(ys), len(xs))
        if ys:
            assert top == ys[0]
        if xs:
            assert left == xs[0]
    assert got[0].tolist() == [0, 0, 70, 90] and got[3, 2] == 0 and got[4, 2:].tolist() == [0, 0]
    with pytest.raises(ValueError, match="shift"):
        overlap_boxes(shift.float(), 70, 90)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from stain2stain_amd import _native
    lib = _native.lib()
    ok = ctypes.c_void_p(4096)
    q = (ctypes.c_int * 256)(*R.q_table().tolist())
    w = (ctypes.c_int * 3)(3000, -105, -961)
    sums = lambda B, h, wd, rad, a=ok, b=ok, t=ok, s=ok: lib.s2s_register_sums(a, b, B, h, wd, rad, None, t, s, None)  # noqa: E731
    # the shape status: R = 33, h = 2 R, w = 2 R, a template above 2^18 pixels, an empty batch
    assert sums(1, 256, 256, 33) == -1
    assert sums(1, 32, 256, 16) == -1 and sums(1, 256, 32, 16) == -1
    assert sums(1, 513 + 32, 512 + 32, 16) == -1
    assert sums(0, 64, 64, 8) == -1 and sums(1, 64, 64, -1) == -1
    # the null status
    for k in range(4):
        args = [ok] * 4
        args[k] = None
        assert sums(1, 64, 64, 8, *args) == -5
    pick = lambda B, rad, ds, *p: lib.s2s_register_pick(*p[:2], None, B, rad, ds, *p[2:], None)  # noqa: E731
    assert pick(1, 33, 1, ok, ok, ok, ok, ok) == -1 and pick(1, 8, 3, ok, ok, ok, ok, ok) == -1
    for k in range(5):
        args = [ok] * 5
        args[k] = None
        assert pick(1, 8, 1, *args) == -5
    smap = lambda img, qt, wt, out, ds=1, pitch=300, H=64, W=64: lib.s2s_structure_map_u8(  # noqa: E731
        img, pitch, pitch * H, 1, H, W, qt, wt, ds, out, None)
    assert smap(None, q, w, ok) == -5 and smap(ok, None, w, ok) == -5 and smap(ok, q, None, ok) == -5
    assert smap(ok, q, w, None) == -5
    assert smap(ok, q, w, ok, ds=3) == -1 and smap(ok, q, w, ok, pitch=191) == -1 and smap(ok, q, w, ok, ds=4, H=3) == -1
    big = (ctypes.c_int * 3)(2 ** 18, 0, 0)                  # 2^18 * q(1) overflows the int32 accumulator
    assert smap(ok, q, big, ok) == -1
    shift = lambda img, sh, out, C=3, fill=255, pitch=192: lib.s2s_shift_tiles_u8(  # noqa: E731
        img, pitch, pitch * 64, 1, 64, 64, C, sh, fill, out, 64 * C, 64 * 64 * C, None)
    assert shift(None, ok, ok) == -5 and shift(ok, None, ok) == -5 and shift(ok, ok, None) == -5
    assert shift(ok, ok, ok, C=2) == -1 and shift(ok, ok, ok, fill=256) == -1 and shift(ok, ok, ok, pitch=191) == -1


def test_wrappers_raise_on_bad_arguments():
    """Everything here is refused before a device is needed (a host tensor is refused as such last)."""
    u8 = torch.zeros((2, 40, 48, 3), dtype=torch.uint8)
    for bad in (u8.int(), u8.double(), u8[0], u8[..., :2], u8[:, :, ::2]):
        with pytest.raises(ValueError, match="src_u8|tgt_u8"):
            register_pairs(bad, bad)
    with pytest.raises(ValueError, match="differ in shape"):
        register_pairs(u8, u8[:, :39])
    with pytest.raises(ValueError, match="tgt_u8 is"):
        register_pairs(u8, u8.float())
    with pytest.raises(TypeError, match="tgt_u8"):
        register_pairs(u8, None)
    for bad in (0, 3, 8, -1):
        with pytest.raises(ValueError, match="downsample"):
            register_pairs(u8, u8, downsample=bad)
        with pytest.raises(ValueError, match="downsample"):
            structure_map(u8, downsample=bad)
    with pytest.raises(ValueError, match="radius"):
        register_pairs(u8, u8, radius=-1)
    with pytest.raises(ValueError, match="GPU"):
        register_pairs(u8, u8)                                # host tensors: there is no CPU path
    with pytest.raises(ValueError, match="tiles_u8"):
        structure_map(u8.int())
    with pytest.raises(ValueError, match="tiles_u8"):
        shift_tiles(u8.float(), torch.zeros((2, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="tiles_u8"):
        shift_tiles(u8[:, :, ::2], torch.zeros((2, 2), dtype=torch.int32))
