"""The tables of tests/wgrad_forms_ref.py against the library's plan queries (host code, no GPU): every row still gets the
launch plan it was written for, and the tables as a whole still contain every form the weight-gradient kernels have.  A
retuning of the split rule, the fold choice or the head dispatch that moves a row out of its form fails here, so that
tests/test_wgrad_forms_gpu.py cannot quietly stop covering it.  (The tables hold the plans with no launch switch set,
which is how the suite runs this file.)"""
import pytest
import torch

import wgrad_forms_ref as R

BF, F32 = torch.bfloat16, torch.float32


@pytest.mark.parametrize("name", list(R.CONV3X3))
def test_conv3x3_wgrad_row_has_its_plan(name):
    from stain2stain_amd import _native, ops
    (B, H, W, c0, c1, cout), (S, tiles, xcd, fold) = R.CONV3X3[name]
    got = ops.conv3x3_wgrad_plan(BF, B, H, W, c0 + c1, cout)
    assert got == {"splits": S, "tiles": tiles, "xcd": xcd, "fold": fold, "kernel": 0}, got
    got = ops.conv3x3_wgrad_plan(F32, B, H, W, c0 + c1, cout)
    assert got == {"splits": S, "tiles": tiles, "xcd": 0, "fold": fold, "kernel": 1}, got
    # the query and the sizing call of the launcher agree
    assert _native.lib().s2s_conv3x3_wgrad_splits(0, B, H, W, c0 + c1, cout) == S
    assert S <= tiles and c0 % 8 == 0 and c1 % 8 == 0 and cout % 8 == 0


def test_conv3x3_wgrad_plan_refuses_what_the_launch_refuses():
    from stain2stain_amd import _native
    L = _native.lib()
    assert L.s2s_conv3x3_wgrad_plan(0, 0, 8, 8, 8, 8, 0) == -1
    assert L.s2s_conv3x3_wgrad_plan(7, 1, 8, 8, 8, 8, 0) == -3
    assert L.s2s_conv3x3_wgrad_plan(0, 1, 8, 8, 8, 8, 5) == -1
    assert L.s2s_head_family(7, 1, 8, 8, 8, 3, 1) == -3
    assert L.s2s_head_family(0, 1, 8, 8, 12, 3, 1) == -1


def _walk_lengths(name):
    return sorted({len(w) for w in R.conv3x3_walks(name)})


def test_conv3x3_wgrad_table_contains_every_form():
    T = R.CONV3X3
    lens = {n: _walk_lengths(n) for n in T}
    plan = {n: T[n][1] for n in T}
    cin = {n: T[n][0][3] + T[n][0][4] for n in T}
    cout = {n: T[n][0][5] for n in T}

    def some(pred, what):
        hits = [n for n in T if pred(n)]
        assert hits, what
        return hits

    some(lambda n: lens[n] == [1], "a walk of exactly one tile")
    some(lambda n: len(lens[n]) == 2 and lens[n][1] >= 3, "an uneven walk: some split owns >= 3 tiles, another fewer")
    some(lambda n: len(lens[n]) == 1 and lens[n][0] >= 3 and plan[n][0] > 1, "an even walk of >= 3 tiles")
    some(lambda n: plan[n][0] == 1 and plan[n][1] > 1, "splits == 1 with more than one tile")
    some(lambda n: plan[n][2] == 1 and lens[n][-1] >= 3, "XCD-aware order with a walk of >= 3")
    some(lambda n: plan[n][2] == 0 and lens[n][-1] >= 3, "plain order with a walk of >= 3")
    some(lambda n: plan[n][3] == 16 and plan[n][0] % 16 != 0, "fold with 16 waves and S % 16 != 0")
    some(lambda n: plan[n][3] == 4 and plan[n][0] % 4 != 0, "fold with 4 waves and S % 4 != 0")
    edge = some(lambda n: cout[n] * cin[n] == R.FOLD_LIMIT and plan[n][0] >= 32, "Cout Cin == 32768 with S >= 32")
    assert all(plan[n][3] == 16 for n in edge)
    # the nearest shape above the edge: one more piece of 8 input channels on the same map and Cout, and the other fold
    above = [n for n in T for e in edge if T[n][0][:3] == T[e][0][:3] and cout[n] == cout[e] and cin[n] == cin[e] + 8]
    assert above and all(plan[n][3] == 4 for n in above), "the shape just above the fold edge"
    some(lambda n: any(any(w) and not all(w) for w in R.conv3x3_walks(n)),
         "interior and border tiles inside one workgroup's walk")
    some(lambda n: not any(any(w) for w in R.conv3x3_walks(n)) and plan[n][1] > 1, "no interior tile at all")
    some(lambda n: T[n][0][4] > 0 and T[n][0][3] % 64 != 0, "a ci tile that spans both sources")
    some(lambda n: T[n][0][1] < 8 and T[n][0][2] < 16, "H < 8 and W < 16 together")


@pytest.mark.parametrize("name", list(R.STEM))
def test_stem_wgrad_row_has_its_plan(name):
    from stain2stain_amd import _native
    (B, H, W, cin, cout), (tiles, blocks, slabs) = R.STEM[name]
    assert tiles == B * -(-H // 16) * -(-W // 16)
    assert _native.lib().s2s_stem_wgrad_blocks(B, H, W) == blocks == min(tiles, 512)
    assert slabs == 2 * blocks


def test_stem_wgrad_table_contains_every_form():
    rows = list(R.STEM.values())
    assert any(tiles > 512 and blocks == 512 and tiles % 512 for (_, (tiles, blocks, _)) in rows)   # a second tile for some
    assert {r[0][3] for r in rows} == {1, 2, 3, 4, 5, 6}
    assert {r[0][4] for r in rows} == {8, 16, 64, 72, 136}
    # stem_wgrad_reduce_kernel: the unrolled loop (b + 32 < slabs) with and without a tail, and the tail loop alone
    slabs = {r[1][2] for r in rows}
    assert any(s <= 32 for s in slabs) and any(s > 32 and (s - 1) % 64 >= 32 for s in slabs)
    assert any(s > 32 and (s - 1) % 64 < 32 for s in slabs)
    assert any(r[0][1] % 16 and r[0][2] % 16 for r in rows)


@pytest.mark.parametrize("C,cout", list(R.HEAD), ids=[f"{c}-{o}" for c, o in R.HEAD])
def test_head_row_has_its_family(C, cout):
    from stain2stain_amd import ops
    for dtype in (BF, F32):
        for px in R.head_pixels(C):
            for fwd in (True, False):
                assert ops.head_family(dtype, *px, C, cout, fwd) == R.HEAD[(C, cout)], (dtype, px, fwd)


def test_head_table_contains_every_form():
    from stain2stain_amd import _native, ops
    fams = set(R.HEAD.values())
    assert fams == {1, 2, 4, 8, 16, 32, 64, R.HEAD_MO4, R.HEAD_MO8}
    assert (R.HEAD_MO4, R.HEAD_MO8) == (ops.HEAD_FALLBACK_MO4, ops.HEAD_FALLBACK_MO8)
    assert R.HEAD[(64, 3)] == 8 and R.HEAD[(64, 4)] == 8            # the segmentation head at production width
    for C, cout, fwd in R.HEAD_REFUSED:
        assert ops.head_family(BF, 1, 7, 9, C, cout, fwd) < 0, (C, cout, fwd)
    assert any(not fwd and cout <= 8 for _, cout, fwd in R.HEAD_REFUSED)        # a refusal of the backward alone
    assert ops.head_family(BF, 1, 7, 9, 512, 4, True) == 64
    # the backward's block cap is reached with an uneven share, and not by the smaller pixel counts
    L = _native.lib()
    nb = [L.s2s_head_wgrad_blocks(*px) for px in R.HEAD_PIXELS]
    assert nb == [1, 1, 20, R.HEAD_BLOCK_CAP]
    B, H, W = R.HEAD_PIXELS[-1]
    blocks64 = -(-B * H * W // 64)
    assert blocks64 > R.HEAD_BLOCK_CAP and blocks64 % R.HEAD_BLOCK_CAP != 0
