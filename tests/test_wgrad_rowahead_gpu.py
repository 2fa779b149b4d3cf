"""The row-ahead tile loop of conv3x3_wgrad_dma_kernel against the loop it replaced, bit for bit.

The product kernel (fragments read a halo row ahead, operand DMAs through raw buffer resources, issued between the
MFMAs) adds the same products in the same order per accumulator as ``ops.conv3x3_wgrad(..., _reference=True)``, so both
the partial slabs (phase 1) and the folded OIHW gradient (phases 1 + 2, overwritten and accumulated) must be ARRAY-EQUAL.
The reference loop itself is held to float64 by tests/test_wgrad_forms_gpu.py.

Everything runs in bf16 on poisoned memory: the slabs start as NaN, the operands are channel slices of NaN-filled wider
buffers (dY, x0 and x1 with three different pixel strides), so a lane that reads outside its operand, or a slab element
nobody writes, shows as NaN.  Each case asserts its launch form through s2s_conv3x3_wgrad_plan (pixel tiles, splits, and
from them the walk lengths), so a case cannot silently degenerate when the split rule moves.

The cases (B, H, W, c0, c1, Cout):
  one_tile        one 8x16 tile, every halo row and column outside the image
  ragged_5x7      an image smaller than a tile
  ragged_13x21    2 x 2 tiles, all ragged
  mixed_24x48     interior and border tiles in one walk; Cin 72 and Cout 40 leave ragged channel tiles (two ci tiles)
  concat_24_16    x0 | x1 with c0 = 24: one 32-channel DMA group reads both tensors (the EXEC-masked pair of loads)
  concat_32_40    x0 | x1 with c0 = 32: the groups of a workgroup read different tensors, none both
  walk4_narrow    a narrow weight, 1024 tiles over 256 splits: every workgroup walks 4 tiles (even buffer parity)
  walk34_narrow   960 tiles over 256 splits: walks of 3 and 4, so the last DMA-ahead iteration and the buffer parity
                  differ between workgroups
  walk4_wide      64 x 64 pixels, B 2, a 256 x 256 weight: 16 splits of 4 tiles
  walk34_wide     64 x 64 pixels, B 2, a 192 x 256 weight: 21 splits of 3 or 4 tiles
  one_split       272 (co, ci) tiles: S = 1, one workgroup walks all four tiles
  width_16        W = 16: the halo columns on both sides are padding in every tile
(A narrow weight at 64 x 64 pixels, B 2 has 64 tiles and as many splits, a walk of one; the narrow walks therefore take a
256-pixel-wide image, and the 64 x 64 walks a wide weight.)
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
DEFAULT_SWITCHES = not (os.environ.get("S2S_WGRAD_XCD") or os.environ.get("S2S_WGRAD_BLOCKS"))

#        name            B   H    W   c0   c1  Cout   tiles splits walks
CASES = {
    "one_tile":      ((1,  8,  16,    8,   0,    8), (1,     1,  (1,))),
    "ragged_5x7":    ((2,  5,   7,   16,   0,    8), (2,     2,  (1,))),
    "ragged_13x21":  ((2, 13,  21,   16,   0,   24), (8,     8,  (1,))),
    "mixed_24x48":   ((2, 24,  48,   72,   0,   40), (18,   18,  (1,))),
    "concat_24_16":  ((2, 24,  48,   24,  16,   16), (18,   18,  (1,))),
    "concat_32_40":  ((1, 16,  32,   32,  40,   72), (4,     4,  (1,))),
    "walk4_narrow":  ((2, 256, 256,   8,   0,    8), (1024, 256, (4,))),
    "walk34_narrow": ((2, 256, 240,   8,   0,   16), (960,  256, (3, 4))),
    "walk4_wide":    ((2, 64,  64,  256,   0,  256), (64,   16,  (4,))),
    "walk34_wide":   ((2, 64,  64,  256,   0,  192), (64,   21,  (3, 4))),
    "one_split":     ((1, 16,  32, 1088,   0, 1024), (4,     1,  (4,))),
    "width_16":      ((1, 24,  16,   16,   0,   16), (3,     3,  (1,))),
}


def _slice_of_wide(t, before, after):
    B, H, W, C = t.shape
    wide = torch.full((B, H, W, before + C + after), NAN, dtype=t.dtype, device=t.device)
    wide[..., before:before + C] = t
    return wide[..., before:before + C]


_OPERANDS = {}


def _operands(name):
    """dY, x0, x1 of the case (made once, never written): strided views inside NaN-filled buffers."""
    if name not in _OPERANDS:
        (B, H, W, c0, c1, cout), _ = CASES[name]
        g = torch.Generator().manual_seed(sum(map(ord, name)))
        mk = lambda c: (torch.rand((B, H, W, c), generator=g) * 2 - 1).to(DEV, BF)
        dy = _slice_of_wide(mk(cout), 8, 16)
        x0 = _slice_of_wide(mk(c0), 16, 8)
        x1 = _slice_of_wide(mk(c1), 8, 40) if c1 else None
        assert dy.stride(2) == cout + 24 and x0.stride(2) == c0 + 24 and (x1 is None or x1.stride(2) == c1 + 48)
        _OPERANDS[name] = (dy, x0, x1)
    return _OPERANDS[name]


def _plan(name):
    from stain2stain_amd import ops
    (B, H, W, c0, c1, cout), (tiles, splits, walks) = CASES[name]
    plan = ops.conv3x3_wgrad_plan(BF, B, H, W, c0 + c1, cout)
    assert plan["kernel"] == 0 and plan["tiles"] == tiles, plan
    S = plan["splits"]
    got = tuple(sorted({len(range(z, tiles, S)) for z in range(S)}))
    if DEFAULT_SWITCHES:
        assert (S, got) == (splits, walks), (plan, got)
    return S


def _slabs(name, reference):
    from stain2stain_amd import ops
    (B, H, W, c0, c1, cout), _ = CASES[name]
    S = _plan(name)
    dy, x0, x1 = _operands(name)
    n = S * 9 * cout * (c0 + c1)
    part = torch.full((n + 64,), NAN, dtype=torch.float32, device=DEV)
    grad = torch.full((cout, c0 + c1, 3, 3), NAN, dtype=torch.float32, device=DEV)
    ops.conv3x3_wgrad(dy, x0, x1, grad, _reference=reference, _phases=1, _part=part)
    torch.cuda.synchronize()
    assert bool(torch.isnan(part[n:]).all()) and bool(torch.isnan(grad).all()), "phase 1 wrote outside its slabs"
    return part[:n]


@pytest.mark.parametrize("name", list(CASES))
def test_partial_slabs_equal_the_reference_loop(name):
    new, ref = _slabs(name, False), _slabs(name, True)
    assert not bool(torch.isnan(ref).any()), "the reference loop left slab elements unwritten"
    bad = (new != ref) | torch.isnan(new)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {new.numel()} slab elements differ, first at {int(bad.nonzero()[0])}"


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("name", list(CASES))
def test_folded_gradient_equals_the_reference_loop(name, accumulate):
    from stain2stain_amd import ops
    (B, H, W, c0, c1, cout), _ = CASES[name]
    S = _plan(name)
    dy, x0, x1 = _operands(name)
    g = torch.Generator().manual_seed(7)
    pre = (torch.rand((cout, c0 + c1, 3, 3), generator=g) * 2 - 1).to(DEV) if accumulate else None
    out = []
    for reference in (False, True):
        part = torch.full((S * 9 * cout * (c0 + c1),), NAN, dtype=torch.float32, device=DEV)
        grad = pre.clone() if accumulate else torch.full((cout, c0 + c1, 3, 3), NAN, dtype=torch.float32, device=DEV)
        ops.conv3x3_wgrad(dy, x0, x1, grad, accumulate=accumulate, _reference=reference, _part=part)
        out.append(grad)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[1]).any())
    assert torch.equal(out[0], out[1]), f"{name}: {int((out[0] != out[1]).sum())} gradient elements differ"
    if accumulate:
        assert not torch.equal(out[0], pre)
