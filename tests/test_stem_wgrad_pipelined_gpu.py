"""The pipelined bf16 stem weight gradient (conv_edge.hip, stem_wgrad_pipe_kernel: dY by LDS-DMA into the other of two
buffers and the next tile's taps in registers while the current tile's MFMAs run) against the kernel it replaced
(``ops.stem_wgrad(..., _reference=True)``): ``dw`` and ``db`` bit for bit, on NaN-poisoned partial and output buffers.
Same tiles in the same order per slab, the same MFMA chain on the same bf16 values, so nothing may differ.

Shapes (B, H, W, Cin, Cout): one tile; ragged tiles (20 x 36); a Cout tail with two channel tiles (72); two channel groups
(Cin = 6); 576 tiles on 512 workgroups, so walks of one and of two tiles (the second through the prefetch).  One case
accumulates into a filled gradient, one takes dY as a channel slice (``lddy > Cout``).  The family query must say
"pipelined" for bf16 and "reference" for fp32 and for the reference call.  The kernels' accuracy against fp64 is held by
tests/test_wgrad_forms_gpu.py."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 16, 16, 3, 64), (2, 20, 36, 3, 64), (3, 48, 80, 3, 72), (2, 32, 32, 6, 64), (9, 128, 128, 3, 64)]


@pytest.fixture(autouse=True)
def poison():
    """torch.empty returns NaN-filled memory: the partial slabs inside ops.stem_wgrad start poisoned."""
    import torch.utils.deterministic as tud
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
            tud.fill_uninitialized_memory)
    torch.use_deterministic_algorithms(True, warn_only=True)
    tud.fill_uninitialized_memory = True
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
        tud.fill_uninitialized_memory = prev[2]


@functools.lru_cache(maxsize=None)
def inputs(shape):
    B, H, W, cin, cout = shape
    g = torch.Generator().manual_seed(sum(s * 31 ** i for i, s in enumerate(shape)))
    dy = torch.randn(B, H, W, cout, generator=g).bfloat16()
    x = torch.rand(B, cin, H, W, generator=g) * 2 - 1
    return dy.to(DEV), x.to(DEV)


def run_both(dy, x, accumulate):
    from stain2stain_amd import ops
    cout, cin = dy.shape[3], x.shape[1]
    out = []
    for reference in (False, True):
        assert ops.stem_wgrad_family(dy, x, _reference=reference) == (0 if reference else 1)
        if accumulate:
            g = torch.Generator().manual_seed(3)
            dw = torch.randn(cout, cin, 3, 3, generator=g).to(DEV)
            db = torch.randn(cout, generator=g).to(DEV)
        else:
            dw = torch.full((cout, cin, 3, 3), float("nan"), device=DEV)
            db = torch.full((cout,), float("nan"), device=DEV)
        ops.stem_wgrad(dy, x, dw, db, accumulate, _reference=reference)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
        out.append((dw, db))
    return out


def assert_same(new, old, what):
    for name, a, b in (("dw", new[0], old[0]), ("db", new[1], old[1])):
        assert torch.equal(a, b), f"{what} {name}: differs in {int((a != b).sum())} of {a.numel()}, max {float((a - b).abs().max()):.3e}"
    assert bool(new[0].any()) and bool(new[1].any()), what


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_pipelined_stem_wgrad_equals_the_reference_kernel(shape):
    dy, x = inputs(shape)
    new, old = run_both(dy, x, accumulate=False)
    assert_same(new, old, str(shape))


def test_accumulate_and_sliced_dy():
    shape = (2, 20, 36, 3, 64)
    dy, x = inputs(shape)
    new, old = run_both(dy, x, accumulate=True)
    assert_same(new, old, "accumulate")
    plain, _ = run_both(dy, x, accumulate=False)
    assert not torch.equal(plain[0], new[0])                       # it did add to what was there
    wide = torch.full((*dy.shape[:3], dy.shape[3] + 24), float("nan"), device=DEV, dtype=dy.dtype)
    wide[..., 8:8 + dy.shape[3]] = dy
    sl = wide[..., 8:8 + dy.shape[3]]
    assert sl.stride(2) > dy.shape[3]
    new_s, old_s = run_both(sl, x, accumulate=False)
    assert_same(new_s, old_s, "sliced dY")
    assert_same(new_s, plain, "sliced against dense")


def test_family_query():
    from stain2stain_amd import ops
    x = torch.zeros(1, 3, 16, 16, device=DEV)
    for dtype, fam in ((torch.bfloat16, 1), (torch.float32, 0)):
        dy = torch.zeros(1, 16, 16, 64, device=DEV, dtype=dtype)
        assert ops.stem_wgrad_family(dy, x) == fam
        assert ops.stem_wgrad_family(dy, x, _reference=True) == 0
    with pytest.raises(RuntimeError):
        ops.stem_wgrad_family(torch.zeros(1, 16, 16, 60, device=DEV, dtype=torch.bfloat16), x)
