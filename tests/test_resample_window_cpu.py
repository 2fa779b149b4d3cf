"""What the 2 x 2 up-sampling backward (resample.hip, upsample2x_bwd_quad_kernel) rests on, without a GPU.

1. Window placement.  With the kernels' fp32 index arithmetic (ac_axis: scale = (n-1)/(2n-1), src = scale * dst,
   i0 = min((int)src, n-1), i1 = i0 + (i0 < n-1), w1 = src - i0, w0 = 1 - w1) every destination that has a non-zero
   weight on source index i lies in [2i - 1, 2i + 2], for every n the host lets the kernel take (4..4096).  w1 is taken
   both as a rounded subtract and as the fused multiply-subtract the compiler emits for it.
2. The host's gate (s2s_upsample2x_bwd_family): the 2 x 2 kernel exactly for 4..4096 source pixels per axis with 32-bit
   offsets inside a row, the branching gather below 4, the per-pixel window kernel otherwise and for the _ref entry."""
import numpy as np

GATHER, WINDOW, QUAD = 0, 1, 2


def outside_window(n, fused):
    nu = 2 * n
    scale = np.float32(n - 1) / np.float32(nu - 1)
    dst = np.arange(nu, dtype=np.int64)
    dstf = dst.astype(np.float32)
    src = scale * dstf                                            # fp32 product, rounded
    i0 = np.minimum(src.astype(np.int64), n - 1)
    i1 = i0 + (i0 < n - 1)
    if fused:                                                     # fma(scale, dst, -i0): exact product, one rounding
        w1 = (np.float64(scale) * dst.astype(np.float64) - i0.astype(np.float64)).astype(np.float32)
    else:
        w1 = src - i0.astype(np.float32)
    w0 = np.float32(1) - w1
    bad = 0
    for idx, w in ((i0, w0), (i1, w1)):
        bad += int(np.count_nonzero((w != 0) & ((dst < 2 * idx - 1) | (dst > 2 * idx + 2))))
    return bad


def test_every_nonzero_weight_lies_in_the_4_wide_window():
    broken = [(n, f) for n in range(4, 4097) for f in (False, True) if outside_window(n, f)]
    assert broken == []


def test_host_gate_picks_the_kernel():
    from stain2stain_amd import _native
    fam = _native.lib().s2s_upsample2x_bwd_family

    def f(hin, win, C=8, B=1, lddy=None, lddx=None, pad=0, ref=0):
        return fam(lddy or C, lddx or C, B, hin, win, 2 * hin + pad, 2 * win + pad, C, ref)

    for hin, win in ((4, 4), (5, 7), (33, 17), (128, 128), (4096, 4), (4, 4096)):
        assert f(hin, win) == QUAD and f(hin, win, pad=3) == QUAD
        assert f(hin, win, ref=1) == WINDOW
    assert f(16, 16, C=1024, B=16, lddy=2048) == QUAD             # the benchmark's bottleneck launch
    assert f(3, 5) == GATHER and f(6, 3) == GATHER and f(3, 5, ref=1) == GATHER and f(1, 1) == GATHER
    assert f(4097, 4) == WINDOW and f(4, 4097) == WINDOW          # beyond the proven placement
    assert f(4, 4, C=8, lddy=1 << 28) == WINDOW                   # Wout * lddy = 2^31: no 32-bit offset inside a row
    assert f(4, 4, C=8, lddx=1 << 29) == WINDOW                   # Win * lddx = 2^31
    assert f(4, 4, C=12) < 0 and f(4, 4, lddy=12) < 0             # the launch's own shape errors
    assert fam(8, 8, 1, 4, 4, 7, 8, 8, 0) < 0                     # a crop is not a pad
