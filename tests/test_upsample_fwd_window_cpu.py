"""What the register-window up-sampling forward (resample.hip, upsample2x_fwd_win_kernel) rests on, without a GPU.

1. The window.  With the kernels' fp32 index arithmetic (ac_axis: scale = (n-1)/(2n-1), src = scale * dst,
   i0 = min((int)src, n-1), i1 = i0 + (i0 < n-1), w1 = src - i0, w0 = 1 - w1) outputs 2a and 2a + 1 of an axis read only
   source indices in [a - 1, a + 1]: i0 is a - 1 or a, and i1 <= a + 1, for every n = 1 .. 4096.  The axis is evaluated
   both with w1 as a rounded subtract and as the fused multiply-subtract the compiler may emit for it; the indices, which
   are all the kernel's choice of rows looks at, do not depend on that choice.
2. The kernel's usual row pair (row 2a mixes source rows (a - 1, a), row 2a + 1 rows (a, a + 1)) holds for every pair
   but the first and the last of a map, so the pairs that reload their rows are two per map.  This one is about speed
   only: the kernel tests every pair and a pair that fails the test loads the rows its taps name.
3. The host's gate (s2s_upsample2x_fwd_family): the register-window kernel for 2 .. 4096 source pixels per axis whose
   rows fit 32-bit byte offsets, the row-sweep kernel otherwise and for the _ref entry."""
import numpy as np

ROWS, WINDOW = 0, 1


def axis(n, fused):
    nu = 2 * n
    scale = np.float32(n - 1) / np.float32(nu - 1)
    dst = np.arange(nu, dtype=np.int64)
    src = scale * dst.astype(np.float32)                          # fp32 product, rounded
    i0 = np.minimum(src.astype(np.int64), n - 1)
    i1 = i0 + (i0 < n - 1)
    if fused:                                                     # fma(scale, dst, -i0): exact product, one rounding
        w1 = (np.float64(scale) * dst.astype(np.float64) - i0.astype(np.float64)).astype(np.float32)
    else:
        w1 = src - i0.astype(np.float32)
    w0 = np.float32(1) - w1
    return dst, i0, i1, w0, w1


def test_outputs_2a_and_2a_plus_1_read_rows_a_minus_1_to_a_plus_1():
    broken = []
    for n in range(1, 4097):
        for fused in (False, True):
            dst, i0, i1, w0, w1 = axis(n, fused)
            a = dst // 2
            ok = ((i0 == a - 1) | (i0 == a)) & (i0 >= 0) & (i1 <= a + 1) & (i1 <= n - 1) & (i1 >= i0)
            if not fused:                                         # the fused form may round a hair below 0; the kernels share it
                ok &= (w1 >= 0) & (w1 <= 1) & (w0 >= 0) & (w0 <= 1)
            if not ok.all():
                broken.append((n, fused))
    assert broken == []


def test_only_the_first_and_last_pair_leave_the_usual_pattern():
    for n in range(2, 4097):
        dst, i0, i1, _, _ = axis(n, False)
        a = np.arange(n)
        usual = (i0[0::2] == a - 1) & (i1[0::2] == a) & (i0[1::2] == a) & (i1[1::2] == a + 1)
        odd = np.flatnonzero(~usual)
        assert set(odd.tolist()) <= {0, n - 1}, (n, odd)


def test_host_gate_picks_the_kernel():
    from stain2stain_amd import _native
    fam = _native.lib().s2s_upsample2x_fwd_family

    def f(hin, win, C=8, B=1, ldx=None, ldy=None, pad=0, ref=0):
        return fam(ldx or C, ldy or C, B, hin, win, 2 * hin + pad, 2 * win + pad, C, ref)

    for hin, win in ((2, 2), (2, 3), (4, 4), (5, 7), (33, 18), (128, 128), (4096, 2), (2, 4096)):
        assert f(hin, win) == WINDOW and f(hin, win, pad=3) == WINDOW
        assert f(hin, win, ref=1) == ROWS
    for C, hin in ((128, 128), (256, 64), (512, 32), (1024, 16)):  # the benchmark's four launches (concat buffers)
        assert f(hin, hin, C=C, B=16, ldy=2 * C) == WINDOW
    assert f(1, 1) == ROWS and f(1, 5) == ROWS and f(6, 1) == ROWS  # a one-pixel axis keeps the row sweep
    assert f(4097, 4) == ROWS and f(4, 4097) == ROWS               # beyond the proven window
    assert f(4, 4, ldx=1 << 27) == ROWS                            # Win * ldx = 2^29 elements: no 32-bit byte offset
    assert f(4, 4, ldy=1 << 26) == ROWS                            # Wout * ldy = 2^29
    assert f(4, 4, ldx=(1 << 27) - 8) == WINDOW
    assert f(4, 4, C=12) < 0 and f(4, 4, ldx=12) < 0 and f(4, 4, ldy=12) < 0   # the launch's own shape errors
    assert fam(8, 8, 1, 4, 4, 7, 8, 8, 0) < 0                      # a crop is not a pad
