"""CPU restatement of stain2stain_amd.augment in numpy.  Nothing here imports the package.

  geometry            crop, the two flips and the transpose by slicing
  stain_matrix, fold  a jitter folded into the 12 numbers of the OD map, in float64
  apply64             the map evaluated in float64 from the fp32 constants; ``unrounded`` is the level before rounding,
                      which decides where a last-bit difference may show
  apply32             the map float32 operation by operation, as the kernel evaluates it
  augment             the whole call: geometry, map, ``white``, for a batch
"""
import numpy as np

from stain_norm_ref import network, od_table32, synthetic_he  # noqa: F401  (re-exported for the tests)

NAMED = {"hdab": [[0.650, 0.704, 0.286], [0.268, 0.570, 0.776]],
         "hed": [[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]]}
LOG2_10 = np.float32(-3.321928094887362)
SYMMETRIES = [(h, v, t) for t in (0, 1) for v in (0, 1) for h in (0, 1)]


def geometry(img, top, left, hflip, vflip, transpose, S):
    """img [H, W, ...] -> [S, S, ...]: crop, ``[::-1]`` if vflip, ``[:, ::-1]`` if hflip, then ``swapaxes(0, 1)``."""
    f = np.asarray(img)[top:top + S, left:left + S]
    if vflip:
        f = f[::-1]
    if hflip:
        f = f[:, ::-1]
    if transpose:
        f = f.swapaxes(0, 1)
    return np.ascontiguousarray(f)


def stain_matrix(stains):
    """float64 [3, 3] with unit rows; a missing third row is the normalised cross product of the first two."""
    m = np.array(NAMED[stains] if isinstance(stains, str) else stains, dtype=np.float64)
    m = m / np.linalg.norm(m, axis=1, keepdims=True)
    if m.shape[0] == 2:
        c = np.cross(m[0], m[1])
        m = np.vstack([m, c / np.linalg.norm(c)])
    return m


def fold(jitter6, stains):
    """(alpha0..2, beta0..2) and a basis -> float64 [12]: A = inv(M) diag(alpha) M row-major, then b = beta M."""
    j = np.asarray(jitter6, dtype=np.float64)
    M = stain_matrix(stains)
    A = np.linalg.inv(M) @ np.diag(j[:3]) @ M
    return np.concatenate([A.reshape(-1), j[3:] @ M])


def apply64(u8, A32, b32):
    """(uint8 [..., 3], unrounded float64 [..., 3]) of od' = od @ A + b, u' = 255 * 10^(-od'), from the fp32 constants."""
    od = od_table32().astype(np.float64)[np.asarray(u8)]
    A = np.asarray(A32, dtype=np.float32).astype(np.float64).reshape(3, 3)
    b = np.asarray(b32, dtype=np.float32).astype(np.float64).reshape(3)
    raw = 255.0 * 10.0 ** (-(od @ A + b))
    return np.clip(np.rint(raw), 0, 255).astype(np.uint8), raw


def apply32(u8, A32, b32):
    """The same in float32, every operation rounded on its own, in the kernel's order; returns (bytes, levels)."""
    od = od_table32()[np.asarray(u8)]
    A = np.asarray(A32, dtype=np.float32).reshape(3, 3)
    b = np.asarray(b32, dtype=np.float32).reshape(3)
    out = []
    for c in range(3):
        d = ((od[..., 0] * A[0, c]) + (od[..., 1] * A[1, c])) + (od[..., 2] * A[2, c])
        o = d + b[c]
        v = np.float32(255.0) * np.exp2(o * LOG2_10)
        assert v.dtype == np.float32
        out.append(v)
    raw = np.stack(out, axis=-1)
    return np.clip(np.rint(raw), 0, 255).astype(np.uint8), raw


def mapped(u8, map12, white=None):
    """(bytes, unrounded) of one image under one 12-number map; pixels with min >= white keep their bytes (and get an
    unrounded level equal to the byte)."""
    m = np.asarray(map12, dtype=np.float32)
    out, raw = apply64(u8, m[:9], m[9:])
    if white is not None:
        keep = np.asarray(u8).min(-1) >= white
        out[keep] = np.asarray(u8)[keep]
        raw[keep] = np.asarray(u8)[keep]
    return out, raw


def augment(imgs, params, S, maps=None, white=None):
    """A batch [B, H, W, 3] (or a mask batch [B, H, W] with maps=None) -> ([B, S, S, ...] bytes, unrounded or None)."""
    outs, raws = [], []
    for n, img in enumerate(imgs):
        p = [int(v) for v in params[n]] + [0]
        f = geometry(img, p[0], p[1], p[2], p[3], p[4], S)
        if maps is None:
            outs.append(f)
        else:
            o, r = mapped(f, maps[n], white)
            outs.append(o)
            raws.append(r)
    return np.stack(outs), (np.stack(raws) if raws else None)


def half_band(raw, width=1e-3):
    """Where the unrounded level lies within ``width`` of a half-integer: the bytes there may differ by one level."""
    frac = raw - np.floor(raw)
    return np.abs(frac - 0.5) <= width
