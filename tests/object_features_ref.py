"""CPU restatement of stain2stain_amd.object_features in numpy and Python integers.  Nothing here imports
the package.

  tables / tables_brute   the integer table of one label image: by np.bincount / np.add.at over the pixels, and again
                          object by object from ``labels == k``
  neighbours              per pixel, how many of the four neighbours carry another label or lie outside the image (shifted
                          comparisons on the label image padded with -1)
  quantise                q = min(rint(max(c, 0) * 1024), 4095) from stain_quant_ref.concentrations32, in float32
  derived_row             the fp64 values of one object in the order include/stain2stain_hip.h spells out: numerators as
                          Python integers, each converted to float once
  exact_row               the same values with mpmath at 60 digits: only there to measure the restatement's own error
"""
import math

import numpy as np

import stain_quant_ref as SQ

FAR = 2 ** 31 - 1
INT_KEYS = ("area", "bbox", "moments", "edges", "boundary", "border")
Q_KEYS = ("sum_q", "sum_q2", "max_q")
DTYPES = {"count": np.int32, "area": np.int64, "bbox": np.int32, "moments": np.int64, "edges": np.int64,
          "boundary": np.int64, "border": np.int32, "max_d2": np.int32, "sum_q": np.int64, "sum_q2": np.int64,
          "max_q": np.int32}
DERIVED = ("centroid_y", "centroid_x", "equivalent_diameter", "mu_yy", "mu_xx", "mu_yx", "major_axis", "minor_axis",
           "eccentricity", "orientation", "compactness", "mean_conc", "std_conc", "max_conc", "inscribed_radius")
EXACT_KEYS = ("centroid_y", "centroid_x", "mu_yy", "mu_xx", "mu_yx", "mean_conc", "max_conc")   # divisions only
FOUR_PI = 12.566370614359172


def neighbours(labels):
    """int64 [H, W]: the 4-neighbours with another label or outside the image."""
    lab = np.asarray(labels).astype(np.int64)
    p = np.pad(lab, 1, constant_values=-1)
    c = p[1:-1, 1:-1]
    return ((p[:-2, 1:-1] != c).astype(np.int64) + (p[2:, 1:-1] != c) + (p[1:-1, :-2] != c) + (p[1:-1, 2:] != c))


def quantise(u8, m32, stain):
    """uint8 [..., 3] -> int64 [...]: the quantised concentration of one stain."""
    c = SQ.concentrations32(u8, m32)[..., stain]
    q = np.rint(np.maximum(c, np.float32(0)) * np.float32(1024))
    assert q.dtype == np.float32
    return np.minimum(q.astype(np.int64), 4095)


def tables(labels, M, d2=None, q=None):
    """The integer table of one 2-D label image: arrays [M, ...]; rows at or beyond min(count, M) are zero."""
    lab = np.asarray(labels).astype(np.int64)
    H, W = lab.shape
    count = int(lab.max()) if lab.size else 0
    out = {"count": np.int32(count), "area": np.zeros(M, np.int64), "bbox": np.zeros((M, 4), np.int32),
           "moments": np.zeros((M, 5), np.int64), "edges": np.zeros(M, np.int64), "boundary": np.zeros(M, np.int64),
           "border": np.zeros(M, np.int32)}
    if d2 is not None:
        out["max_d2"] = np.zeros(M, np.int32)
    if q is not None:
        out.update(sum_q=np.zeros(M, np.int64), sum_q2=np.zeros(M, np.int64), max_q=np.zeros(M, np.int32))
    ys, xs = np.nonzero((lab > 0) & (lab <= M))
    if ys.size == 0:
        return out
    k = lab[ys, xs] - 1
    e = neighbours(lab)[ys, xs]
    ys64, xs64 = ys.astype(np.int64), xs.astype(np.int64)
    area = np.bincount(k, minlength=M)[:M].astype(np.int64)
    out["area"][:] = area

    def isum(v):
        s = np.zeros(M, np.int64)
        np.add.at(s, k, v)
        return s

    out["moments"][:] = np.stack([isum(ys64), isum(xs64), isum(ys64 * ys64), isum(xs64 * xs64), isum(ys64 * xs64)], axis=1)
    out["edges"][:] = isum(e)
    out["boundary"][:] = isum((e > 0).astype(np.int64))
    big = np.iinfo(np.int32).max
    y0, x0 = np.full(M, big, np.int64), np.full(M, big, np.int64)
    y1, x1 = np.zeros(M, np.int64), np.zeros(M, np.int64)
    np.minimum.at(y0, k, ys64)
    np.minimum.at(x0, k, xs64)
    np.maximum.at(y1, k, ys64 + 1)
    np.maximum.at(x1, k, xs64 + 1)
    have = area > 0
    out["bbox"][have] = np.stack([y0, x0, y1, x1], axis=1)[have]
    edge = np.zeros(M, np.int64)
    np.maximum.at(edge, k, ((ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)).astype(np.int64))
    out["border"][:] = edge
    if d2 is not None:
        m = np.zeros(M, np.int64)
        np.maximum.at(m, k, np.asarray(d2).astype(np.int64)[ys, xs])
        out["max_d2"][:] = m
    if q is not None:
        qv = np.asarray(q).astype(np.int64)[ys, xs]
        out["sum_q"][:] = isum(qv)
        out["sum_q2"][:] = isum(qv * qv)
        m = np.zeros(M, np.int64)
        np.maximum.at(m, k, qv)
        out["max_q"][:] = m
    return out


def tables_brute(labels, M, d2=None, q=None):
    """``tables`` object by object from ``labels == k``."""
    lab = np.asarray(labels).astype(np.int64)
    H, W = lab.shape
    out = tables(np.zeros((1, 1), np.int64), M, d2 if d2 is None else np.zeros((1, 1)), q if q is None else np.zeros((1, 1)))
    out["count"] = np.int32(lab.max())
    p = np.pad(lab, 1, constant_values=-1)
    for k in range(1, min(int(lab.max()), M) + 1):
        m = lab == k
        if not m.any():
            continue
        ys, xs = np.nonzero(m)
        r = k - 1
        out["area"][r] = ys.size
        out["bbox"][r] = (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1)
        out["moments"][r] = (int(ys.sum()), int(xs.sum()), int((ys.astype(np.int64) ** 2).sum()),
                             int((xs.astype(np.int64) ** 2).sum()), int((ys.astype(np.int64) * xs).sum()))
        e = np.zeros(ys.size, np.int64)
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            e += p[ys + 1 + dy, xs + 1 + dx] != k
        out["edges"][r] = e.sum()
        out["boundary"][r] = (e > 0).sum()
        out["border"][r] = int(ys.min() == 0 or xs.min() == 0 or ys.max() == H - 1 or xs.max() == W - 1)
        if d2 is not None:
            out["max_d2"][r] = np.asarray(d2)[m].max()
        if q is not None:
            qv = np.asarray(q).astype(np.int64)[m]
            out["sum_q"][r], out["sum_q2"][r], out["max_q"][r] = qv.sum(), (qv * qv).sum(), qv.max()
    return out


def batch(labels, M, d2=None, q=None):
    per = [tables(l, M, None if d2 is None else d2[n], None if q is None else q[n]) for n, l in enumerate(labels)]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


# ---- derived values ----------------------------------------------------------------------------------------------------
def numerators(A, sy, sx, syy, sxx, syx):
    """The exact integer numerators of mu_yy, mu_xx, mu_yx (times A^2)."""
    return A * syy - sy * sy, A * sxx - sx * sx, A * syx - sy * sx


def derived_row(A, sy, sx, syy, sxx, syx, E, sq=None, sq2=None, mq=None, md2=None):
    """dict of Python floats, in the documented order of operations; everything 0 for an empty row."""
    A, sy, sx, syy, sxx, syx, E = (int(v) for v in (A, sy, sx, syy, sxx, syx, E))
    out = dict.fromkeys(DERIVED, 0.0)
    if A <= 0:
        return out
    Ad = float(A)
    A2 = Ad * Ad
    out["centroid_y"], out["centroid_x"] = float(sy) / Ad, float(sx) / Ad
    out["equivalent_diameter"] = math.sqrt((4.0 * Ad) / math.pi)
    nyy, nxx, nyx = numerators(A, sy, sx, syy, sxx, syx)
    myy, mxx, myx = float(nyy) / A2, float(nxx) / A2, float(nyx) / A2
    out["mu_yy"], out["mu_xx"], out["mu_yx"] = myy, mxx, myx
    t, d = mxx + myy, mxx - myy
    root = math.sqrt(d * d + 4.0 * (myx * myx))
    l1, l2 = max(0.5 * (t + root), 0.0), max(0.5 * (t - root), 0.0)
    out["l1"], out["l2"] = l1, l2
    out["major_axis"], out["minor_axis"] = 4.0 * math.sqrt(l1), 4.0 * math.sqrt(l2)
    out["eccentricity"] = math.sqrt(max(1.0 - l2 / l1, 0.0)) if l1 > 0.0 else 0.0
    twice = 2.0 * myx
    out["orientation"] = 0.0 if (twice == 0.0 and d == 0.0) else 0.5 * math.atan2(twice, d)
    Ed = float(E)
    out["compactness"] = (FOUR_PI * Ad) / (Ed * Ed)
    if sq is not None:
        sq, sq2, mq = int(sq), int(sq2), int(mq)
        out["mean_conc"] = (float(sq) / Ad) / 1024.0
        out["std_conc"] = math.sqrt(max(float(A * sq2 - sq * sq) / A2, 0.0)) / 1024.0
        out["max_conc"] = float(mq) / 1024.0
    if md2 is not None:
        out["inscribed_radius"] = math.inf if int(md2) == FAR else math.sqrt(float(int(md2)))
    return out


def exact_row(A, sy, sx, syy, sxx, syx, E, sq=None, sq2=None, mq=None, md2=None):
    """The same values as mpmath numbers at 60 digits (no float64 anywhere)."""
    import mpmath as mp
    A, sy, sx, syy, sxx, syx, E = (int(v) for v in (A, sy, sx, syy, sxx, syx, E))
    out = dict.fromkeys(DERIVED, mp.mpf(0))
    if A <= 0:
        return out
    with mp.workdps(60):
        a = mp.mpf(A)
        out["centroid_y"], out["centroid_x"] = mp.mpf(sy) / a, mp.mpf(sx) / a
        out["equivalent_diameter"] = mp.sqrt(4 * a / mp.pi)
        nyy, nxx, nyx = numerators(A, sy, sx, syy, sxx, syx)
        myy, mxx, myx = mp.mpf(nyy) / (a * a), mp.mpf(nxx) / (a * a), mp.mpf(nyx) / (a * a)
        out["mu_yy"], out["mu_xx"], out["mu_yx"] = myy, mxx, myx
        t, d = mxx + myy, mxx - myy
        root = mp.sqrt(d * d + 4 * myx * myx)
        l1, l2 = max((t + root) / 2, mp.mpf(0)), max((t - root) / 2, mp.mpf(0))
        out["l1"], out["l2"] = l1, l2
        out["major_axis"], out["minor_axis"] = 4 * mp.sqrt(l1), 4 * mp.sqrt(l2)
        out["eccentricity"] = mp.sqrt(max(1 - l2 / l1, mp.mpf(0))) if l1 > 0 else mp.mpf(0)
        out["orientation"] = mp.mpf(0) if (nyx == 0 and nxx == nyy) else mp.atan2(2 * myx, d) / 2
        out["compactness"] = 4 * mp.pi * a / (mp.mpf(E) * mp.mpf(E))
        if sq is not None:
            sq, sq2, mq = int(sq), int(sq2), int(mq)
            out["mean_conc"] = mp.mpf(sq) / a / 1024
            out["std_conc"] = mp.sqrt(mp.mpf(A * sq2 - sq * sq) / (a * a)) / 1024
            out["max_conc"] = mp.mpf(mq) / 1024
        if md2 is not None:
            out["inscribed_radius"] = mp.inf if int(md2) == FAR else mp.sqrt(mp.mpf(int(md2)))
    return out


def row_args(t, r):
    """The arguments of derived_row / exact_row for row r of a table of one sample."""
    a = [t["area"][r], *t["moments"][r], t["edges"][r]]
    kw = {}
    if "sum_q" in t:
        kw.update(sq=t["sum_q"][r], sq2=t["sum_q2"][r], mq=t["max_q"][r])
    if "max_d2" in t:
        kw["md2"] = t["max_d2"][r]
    return a, kw


def derived(t):
    """float64 arrays [M] (plus l1, l2) of one sample's table; rows at or beyond min(count, M) are zero."""
    M = t["area"].shape[0]
    n = min(int(t["count"]), M)
    out = {k: np.zeros(M, np.float64) for k in DERIVED + ("l1", "l2")}
    for r in range(n):
        a, kw = row_args(t, r)
        for k, v in derived_row(*a, **kw).items():
            out[k][r] = v
    return out


def isotropic(l1, l2):
    """Where the orientation is not compared: a multi-pixel object whose two eigenvalues agree to 1e-9 (an object with
    l1 == 0 is a single pixel, whose orientation is 0 by definition and IS compared)."""
    return (l1 > 0) & (l1 - l2 <= 1e-9 * l1)


def restatement_errors(t):
    """Per quantity the largest error of ``derived_row`` against ``exact_row`` over the rows of one table: axis lengths
    in ulp(major_axis), equivalent_diameter / std_conc / inscribed_radius in their own ulp, eccentricity, orientation
    and compactness absolutely.  Orientation skips ``isotropic`` rows."""
    import mpmath as mp
    worst = dict.fromkeys(("major_axis", "minor_axis", "equivalent_diameter", "std_conc", "inscribed_radius",
                           "eccentricity", "orientation", "compactness"), 0.0)
    n = min(int(t["count"]), t["area"].shape[0])
    for r in range(n):
        a, kw = row_args(t, r)
        if int(a[0]) <= 0:
            continue
        f, x = derived_row(*a, **kw), exact_row(*a, **kw)
        with mp.workdps(60):
            err = lambda k: float(abs(mp.mpf(f[k]) - x[k])) if math.isfinite(f[k]) else 0.0
            ulp_major = float(np.spacing(f["major_axis"])) if f["major_axis"] > 0 else float(np.spacing(1.0))
            for k in ("major_axis", "minor_axis"):
                worst[k] = max(worst[k], err(k) / ulp_major)
            for k in ("equivalent_diameter", "std_conc", "inscribed_radius"):
                if f[k] > 0 and math.isfinite(f[k]):
                    worst[k] = max(worst[k], err(k) / float(np.spacing(f[k])))
            for k in ("eccentricity", "compactness"):
                worst[k] = max(worst[k], err(k))
            if not isotropic(np.float64(f["l1"]), np.float64(f["l2"])):
                worst["orientation"] = max(worst["orientation"], err("orientation"))
    return worst


# ---- analytic sums over a rectangle (no array) ---------------------------------------------------------------------------
def rectangle_sums(y0, x0, a, b):
    """(A, sum y, sum x, sum y^2, sum x^2, sum yx) of the a x b rectangle with top-left pixel (y0, x0), as Python ints."""
    s1 = lambda lo, n: n * lo + n * (n - 1) // 2
    s2 = lambda lo, n: sum_sq(lo + n - 1) - sum_sq(lo - 1)
    return a * b, b * s1(y0, a), a * s1(x0, b), b * s2(y0, a), a * s2(x0, b), s1(y0, a) * s1(x0, b)


def sum_sq(n):
    return n * (n + 1) * (2 * n + 1) // 6 if n >= 0 else 0
