"""Host model of the per-sample Dormand-Prince 5(4) kernels (csrc/ode.hip): plain Python and numpy.

Every function restates the contract of one kernel; ``solve`` strings them together into a complete per-sample solver so
that the model itself can be checked on the CPU against the batch-wide ``dopri5_integrate`` at batch 1
(tests/test_dopri5_ref_cpu.py) before the kernels are checked against the model (tests/test_dopri5_kernels_gpu.py).

The tableau is typed here from Dormand & Prince (1980) / Hairer, Norsett, Wanner II.5 and deliberately NOT imported from
the package.  State row per sample (include/stain2stain_hip.h): ``t, h, accepted, rejected, rejected-flag, done, accept,
aux``; status word of the batch: ``active, limit, attempts, 0``."""
import math

import numpy as np

T, H, ACC, REJ, REJECTED, DONE, ACCEPT, AUX = range(8)

# nodes c_i, stage rows a_ij (row 6 = the 5th-order weights b_j: first same as last), 4th-order weights b*_j
C = (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0)
A = ((),
     (1 / 5,),
     (3 / 40, 9 / 40),
     (44 / 45, -56 / 15, 32 / 9),
     (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
     (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656),
     (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84))
B5 = A[6] + (0.0,)
# error weights b*_j - b_j, as DESIGN.md 3.12 / scipy's RK45 tabulate them (test_dopri5_ref_cpu.py re-derives them
# from the 4th-order weights in exact rationals)
E = (-71 / 57600, 0.0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40)
PROBE_NODE = 1.0                      # the initial-step probe y + h0 k1 is evaluated at t + 1.0 * h0

LIMIT_MESSAGE = "dopri5_generate: max_steps reached before t = 1"


def node_time(t, c, h):
    """The time the network sees at a stage: ``t + c * h`` in double (two roundings), rounded to fp32 once."""
    return np.float32(float(t) + float(c) * float(h))


def stage_coeffs(i, h):
    """The fp32 coefficients of stage row ``i`` (0 = the probe): each ``h * a_ij`` formed in double, rounded once."""
    if i == 0:
        return [np.float32(float(h))]
    return [np.float32(float(h) * a) for a in A[i]]


def _terms(coeffs, weights):
    return [(j, float(c)) for j, (c, w) in enumerate(zip(coeffs, weights)) if w != 0.0]


def stage64(i, y, ks, h, frozen):
    """``y + sum_j c_j k_j`` in float64 with the fp32 coefficients of ``stage_coeffs``; zero a_ij are left out (so a
    non-finite k_j under a zero weight does not count); a frozen sample's stage input is ``y`` whatever the k_j hold."""
    out = np.asarray(y, dtype=np.float64).copy()
    if frozen:
        return out
    for j, c in _terms(stage_coeffs(i, h), (1.0,) if i == 0 else A[i]):
        out += c * np.asarray(ks[j], dtype=np.float64)
    return out


def stage_bound(i, y, ks, h, frozen):
    """Rounding of the kernel's chain against ``stage64``, per element: NJ fp32 fmas, each rounding an intermediate of
    magnitude <= |y| + sum_j |c_j k_j| to 2**-24 relative, plus one more unit for the second-order terms and the store:
    ``(NJ + 1) * 2**-24 * (|y| + sum_j |c_j k_j|)``; 0 for a frozen sample (its output is ``y`` itself)."""
    mag = np.abs(np.asarray(y, dtype=np.float64))
    if frozen:
        return np.zeros_like(mag)
    weights = (1.0,) if i == 0 else A[i]
    for j, c in _terms(stage_coeffs(i, h), weights):
        mag += np.abs(c * np.asarray(ks[j], dtype=np.float64))
    return (len(weights) + 1) * 2.0 ** -24 * mag


def error_coeffs(h):
    return [np.float32(float(h) * e) for e in E]


def error64(ks, h):
    """The error estimate ``sum_j (float)(h e_j) k_j`` in float64, zero e_j left out (k2 may be None)."""
    terms = _terms(error_coeffs(h), E)
    out = np.zeros(np.asarray(ks[terms[0][0]]).shape, dtype=np.float64)
    for j, c in terms:
        out += c * np.asarray(ks[j], dtype=np.float64)
    return out


def scaled_square_sum(e, y0, y1, atol, rtol):
    """``sum((e / (atol + rtol max(|y0|, |y1|)))^2)``: the scale and the quotient in fp32 (each operation rounded, no
    contraction), the squares and their sum in float64."""
    e, y0, y1 = (np.asarray(a, dtype=np.float32) for a in (e, y0, y1))
    sc = np.float32(atol) + np.float32(rtol) * np.maximum(np.abs(y0), np.abs(y1))
    r = (e / sc).astype(np.float32)
    return float(np.sum(r.astype(np.float64) ** 2))


def rms_f32(total, n):
    """``sqrt(mean)`` rounded to fp32, as ``s2s_ode_error_norm`` hands the batch-wide solver its norm."""
    return float(np.float32(math.sqrt(float(total) * (1.0 / n))))


def init_h0(d0, d1):
    """Hairer, Norsett, Wanner II.4, first guess."""
    return 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1


def init_h(h0, d1, d2):
    """The first step: ``d2`` is the norm of ``f(t + h0, y + h0 k1) - k1`` divided by ``h0``; the interval is [0, 1]."""
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = math.pow(0.01 / max(d1, d2), 1.0 / 5.0)
    return min(100 * h0, h1, 1.0 - 0.0)


def init_h_is_exact(h0, d1, d2):
    """True where ``init_h`` returns a value no ``pow`` went into (a cap binds or the 1e-15 branch was taken)."""
    if d1 <= 1e-15 and d2 <= 1e-15:
        return True
    return init_h(h0, d1, d2) != math.pow(0.01 / max(d1, d2), 1.0 / 5.0)


def control(row, en):
    """One pass of the step controller over one state row (the part that does not depend on ``max_steps``): accept when
    ``en < 1``, factor ``0.9 en^(-1/5)`` clamped to [0.2, 10] (10 when ``en == 0``), no growth right after a rejection,
    ``t >= 1`` freezes the row, else ``h = min(h, 1 - t)``.  A frozen row only has its accept flag cleared."""
    row = [float(v) for v in row]
    if row[DONE] != 0.0:
        row[ACCEPT] = 0.0
        return row
    t, h = row[T], row[H]
    if en < 1.0:
        factor = 10.0 if en == 0.0 else min(10.0, 0.9 * math.pow(en, -0.2))
        if row[REJECTED] != 0.0:
            factor = min(1.0, factor)
        t = t + h
        h = h * factor
        row[REJECTED] = 0.0
        row[ACC] += 1.0
        row[ACCEPT] = 1.0
    else:
        h = h * max(0.2, 0.9 * math.pow(en, -0.2))
        row[REJECTED] = 1.0
        row[REJ] += 1.0
        row[ACCEPT] = 0.0
    if t >= 1.0:
        row[DONE] = 1.0
        h = 0.0
    else:
        h = min(h, 1.0 - t)
    row[T], row[H], row[AUX] = t, h, float(en)
    return row


def control_h_is_exact(row, en):
    """True where the new ``h`` of ``control`` does not depend on the value of ``pow``: a clamp binds (factor 10, the
    0.2 floor, the cap to 1 after a rejection, ``1 - t``) or the row is or becomes frozen."""
    if row[DONE] != 0.0 or en == 0.0 or not (en == en):
        return True
    new = control(row, en)
    if new[DONE] != 0.0 or new[H] == 1.0 - new[T]:
        return True
    raw = 0.9 * math.pow(en, -0.2)
    if en < 1.0:
        return raw >= 10.0 or (row[REJECTED] != 0.0 and raw >= 1.0)
    return raw <= 0.2


def status_after(rows, attempts_before, max_steps):
    """The status word once ``control`` has run over every row: samples still active, limit reached (as soon as
    ``max_steps`` attempts have run, like the batch-wide loop's ``for ... else``), attempts so far, 0."""
    attempts = int(attempts_before) + 1
    active = sum(1 for r in rows if r[DONE] == 0.0)
    return (active, 1 if attempts >= max_steps else 0, attempts, 0)


def ulp_distance(a, b):
    """|a - b| in units of the fp64 spacing at ``b``."""
    if a == b:
        return 0.0
    return abs(a - b) / float(np.spacing(abs(b)))


def solve(f, y0, atol=1e-4, rtol=1e-4, max_steps=1000):
    """The model as a complete solver of one sample: ``f(t: np.float32, y: float32 array) -> float32 array``.  Returns
    ``(y(1), final state row, evaluations)``; raises the solvers' RuntimeError when ``max_steps`` attempts have run."""
    if max_steps < 1:
        raise RuntimeError(LIMIT_MESSAGE)
    y = np.asarray(y0, dtype=np.float32).copy()
    n = y.size
    evals = [0]

    def ev(t, x):
        evals[0] += 1
        return np.asarray(f(t, x), dtype=np.float32)

    norm = lambda e, a, b: rms_f32(scaled_square_sum(e, a, b, atol, rtol), n)
    k1 = ev(np.float32(0.0), y)
    d0, d1 = norm(y, y, y), norm(k1, y, y)
    h0 = init_h0(d0, d1)
    probe = stage64(0, y, [k1], h0, False).astype(np.float32)
    fa = ev(node_time(0.0, PROBE_NODE, h0), probe)
    d2 = norm(fa - k1, y, y) / h0
    row = [0.0, init_h(h0, d1, d2), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    attempts = 0
    while True:
        ks = [k1]
        for i in range(1, 7):
            yi = stage64(i, y, ks, row[H], False).astype(np.float32)
            ks.append(ev(node_time(row[T], C[i], row[H]), yi))
        y_new = yi
        en = norm(error64(ks, row[H]).astype(np.float32), y, y_new)
        row = control(row, en)
        if row[ACCEPT] != 0.0:
            y, k1 = y_new, ks[6]
        active, limit, attempts, _ = status_after([row], attempts, max_steps)
        if limit:
            raise RuntimeError(LIMIT_MESSAGE)
        if active == 0:
            return y, row, evals[0]


# Analytic velocity fields ``f(xp, t, x)`` for one or more samples (``t`` broadcasts against ``x``; ``xp`` is the array
# module, torch in the tests), with the counts the issue recorded for them on a 2.0 + rand(1, 3, 4, 4) source at 1e-4.
FIELDS = {
    "zero": lambda xp, t, x: xp.zeros_like(x),
    "one": lambda xp, t, x: xp.ones_like(x),
    "relax_slow": lambda xp, t, x: -0.5 * (x - xp.cos(t)),
    "relax_fast": lambda xp, t, x: -25.0 * (x - xp.cos(2.0 * t)),
    "decay": lambda xp, t, x: -40.0 * x,
    "osc": lambda xp, t, x: xp.zeros_like(x) + 30.0 * xp.cos(30.0 * t),
    "nan": lambda xp, t, x: xp.full_like(x, float("nan")),
}
# (field, zero source?) in the issue's order; the last is ``v = 1`` from a zero source
CASES = (("zero", False), ("one", False), ("relax_slow", False), ("relax_fast", False), ("decay", False),
         ("osc", False), ("one", True))
REJECTING = ("relax_fast", "decay", "osc")
