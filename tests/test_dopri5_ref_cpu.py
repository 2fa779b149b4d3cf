"""The host model of the per-sample Dormand-Prince kernels (tests/dopri5_ref.py) is itself right: driven as a complete
per-sample solver on numpy arrays it takes the steps of the batch-wide ``dopri5_integrate`` at batch 1 (whose two HIP
ops are replaced by their torch one-liners, as tests/test_modules_cpu.py does), its tableau satisfies the order
conditions, and the step limit and a non-finite field end both solvers the same way.  No GPU."""
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

import dopri5_ref as R

ATOL = RTOL = 1e-4


def source(zero=False):
    g = torch.Generator().manual_seed(3)
    x = 2.0 + torch.rand(1, 3, 4, 4, generator=g)
    return torch.zeros_like(x) if zero else x


def torch_field(name, calls=None):
    """``f(t[B], x)`` as the solvers call it."""
    def f(t, x):
        if calls is not None:
            calls.append(float(t[0]))
        return R.FIELDS[name](torch, t.view(-1, 1, 1, 1), x).contiguous()
    return f


def model_field(name, calls=None):
    """The same field for the model: one sample, ``t`` an fp32 scalar, numpy in and out."""
    f = torch_field(name, calls)
    return lambda t, y: f(torch.full((1,), float(t), dtype=torch.float32), torch.from_numpy(y).clone()[None])[0].numpy()


@pytest.fixture
def cpu_ops(monkeypatch):
    from stain2stain_amd import ops
    monkeypatch.setattr(ops, "axpy_", lambda x, y, a: x.add_(y, alpha=a))
    monkeypatch.setattr(ops, "ode_error_norm", lambda e, a, b, atol, rtol: torch.sqrt(torch.mean(
        (e / (atol + rtol * torch.maximum(a.abs(), b.abs()))) ** 2)).reshape(1))


def test_tableau_satisfies_the_order_conditions():
    """Exact rationals typed a second time: row sums = nodes, the 5th-order weights integrate t^k exactly for k < 5, the
    4th-order ones for k < 4, and the error weights are their difference."""
    c = [Fr(0), Fr(1, 5), Fr(3, 10), Fr(4, 5), Fr(8, 9), Fr(1), Fr(1)]
    a = [[], [Fr(1, 5)], [Fr(3, 40), Fr(9, 40)], [Fr(44, 45), Fr(-56, 15), Fr(32, 9)],
         [Fr(19372, 6561), Fr(-25360, 2187), Fr(64448, 6561), Fr(-212, 729)],
         [Fr(9017, 3168), Fr(-355, 33), Fr(46732, 5247), Fr(49, 176), Fr(-5103, 18656)],
         [Fr(35, 384), Fr(0), Fr(500, 1113), Fr(125, 192), Fr(-2187, 6784), Fr(11, 84)]]
    b4 = [Fr(5179, 57600), Fr(0), Fr(7571, 16695), Fr(393, 640), Fr(-92097, 339200), Fr(187, 2100), Fr(1, 40)]
    b5 = a[6] + [Fr(0)]
    for i in range(7):
        assert sum(a[i], Fr(0)) == c[i]
        assert [float(v) for v in a[i]] == list(R.A[i]) and float(c[i]) == R.C[i]
    for k in range(5):
        assert sum(w * ci ** k for w, ci in zip(b5, c)) == Fr(1, k + 1)
    for k in range(4):
        assert sum(w * ci ** k for w, ci in zip(b4, c)) == Fr(1, k + 1)
    # the first condition that separates order 5 from order 4 must fail for the embedded weights
    assert sum(w * ci ** 4 for w, ci in zip(b4, c)) != Fr(1, 5)
    assert [float(x - y) for x, y in zip(b4, b5)] == list(R.E)


def test_scalar_pieces():
    assert R.node_time(0.25, 0.2, 0.05) == np.float32(0.25 + 0.2 * 0.05)
    assert R.stage_coeffs(0, 0.3) == [np.float32(0.3)] and len(R.stage_coeffs(5, 0.3)) == 5
    assert R.rms_f32(48.0, 48) == 1.0 and R.rms_f32(0.0, 48) == 0.0
    assert R.init_h0(0.0, 3.0) == 1e-6 and R.init_h0(3.0, 0.0) == 1e-6 and R.init_h0(2.0, 4.0) == 0.01 * 2.0 / 4.0
    assert R.init_h(1e-6, 0.0, 0.0) == 1e-6 and R.init_h(1.0, 1e-3, 1e-4) == 1.0 and R.init_h(1e-6, 0.0, 1e9) == 100 * 1e-6
    row = [0.5, 0.25, 2.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    got = R.control(row, 1e-9)                              # accepted right after a rejection: no growth
    assert got == [0.75, 0.25, 3.0, 1.0, 0.0, 0.0, 1.0, 1e-9]
    got = R.control(row, float("nan"))                      # a non-finite norm rejects with the 0.2 floor
    assert got[:7] == [0.5, 0.25 * 0.2, 2.0, 2.0, 1.0, 0.0, 0.0] and np.isnan(got[7])
    got = R.control([0.75, 0.25, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], 0.0)
    assert got == [1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0]  # reaching t = 1 freezes the row
    assert R.control(got, 5.0) == got[:6] + [0.0, 0.0]      # a frozen row only loses its accept flag
    assert R.status_after([got, row], 6, 8) == (1, 0, 7, 0) and R.status_after([got, row], 6, 7) == (1, 1, 7, 0)


@pytest.mark.parametrize("name,zero", R.CASES)
def test_model_takes_the_steps_of_the_batch_wide_solver(cpu_ops, name, zero):
    from stain2stain_amd import dopri5_integrate
    x0 = source(zero)
    want, st = dopri5_integrate(torch_field(name), x0.clone(), ATOL, RTOL, return_stats=True)
    y, row, evals = R.solve(model_field(name), x0[0].numpy(), ATOL, RTOL)
    counts = (int(row[R.ACC]), int(row[R.REJ]))
    print(f"{name} (zero source: {zero}): accepted / rejected {counts}, batch-wide {st}")
    assert counts == (st["accepted"], st["rejected"]), (name, counts, st)
    assert evals == 2 + 6 * sum(counts) and row[R.T] >= 1.0 and row[R.DONE] == 1.0 and row[R.H] == 0.0
    # same steps, so the two differ by rounding alone: the model rounds each stage once from float64, the batch-wide
    # chain once per term; at most 6 roundings of 2**-24 per stage input, amplified by |h df/dy| <= 8 (every step of
    # these fields keeps h * lambda inside the scheme's stability interval, |h lambda| < 3.4) over <= 24 attempted steps;
    # relative to the largest magnitude along the trajectory (its ends: the fields relax or add at most 1)
    err = float((torch.from_numpy(y) - want[0]).abs().max() / max(float(x0.abs().max()), float(want.abs().max())))
    print(f"{name}: model vs batch-wide rel err {err:.3e}")
    assert err <= 24 * 8 * 6 * 2.0 ** -24, (name, err)
    if name in R.REJECTING:
        assert counts[1] >= 1, (name, counts)               # the GPU tests rely on these fields rejecting
    if name == "zero":
        assert counts == (7, 0) and np.array_equal(y, x0[0].numpy())


@pytest.mark.parametrize("solver", ["model", "batch-wide"])
def test_step_limit_on_the_zero_field(cpu_ops, solver):
    """The zero field needs 7 attempts (h = 1e-6 growing tenfold); the limit fires as soon as ``max_steps`` attempts have
    run, also when the last allowed one reaches t = 1."""
    from stain2stain_amd import dopri5_integrate
    x0 = source()
    if solver == "model":
        run = lambda m: torch.from_numpy(R.solve(model_field("zero"), x0[0].numpy(), ATOL, RTOL, m)[0])[None]
    else:
        run = lambda m: dopri5_integrate(torch_field("zero"), x0.clone(), ATOL, RTOL, m)
    with pytest.raises(RuntimeError, match="max_steps"):
        run(7)
    assert torch.equal(run(8), x0)


@pytest.mark.parametrize("solver", ["model", "batch-wide"])
def test_nan_field_runs_into_the_limit_after_38_evaluations(cpu_ops, solver):
    from stain2stain_amd import dopri5_integrate
    x0, calls = source(), []
    with pytest.raises(RuntimeError, match="max_steps"):
        if solver == "model":
            R.solve(model_field("nan", calls), x0[0].numpy(), ATOL, RTOL, 6)
        else:
            dopri5_integrate(torch_field("nan", calls), x0.clone(), ATOL, RTOL, 6)
    assert len(calls) == 2 + 6 * 6
