"""Fixed-step Runge-Kutta samplers (stain2stain_amd.flow_matching), the parts that need no GPU: the
tableaus satisfy the order conditions of their stated order in exact rational arithmetic, the node-time table and the
kernel coefficients are rounded once, and the solver-name handling accepts the new names and lists them when it refuses
one."""
import functools
from fractions import Fraction as Fr

import numpy as np
import pytest
import torch

from stain2stain_amd import flow_matching as F

NAMES = ("euler", "midpoint", "heun", "rk4", "rk4_38")


def order_conditions(c, A, b):
    """{order: [(left side, right side), ...]} of the rooted-tree conditions up to order 4, in Fractions."""
    s = len(c)
    a = [[(A[i][j] if j < len(A[i]) else Fr(0)) for j in range(s)] for i in range(s)]
    R = range(s)
    return {
        1: [(sum(b), Fr(1))],
        2: [(sum(b[i] * c[i] for i in R), Fr(1, 2))],
        3: [(sum(b[i] * c[i] ** 2 for i in R), Fr(1, 3)),
            (sum(b[i] * a[i][j] * c[j] for i in R for j in R), Fr(1, 6))],
        4: [(sum(b[i] * c[i] ** 3 for i in R), Fr(1, 4)),
            (sum(b[i] * c[i] * a[i][j] * c[j] for i in R for j in R), Fr(1, 8)),
            (sum(b[i] * a[i][j] * c[j] ** 2 for i in R for j in R), Fr(1, 12)),
            (sum(b[i] * a[i][j] * a[j][k] * c[k] for i in R for j in R for k in R), Fr(1, 24))],
    }


def test_the_method_names_and_their_export():
    import stain2stain_amd
    assert F.FIXED_STEP_METHODS == NAMES and stain2stain_amd.FIXED_STEP_METHODS == NAMES
    assert stain2stain_amd.fixed_step_generate is F.fixed_step_generate
    assert stain2stain_amd.fixed_step_integrate is F.fixed_step_integrate
    assert {n: F._RK_TABLEAUS[n][0] for n in NAMES} == {"euler": 1, "midpoint": 2, "heun": 2, "rk4": 4, "rk4_38": 4}
    assert [F.fixed_step_evaluations(n, 6) for n in NAMES] == [6, 12, 12, 24, 24]


@pytest.mark.parametrize("name", NAMES)
def test_tableau_meets_the_order_conditions_exactly(name):
    order, c, A, b = F._RK_TABLEAUS[name]
    assert all(isinstance(v, Fr) for v in (*c, *b, *(a for row in A for a in row)))
    assert len(c) == len(A) == len(b) <= 4
    for i, row in enumerate(A):                       # explicit, strictly lower triangular; row sums are the nodes
        assert len(row) <= i and sum(row, Fr(0)) == c[i]
    cond = order_conditions(c, A, b)
    for p in range(1, order + 1):
        for lhs, rhs in cond[p]:
            assert lhs == rhs, (name, p, lhs, rhs)
    if order < 4:                                     # and no higher: the next order's conditions do not all hold
        assert any(lhs != rhs for lhs, rhs in cond[order + 1]), name


def test_euler_fails_the_second_order_condition():
    _, c, A, b = F._RK_TABLEAUS["euler"]
    (lhs, rhs), = order_conditions(c, A, b)[2]
    assert lhs == 0 and rhs == Fr(1, 2)


@pytest.mark.parametrize("num_steps", [1, 3, 7, 12, 50])
@pytest.mark.parametrize("name", NAMES)
def test_node_time_table_is_rounded_once(name, num_steps):
    c = [float(v) for v in F._RK_TABLEAUS[name][1]]
    h = 1.0 / num_steps
    want = np.array([np.float32(k * h + ci * h) for k in range(num_steps) for ci in c], dtype=np.float32)
    got = F.fixed_step_node_times(name, num_steps)
    assert got.dtype == torch.float32 and not got.is_cuda and got.shape == (num_steps * len(c),)
    assert np.array_equal(got.numpy(), want)
    if name == "euler":                               # the table GraphedVelocity walks: k * dt
        assert np.array_equal(got.numpy(), np.array([k * h for k in range(num_steps)], dtype=np.float32))


def test_coefficients_are_double_products_of_the_nonzero_entries():
    rows, weights = F.fixed_step_coefficients("rk4_38", 12)
    h = 1.0 / 12
    assert rows == [[], [(0, h * (1 / 3))], [(0, h * (-1 / 3)), (1, h * 1.0)], [(0, h), (1, -h), (2, h)]]
    assert weights == [(0, h * 0.125), (1, h * 0.375), (2, h * 0.375), (3, h * 0.125)]
    rows, weights = F.fixed_step_coefficients("rk4", 6)
    assert [[j for j, _ in r] for r in rows] == [[], [0], [1], [2]]          # zero coefficients are left out
    assert [j for j, _ in F.fixed_step_coefficients("midpoint", 6)[1]] == [1]


@pytest.mark.parametrize("name", NAMES + ("dopri5",))
def test_solver_name_from_a_config_object_a_partial_and_the_argument(name):
    assert F._solver_method(F.SolverConfig(solver=name)) == name
    assert F._solver_method(functools.partial(dict, solver=name, atol=1e-5)) == name
    assert F._solver_method(F.SolverConfig(solver="dopri5"), name) == name   # method= overrides the solver's choice
    assert F._solver_method(object()) == "dopri5"


@pytest.mark.parametrize("bad", ["rk-4", "RungeKutta4", "RK4", "tsit5", "", 4])
def test_unknown_names_raise_and_the_message_lists_the_accepted_ones(bad):
    def listed(e):
        return all(repr(n) in str(e.value) for n in NAMES + ("dopri5",))
    if bad != "":                                      # an empty method= means "ask the solver", as before
        with pytest.raises(ValueError) as e:
            F._solver_method(F.SolverConfig(), bad)
        assert listed(e)
    with pytest.raises(ValueError) as e:
        F._solver_method(F.SolverConfig(solver=bad) if bad != "" else functools.partial(dict, solver="nope"))
    assert listed(e)
    if isinstance(bad, str) and bad:
        with pytest.raises(ValueError) as e:           # the fixed-step functions: before any tensor is touched
            F.fixed_step_integrate(None, None, 4, bad)
        assert all(repr(n) in str(e.value) for n in NAMES)
        with pytest.raises(ValueError):
            F.fixed_step_generate(None, None, 4, bad)


def test_a_module_refuses_an_unknown_name_before_any_launch():
    mod = F.ConditionalFlowMatchingModule(torch.nn.Identity(), solver=F.SolverConfig(solver="rk-4"))
    x = torch.zeros(1, 3, 4, 4)                        # a host tensor: any launch would raise RuntimeError instead
    with pytest.raises(ValueError, match="'rk4_38'"):
        mod.generate(x, 4)
    with pytest.raises(ValueError, match="'midpoint'"):
        mod.generate(x, 4, method="heun2")
    from stain2stain_amd import multitask_sampler
    with pytest.raises(ValueError, match="'heun'"):
        multitask_sampler(object(), 4, method="rk-4")
    with pytest.raises(ValueError):
        F.fixed_step_generate(None, None, 0, "rk4")    # no steps


def test_per_sample_with_a_fixed_step_method_keeps_raising():
    mod = F.ConditionalFlowMatchingModule(torch.nn.Identity(), solver=F.SolverConfig(solver="midpoint"))
    with pytest.raises(ValueError, match="per_sample"):
        mod.generate(torch.zeros(1, 3, 4, 4), 4, per_sample=True)
    with pytest.raises(ValueError, match="per_sample"):
        mod.generate(torch.zeros(1, 3, 4, 4), 4, method="rk4", per_sample=True)
