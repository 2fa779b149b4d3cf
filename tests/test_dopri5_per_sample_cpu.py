"""Host side of the per-sample Dormand-Prince solver (csrc/ode.hip): argument validation returns status codes before
any launch, and the solver refuses CPU tensors (there is no CPU path)."""
import ctypes

import pytest
import torch

OK = ctypes.c_void_p(4096)
ODD = ctypes.c_void_p(4096 + 8)


def test_dp_entry_points_reject_bad_arguments_without_a_gpu():
    from stain2stain_amd import _native
    lib = _native.lib()
    assert lib.s2s_dp_partials(4) == 1 and lib.s2s_dp_partials(3 * 256 * 256) >= 1 and lib.s2s_dp_partials(0) == 0
    # init
    init = lambda ph, y, fa, n: lib.s2s_dp_init(ph, y, OK, fa, OK, OK, OK, OK, OK, 1e-4, 1e-4, 2, n, None)
    assert init(0, None, None, 16) == -5 and init(1, OK, None, 16) == -5
    assert init(0, OK, None, 18) == -1 and init(2, OK, OK, 16) == -1 and init(0, OK, None, 0) == -1
    assert init(0, ODD, None, 16) == -2 and init(1, OK, ODD, 16) == -2
    # stage
    stage = lambda i, y, k, n, B=2: lib.s2s_dp_stage(i, y, *k, OK, OK, OK, B, n, None)
    ks = [OK] * 6
    assert stage(0, OK, ks, 16) == -1 and stage(7, OK, ks, 16) == -1
    assert stage(3, None, ks, 16) == -5 and stage(3, OK, [OK, OK, None, None, None, None], 16) == -5
    assert stage(2, OK, [OK, OK, None, None, None, None], 6) == -1 and stage(1, OK, ks, 16, B=0) == -1
    assert stage(2, ODD, ks, 16) == -2 and stage(2, OK, [OK, ODD] + [None] * 4, 16) == -2
    # error
    err = lambda k, y, n: lib.s2s_dp_error(*k, y, OK, OK, OK, 1e-4, 1e-4, 2, n, None)
    k7 = [OK] * 7
    assert err(k7, None, 16) == -5 and err([OK] * 6 + [None], OK, 16) == -5
    assert err(k7, OK, 10) == -1 and err(k7, ODD, 16) == -2 and err([OK] * 6 + [ODD], OK, 16) == -2
    # control, commit
    assert lib.s2s_dp_control(None, OK, OK, 10, 2, 16, None) == -5
    assert lib.s2s_dp_control(OK, OK, OK, 10, 0, 16, None) == -1
    assert lib.s2s_dp_commit(OK, OK, None, OK, OK, 2, 16, None) == -5
    assert lib.s2s_dp_commit(OK, OK, OK, OK, OK, 2, 14, None) == -1
    assert lib.s2s_dp_commit(OK, OK, OK, ODD, OK, 2, 16, None) == -2


def test_per_sample_dopri5_refuses_cpu_tensors():
    from stain2stain_amd import dopri5_generate, dopri5_integrate
    x = torch.zeros(2, 3, 4, 4)
    f = lambda t, y: -y
    with pytest.raises(RuntimeError, match="GPU"):
        dopri5_integrate(f, x, per_sample=True)
    with pytest.raises(RuntimeError, match="GPU"):
        dopri5_generate(f, x, per_sample=True)
