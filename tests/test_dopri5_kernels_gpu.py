"""The per-sample Dormand-Prince kernels of csrc/ode.hip one by one, on hand-written state rows and
NaN-poisoned outputs, against two independent references: the ``ops.axpy_`` / ``ops.ode_error_norm`` chain of the
batch-wide solver (bit equality where the design promises it) and the host model tests/dopri5_ref.py, which
tests/test_dopri5_ref_cpu.py holds to the batch-wide solver on the CPU.  Then whole solves on analytic fields, the step
limit and a non-finite field.

Per-sample sizes: 48 (less than one block), 2160 (two blocks and a tail), 263344 = 4 (65536 + 300) (just over the cap of
128 error partials: every block strides) and 1049776 = 4 (262144 + 300) (just over the 1024-block cap of stage and
commit).  B = 4 at the small sizes, B = 2 at the large ones.  All fp32 elements and fp64 state."""
import math

import numpy as np
import pytest
import torch

import dopri5_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL = RTOL = 1e-4
NAN = float("nan")
SIZES = [(4, 48), (4, 2160), (2, 263344), (2, 1049776)]

# Largest fp64 distance of the device's h from the host model's where h depends on pow, measured on the MI355X: 0 ulp
# over the control rows, 1 ulp over the first steps of dp_init.  The bound is four times the larger and
# may never exceed 64 ulp; a wrong factor or clamp moves h by more than 1e-3 relative.
POW_ULP_MEASURED = 1
POW_ULP_BOUND = 4 * POW_ULP_MEASURED
assert POW_ULP_BOUND <= 64


def rand(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, generator=g).to(DEV)


def poisoned(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def expected_partials(N):
    return min(128, max(1, -(-(N // 4) // 512)))


def frozen_sample(B):
    """The last of four; the first of two, so that the one active sample of a large case does not sit at offset 0."""
    return B - 1 if B > 2 else 0


def stage_state(B):
    """Distinct t_b, h_b per sample; one sample is frozen (done = 1, h = 0, t = 1)."""
    rows = [[0.1 + 0.17 * b, 0.03 * (b + 1) + 1e-3 / 7, float(b), 1.0, float(b & 1), 0.0, 1.0, 0.25] for b in range(B)]
    rows[frozen_sample(B)] = [1.0, 0.0, 5.0, 1.0, 0.0, 1.0, 0.0, 0.5]
    return rows


def to_state(rows):
    return torch.tensor(rows, dtype=torch.float64, device=DEV)


def row_sums(part, B, nblk, half=0):
    """Every sample's partials summed in index order, as the control and init kernels sum them."""
    p = part.cpu().numpy()[half * B * nblk:(half + 1) * B * nblk].reshape(B, nblk)
    out = []
    for b in range(B):
        s = 0.0
        for v in p[b]:
            s += float(v)
        out.append(s)
    return out


def f32_ulp(v):
    return float(np.spacing(np.float32(abs(v))))


# ---- stage kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", SIZES)
def test_stage_kernels_against_the_axpy_chain_and_the_model(B, N):
    from stain2stain_amd import ops
    rows = stage_state(B)
    frozen = frozen_sample(B)
    y = rand(B, N, 1)
    ks = [rand(B, N, 10 + j) for j in range(6)]
    for k in ks:
        k[frozen] = NAN                                    # a frozen sample's k_j must never reach its output
    state = to_state(rows)
    y_np, ks_np = y.cpu().numpy(), [k.cpu().numpy() for k in ks]
    for i in range(1, 7):
        who = f"dp_stage_kernel<{i}> B={B} N={N}"
        out, t_out = poisoned(B, N), poisoned(B)
        ops.dp_stage_(i, y, ks, state, out, t_out)
        want = y.clone()
        for b in range(B):
            if b == frozen:
                continue
            for j, a in enumerate(R.A[i]):
                if a != 0.0:
                    ops.axpy_(want[b:b + 1], ks[j][b:b + 1], float(rows[b][R.H] * a))
        assert not bool(out.isnan().any()), f"{who}: output left NaN"
        assert torch.equal(bits(out[frozen]), bits(y[frozen])), f"{who}: frozen sample moved"
        for b in range(B):
            assert torch.equal(bits(out[b]), bits(want[b])), \
                f"{who}: sample {b} differs from the axpy chain by {float((out[b] - want[b]).abs().max()):.3e}"
        out_np, t_np = out.cpu().numpy(), t_out.cpu().numpy()
        for b in range(B):
            kb = [k[b] for k in ks_np]
            ref = R.stage64(i, y_np[b], kb, rows[b][R.H], b == frozen)
            bound = R.stage_bound(i, y_np[b], kb, rows[b][R.H], b == frozen)
            excess = np.abs(out_np[b].astype(np.float64) - ref) - bound
            assert float(excess.max()) <= 0.0, f"{who}: sample {b} is {float(excess.max()):.3e} past the model's bound"
            want_t = R.node_time(rows[b][R.T], R.C[i], rows[b][R.H])
            assert t_np[b] == want_t and t_np[b].dtype == np.float32, f"{who}: t_out[{b}] = {t_np[b]!r}, want {want_t!r}"
        assert t_np[frozen] == np.float32(rows[frozen][R.T])
        assert torch.equal(state, to_state(rows)), f"{who}: wrote the state"


# ---- error kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,k2_none", [(b, n, False) for b, n in SIZES] + [(4, 2160, True)])
def test_error_kernel_partials(B, N, k2_none):
    from stain2stain_amd import ops
    who = f"dp_error_kernel B={B} N={N} k2={'None' if k2_none else 'given'}"
    rows = stage_state(B)
    frozen = frozen_sample(B)
    y, y_new = rand(B, N, 2), rand(B, N, 3)
    ks = [rand(B, N, 20 + j) for j in range(7)]
    for k in ks:
        k[frozen] = NAN
    args = [None if (k2_none and j == 1) else k for j, k in enumerate(ks)]
    state = to_state(rows)
    nblk = ops.dp_partials(N)
    assert nblk == expected_partials(N), f"s2s_dp_partials({N}) = {nblk}"
    part = poisoned(2 * B * nblk, dtype=torch.float64)
    ops.dp_error_(args, y, y_new, state, part, ATOL, RTOL)
    again = poisoned(2 * B * nblk, dtype=torch.float64)
    ops.dp_error_(args, y, y_new, state, again, ATOL, RTOL)
    assert torch.equal(bits(part), bits(again)), f"{who}: two launches differ"
    p = part.cpu().numpy()
    assert np.isnan(p[B * nblk:]).all(), f"{who}: wrote the second half of the workspace"
    assert np.isnan(p[frozen * nblk:(frozen + 1) * nblk]).all(), f"{who}: wrote the frozen sample's partials"
    sums = row_sums(part, B, nblk)
    equal = 0
    for b in range(B):
        if b == frozen:
            continue
        assert np.isfinite(p[b * nblk:(b + 1) * nblk]).all(), f"{who}: sample {b} has a non-finite or unwritten partial"
        en = R.rms_f32(sums[b], N)
        err = torch.zeros(1, N, device=DEV)
        for j, e in enumerate(R.E):
            if e != 0.0:
                ops.axpy_(err, ks[j][b:b + 1], float(rows[b][R.H] * e))
        ref = float(ops.ode_error_norm(err, y[b:b + 1].contiguous(), y_new[b:b + 1].contiguous(), ATOL, RTOL))
        equal += en == ref
        assert abs(en - ref) <= f32_ulp(ref), f"{who}: sample {b} norm {en!r} vs s2s_ode_error_norm {ref!r}"
        host = R.rms_f32(R.scaled_square_sum(err[0].cpu().numpy(), y[b].cpu().numpy(), y_new[b].cpu().numpy(), ATOL,
                                             RTOL), N)
        assert abs(en - host) <= 2.0 ** -21 * host, f"{who}: sample {b} norm {en!r} vs the host model {host!r}"
        # the error estimate itself, against the model's float64 one (6 fp32 fmas from 0)
        e64 = R.error64([k[b].cpu().numpy() for k in ks], rows[b][R.H])
        mag = sum(abs(float(c)) * np.abs(k[b].cpu().numpy().astype(np.float64))
                  for c, k, e in zip(R.error_coeffs(rows[b][R.H]), ks, R.E) if e != 0.0)
        assert float((np.abs(err[0].cpu().numpy() - e64) - 7 * 2.0 ** -24 * mag).max()) <= 0.0, \
            f"{who}: the axpy chain's error estimate of sample {b} is off the model's"
    print(f"{who}: {equal} of {B - 1} norms exactly equal to s2s_ode_error_norm's")


# ---- control kernel ---------------------------------------------------------------------------------------------------
def below_one():
    return float(np.float32(1.0) - np.float32(2.0 ** -24))


# (what, t, h, rejected flag, done, chosen en); the partials are built so that rms_f32 gives en
CONTROL_KINDS = [
    ("en = 0: factor 10", 0.1, 0.05, 0.0, 0.0, 0.0),
    ("tiny en: clamp to 10", 0.1, 0.02, 0.0, 0.0, 1e-8),
    ("mid-range accept", 0.2, 0.05, 0.0, 0.0, 0.3),
    ("accept after a rejection: capped to 1", 0.2, 0.07, 1.0, 0.0, 0.3),
    ("en just below 1", 0.3, 0.05, 0.0, 0.0, below_one()),
    ("en exactly 1: reject", 0.3, 0.06, 0.0, 0.0, 1.0),
    ("mid-range reject", 0.4, 0.05, 0.0, 0.0, 3.0),
    ("huge en: the 0.2 floor", 0.4, 0.08, 0.0, 0.0, 1e6),
    ("en = inf", 0.5, 0.05, 0.0, 0.0, float("inf")),
    ("en = NaN", 0.5, 0.09, 1.0, 0.0, NAN),
    ("accept with t + h >= 1: freezes", 0.75, 0.25, 0.0, 0.0, 0.5),
    ("accept with h * factor > 1 - t", 0.5, 0.3, 0.0, 0.0, 1e-8),
    ("already frozen", 1.0, 0.0, 0.0, 1.0, NAN),
]
CONTROL_N = 2160                                           # two partials per sample


def control_case(kinds):
    """State rows and the partial workspace (first half) for a list of kinds."""
    n, nblk = CONTROL_N, expected_partials(CONTROL_N)
    rows, part = [], []
    for q, (what, t, h, rejflag, done, en) in enumerate(kinds):
        rows.append([t, h, float(q % 5), float(q % 3), rejflag, done, float(q & 1), 0.125])
        if done:
            part += [NAN, NAN]                              # a frozen row's partials are stale: never read
        elif en != en:
            part += [1.0, NAN]
        elif math.isinf(en):
            part += [en, 1.0]
        else:
            total = en * en * n
            part += [0.25 * total, 0.75 * total]
    return rows, part, nblk


@pytest.mark.parametrize("B,first", [(12, 0), (12, 1), (300, 0)])
def test_control_kernel_rows_and_status(B, first):
    """Thirteen kinds of row: a launch of 12 holds kinds 0..11 or 1..12, one of 300 repeats all of them round-robin (so
    the strided tail beyond 256 threads is not uniform).  Three step limits around the attempt counter."""
    from stain2stain_amd import ops
    kinds = [CONTROL_KINDS[(first + b) % len(CONTROL_KINDS)] for b in range(B)]
    rows, part_rows, nblk = control_case(kinds)
    # the construction really gives the chosen norms at the two edges of the accept test
    for b, kind in enumerate(kinds):
        if kind[0] in ("en just below 1", "en exactly 1: reject"):
            s = part_rows[2 * b] + part_rows[2 * b + 1]
            assert R.rms_f32(s, CONTROL_N) == kind[5], kind
    attempts = 41
    worst = 0.0
    for max_steps in (attempts + 2, attempts + 1, attempts):          # attempts + 1 is the counter after this launch
        who = f"dp_control_kernel B={B} first={first} max_steps={max_steps}"
        state = to_state(rows)
        part = torch.cat([torch.tensor(part_rows, dtype=torch.float64),
                          torch.full((B * nblk,), NAN, dtype=torch.float64)]).to(DEV)       # second half: not control's
        part0 = part.clone()
        status = torch.tensor([77, 5, attempts, 0], dtype=torch.int32, device=DEV)
        ops.dp_control_(state, part, status, max_steps, B, CONTROL_N)
        got = state.cpu().numpy()
        sums = row_sums(part, B, nblk)
        want_rows = []
        for b, kind in enumerate(kinds):
            en = NAN if rows[b][R.DONE] else R.rms_f32(sums[b], CONTROL_N)
            want = R.control(rows[b], en)
            want_rows.append(want)
            g = [float(v) for v in got[b]]
            msg = f"{who}: row {b} ({kind[0]}): got {g}, want {want}"
            for slot in (R.T, R.ACC, R.REJ, R.REJECTED, R.DONE, R.ACCEPT):
                assert g[slot] == want[slot], msg
            assert g[R.AUX] == want[R.AUX] or (g[R.AUX] != g[R.AUX] and want[R.AUX] != want[R.AUX]), msg
            if rows[b][R.DONE]:
                assert g[:R.ACCEPT] == rows[b][:R.ACCEPT] and g[R.ACCEPT] == 0.0 and g[R.AUX] == rows[b][R.AUX], msg
            if R.control_h_is_exact(rows[b], en):
                assert g[R.H] == want[R.H], msg
            else:
                d = R.ulp_distance(g[R.H], want[R.H])
                worst = max(worst, d)
                assert d <= POW_ULP_BOUND, msg + f": h is {d} ulp from the model"
        by_pow = {k[0] for k, r in zip(kinds, rows) if not R.control_h_is_exact(r, k[5])}    # everything else: exact
        assert by_pow <= {"mid-range accept", "en just below 1", "en exactly 1: reject", "mid-range reject"}, by_pow
        want_status = R.status_after(want_rows, attempts, max_steps)
        assert tuple(status.tolist()) == want_status, f"{who}: status {status.tolist()}, want {want_status}"
        assert want_status[1] == (1 if max_steps <= attempts + 1 else 0)
        assert torch.equal(bits(part), bits(part0)), f"{who}: wrote the partials"
    print(f"dp_control_kernel B={B} first={first}: largest distance of h from the host model where pow decides: "
          f"{worst} ulp (fp64)")


# ---- commit kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", SIZES)
def test_commit_kernel_moves_accepted_rows_only(B, N):
    from stain2stain_amd import ops
    rows = stage_state(B)
    accept = [1.0, 0.0, 1.0, 0.0] if B == 4 else [0.0, 1.0]           # the frozen row is never accepted
    for b in range(B):
        rows[b][R.ACCEPT] = accept[b]
    state = to_state(rows)
    y, y_new, k1, k7 = rand(B, N, 4), rand(B, N, 5), rand(B, N, 6), rand(B, N, 7)
    y0, k10, yn0, k70 = y.clone(), k1.clone(), y_new.clone(), k7.clone()
    ops.dp_commit_(y, y_new, k1, k7, state)
    for b in range(B):
        who = f"dp_commit_kernel B={B} N={N} sample {b}"
        if accept[b]:
            assert torch.equal(bits(y[b]), bits(yn0[b])) and torch.equal(bits(k1[b]), bits(k70[b])), \
                f"{who}: accepted but not committed"
        else:
            assert torch.equal(bits(y[b]), bits(y0[b])) and torch.equal(bits(k1[b]), bits(k10[b])), \
                f"{who}: changed without an accept"
    assert torch.equal(y_new, yn0) and torch.equal(k7, k70) and torch.equal(state, to_state(rows))


# ---- init, both phases ------------------------------------------------------------------------------------------------
def init_sample(kind, N, seed):
    """(y, k1, fa) of one sample."""
    g = torch.Generator().manual_seed(seed)
    y, k1, fa = (torch.randn(N, generator=g) for _ in range(3))
    if kind == "generic":
        pass
    elif kind == "y = 0":
        y = torch.zeros(N)
    elif kind == "k1 = 0":
        k1 = torch.zeros(N)
    elif kind == "k1 = 0 = fa":
        k1, fa = torch.zeros(N), torch.zeros(N)
    elif kind == "cap at 1":                               # d1 small but >= 1e-5, d2 smaller still: h1 > 1, 100 h0 > 1
        k1 = torch.full((N,), 1e-7)
        fa = 2.0 * k1
    else:
        raise ValueError(kind)
    return y, k1, fa


FOUR = ("generic", "y = 0", "k1 = 0", "k1 = 0 = fa")
INIT_CASES = [(48, FOUR), (2160, FOUR), (2160, ("cap at 1", "k1 = 0 = fa", "generic", "y = 0")),
              (263344, ("generic", "k1 = 0 = fa")), (1049776, ("cap at 1", "k1 = 0"))]


@pytest.mark.parametrize("N,kinds", INIT_CASES, ids=[f"{n}-{k[0].split()[0]}" for n, k in INIT_CASES])
def test_init_kernels_both_phases(N, kinds):
    from stain2stain_amd import ops
    B = len(kinds)
    who = f"dp_init N={N} {kinds}"
    samples = [init_sample(kind, N, 30 + b) for b, kind in enumerate(kinds)]
    y, k1, fa = (torch.stack([s[j] for s in samples]).to(DEV) for j in range(3))
    y_np, k1_np, fa_np = (t.cpu().numpy() for t in (y, k1, fa))
    nblk = ops.dp_partials(N)
    norm = lambda e, b: R.rms_f32(R.scaled_square_sum(e, y_np[b], y_np[b], ATOL, RTOL), N)
    near = lambda got, want: abs(got - want) <= 2.0 ** -21 * abs(want)

    state = poisoned(B, 8, dtype=torch.float64)
    status = torch.tensor([-7, 9, 1234, 55], dtype=torch.int32, device=DEV)
    part = poisoned(2 * B * nblk, dtype=torch.float64)
    out, t_out = poisoned(B, N), poisoned(B)
    ops.dp_init_(0, y, k1, None, state, part, out, t_out, status, ATOL, RTOL)
    assert bool(part.isfinite().all()), f"{who} phase 0: partials left unwritten"
    d0s, d1s = ([R.rms_f32(s, N) for s in row_sums(part, B, nblk, half)] for half in (0, 1))
    st0 = state.cpu().numpy()
    want_probe = y.clone()
    for b, kind in enumerate(kinds):
        msg = f"{who} phase 0 sample {b} ({kind}): row {st0[b].tolist()}, d0 {d0s[b]!r}, d1 {d1s[b]!r}"
        assert near(d0s[b], norm(y_np[b], b)) and near(d1s[b], norm(k1_np[b], b)), msg
        h0 = R.init_h0(d0s[b], d1s[b])
        assert st0[b][R.H] == h0 and near(h0, R.init_h0(norm(y_np[b], b), norm(k1_np[b], b))), msg
        assert st0[b][R.AUX] == d1s[b], msg
        assert all(st0[b][s] == 0.0 for s in (R.T, R.ACC, R.REJ, R.REJECTED, R.DONE, R.ACCEPT)), msg
        if kind != "generic" and kind != "cap at 1":
            assert h0 == 1e-6, msg
        ops.axpy_(want_probe[b:b + 1], k1[b:b + 1], float(h0))
        assert t_out[b].item() == float(R.node_time(0.0, R.PROBE_NODE, h0)), msg
    assert torch.equal(bits(out), bits(want_probe)), f"{who} phase 0: probe differs from y + axpy(h0 k1)"
    assert status.tolist() == [-7, 9, 1234, 55], f"{who} phase 0 wrote the status word"

    part.fill_(NAN)
    out2, t2 = poisoned(B, N), poisoned(B)
    ops.dp_init_(1, y, k1, fa, state, part, out2, t2, status, ATOL, RTOL)
    assert bool(out2.isnan().all()) and bool(t2.isnan().all()), f"{who} phase 1 wrote the probe outputs"
    assert bool(part[B * nblk:].isnan().all()) and bool(part[:B * nblk].isfinite().all()), f"{who} phase 1 partials"
    sums = row_sums(part, B, nblk)
    st1 = state.cpu().numpy()
    worst = 0.0
    for b, kind in enumerate(kinds):
        h0, d1 = float(st0[b][R.H]), d1s[b]
        dd = R.rms_f32(sums[b], N)
        assert near(dd, norm(fa_np[b] - k1_np[b], b)), f"{who} phase 1 sample {b} ({kind}): norm {dd!r}"
        d2 = dd / h0
        want = R.init_h(h0, d1, d2)
        msg = f"{who} phase 1 sample {b} ({kind}): row {st1[b].tolist()}, want h {want!r} (h0 {h0!r} d1 {d1!r} d2 {d2!r})"
        if R.init_h_is_exact(h0, d1, d2):
            assert st1[b][R.H] == want, msg
        else:
            d = R.ulp_distance(float(st1[b][R.H]), want)
            worst = max(worst, d)
            assert d <= POW_ULP_BOUND, msg + f": {d} ulp"
        assert (kind == "generic") == (not R.init_h_is_exact(h0, d1, d2)), msg      # the kinds take the paths they name
        if kind == "cap at 1":
            assert st1[b][R.H] == 1.0, msg
        if kind == "k1 = 0 = fa":
            assert d1 == 0.0 and d2 == 0.0 and st1[b][R.H] == 1e-6, msg
        assert all(st1[b][s] == 0.0 for s in (R.T, R.ACC, R.REJ, R.REJECTED, R.DONE, R.ACCEPT, R.AUX)), msg
    assert status.tolist() == [B, 0, 0, 0], f"{who} phase 1: status {status.tolist()}"
    print(f"{who}: largest distance of the first step from the host model where pow decides: {worst} ulp (fp64)")


# ---- whole solves on analytic fields ----------------------------------------------------------------------------------
def source_tile():
    g = torch.Generator().manual_seed(3)
    return 2.0 + torch.rand(1, 3, 4, 4, generator=g)


def batch_field(names, calls=None):
    """``f(t[B], x)``: sample b follows field ``names[b]``; every field is element-wise, so a sample's velocity does not
    depend on its position or its batch mates."""
    def f(t, x):
        if calls is not None:
            calls.append(x.shape[0])
        tt = t.view(-1, 1, 1, 1)
        return torch.cat([R.FIELDS[n](torch, tt[b:b + 1], x[b:b + 1]) for b, n in enumerate(names)]).contiguous()
    return f


def batch_sources():
    tile = source_tile()
    return torch.cat([torch.zeros_like(tile) if zero else tile for _, zero in R.CASES]).to(DEV)


def test_batch_of_seven_fields_equals_each_sample_alone():
    from conftest import relerr
    from stain2stain_amd import dopri5_integrate
    names = [n for n, _ in R.CASES]
    x0 = batch_sources()
    got, st = dopri5_integrate(batch_field(names), x0.clone(), ATOL, RTOL, return_stats=True, per_sample=True)
    assert st["attempted"] == max(a + r for a, r in zip(st["accepted"], st["rejected"]))
    for b, name in enumerate(names):
        who = f"per-sample dopri5, sample {b} ({name})"
        f = batch_field([name])
        alone, sa = dopri5_integrate(f, x0[b:b + 1].clone(), ATOL, RTOL, return_stats=True, per_sample=True)
        assert torch.equal(bits(got[b:b + 1]), bits(alone)), f"{who}: differs from its solve alone"
        counts = (st["accepted"][b], st["rejected"][b])
        assert counts == (sa["accepted"][0], sa["rejected"][0]), who
        wide, sw = dopri5_integrate(f, x0[b:b + 1].clone(), ATOL, RTOL, return_stats=True)
        print(f"{who}: accepted / rejected {counts}, batch-wide {sw}, bit-equal {torch.equal(alone, wide)}")
        assert counts == (sw["accepted"], sw["rejected"]), f"{who}: {counts} vs the batch-wide solver's {sw}"
        assert relerr(alone, wide) <= 1e-6, who
        if name in R.REJECTING:
            assert counts[1] >= 1, who
        if name == "zero":
            assert counts == (7, 0) and torch.equal(bits(got[b]), bits(x0[b])), who


def test_a_nan_mate_leaves_the_healthy_samples_alone():
    from stain2stain_amd.samplers import _PerSampleDopri5
    names = [n for n, _ in R.CASES]
    x0 = batch_sources()
    runs = []
    for mates in ([], ["nan"]):
        src = torch.cat([x0, source_tile().to(DEV)]) if mates else x0
        solver = _PerSampleDopri5(batch_field(names + mates), src, ATOL, RTOL, 1000)
        solver.init(src)
        trace = [(solver.state.clone(), solver.y.clone())]
        for _ in range(5):
            solver.step()
            trace.append((solver.state.clone(), solver.y.clone(), solver.status.clone()))
        runs.append(trace)
    n = len(names)
    for k, (a, b) in enumerate(zip(*runs)):
        assert not bool(a[0].isnan().any()), f"attempt {k}: a healthy state row holds NaN"
        assert torch.equal(bits(a[0]), bits(b[0][:n])), f"per-sample dopri5: state rows differ after attempt {k}"
        assert torch.equal(bits(a[1]), bits(b[1][:n])), f"per-sample dopri5: y differs after attempt {k}"
        if k:
            assert b[2].tolist()[0] == a[2].tolist()[0] + 1                         # the NaN mate never finishes
            assert b[0][n, R.ACC].item() == 0.0 and b[0][n, R.REJ].item() == float(k)
            assert torch.equal(bits(b[1][n]), bits(source_tile().to(DEV)[0]))


@pytest.mark.parametrize("per_sample", [True, False])
def test_step_limit_on_the_zero_field(per_sample):
    from stain2stain_amd import dopri5_integrate
    x0 = source_tile().to(DEV)
    f = batch_field(["zero"])
    with pytest.raises(RuntimeError, match="max_steps"):
        dopri5_integrate(f, x0.clone(), ATOL, RTOL, 7, per_sample=per_sample)
    got, st = dopri5_integrate(f, x0.clone(), ATOL, RTOL, 8, return_stats=True, per_sample=per_sample)
    assert torch.equal(got, x0)
    assert (st["accepted"], st["rejected"]) == (([7], [0]) if per_sample else (7, 0))


@pytest.mark.parametrize("per_sample", [True, False])
def test_nan_field_runs_into_the_limit_after_38_evaluations(per_sample):
    from stain2stain_amd import dopri5_integrate
    calls = []
    with pytest.raises(RuntimeError, match="max_steps"):
        dopri5_integrate(batch_field(["nan"], calls), source_tile().to(DEV), ATOL, RTOL, 6, per_sample=per_sample)
    assert len(calls) == 2 + 6 * 6
