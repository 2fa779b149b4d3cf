"""The ODE samplers: x(1) of dx/dt = v(t, x), x(0) = source, for an eval-mode network or any callable ``f(t[B], x)``.

  reference                                                               here
  ----------------------------------------------------------------------  ---------------------------
  NeuralODE(dopri5).trajectory in generate                                dopri5_integrate / dopri5_generate (batch-wide
    (src/models/conditional_flow_matching.py:157-170, torchdyn, absent)   step size; ``per_sample=True``: one per sample,
                                                                          _PerSampleDopri5)
  fixed-step Euler (BASELINE.json configs[3])                             euler_integrate / euler_generate
  the fixed-step solver names a ``solver:`` entry may carry               fixed_step_integrate / fixed_step_generate
    (midpoint, Heun, RK4; configs/model/conditional_flow_matching.yaml)   (_FixedStepRK)

Every solver also runs as a replayed hipGraph: ``GraphedVelocity`` (one evaluation or one Euler step), ``_FixedStepGraph``
(one Runge-Kutta step) and ``_Dopri5Graph`` (one attempted per-sample step) are ``_GraphedStep``s, which owns the cache
key, the warm-up, the capture and the lifetime.  ``solve`` is the one place that maps (method, graph, per_sample) to a
solver; the ``*_generate`` functions, the modules' ``generate`` and ``region.multitask_sampler`` all call it.
"""
from __future__ import annotations

from fractions import Fraction as _Fr
from typing import List, Optional

import torch

from . import ops


class _eval_mode:
    """``module.eval()`` for the duration of a sampling loop, previous mode restored even when the loop raises.  Only
    the module handed in is touched: wrappers around a LightningModule are plain callables, never ``nn.Module``s that
    would register it as a child and flip its mode behind its back."""

    def __init__(self, net):
        self.net = net if isinstance(net, torch.nn.Module) else None

    def __enter__(self):
        if self.net is not None:
            self.was = self.net.training
            self.net.eval()

    def __exit__(self, *exc):
        if self.net is not None:
            self.net.train(self.was)
        return False


def _prep_source(source_img: torch.Tensor) -> torch.Tensor:
    if source_img.dim() == 3:
        source_img = source_img.unsqueeze(0)
    return source_img.detach().float().contiguous().clone()


@torch.no_grad()
def euler_integrate(f, x: torch.Tensor, num_steps: int) -> torch.Tensor:
    """x <- x + f(t_k, x)/n at t_k = k/n for a callable ``f(t[B], x)``; ``x`` is advanced in place and returned."""
    dt = 1.0 / num_steps
    for k in range(num_steps):
        t = torch.full((x.shape[0],), k * dt, device=x.device, dtype=torch.float32)
        ops.axpy_(x, f(t, x).contiguous(), dt)
    return x

def _params(net):
    net = getattr(net, "__self__", net)                 # a bound method: the parameters of its module
    return list(net.parameters()) if isinstance(net, torch.nn.Module) else []


# Dormand-Prince 5(4): nodes, stage matrix (row 7 = the 5th-order weights, first-same-as-last) and error weights
_DP_C = (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0)
_DP_A = ((),
         (1 / 5,),
         (3 / 40, 9 / 40),
         (44 / 45, -56 / 15, 32 / 9),
         (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
         (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656),
         (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84))
_DP_E = (-71 / 57600, 0.0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40)


# Explicit fixed-step Runge-Kutta tableaus with at most four stages: name -> (order, c, A rows, b), exact rationals.
# ``rk4`` is the classical scheme, ``rk4_38`` Kutta's 3/8 rule; which of the two torchdyn's ``rk4`` name selects is
# unpinned (the package is absent), so both are offered.
_RK_TABLEAUS = {
    "euler": (1, (_Fr(0),), ((),), (_Fr(1),)),
    "midpoint": (2, (_Fr(0), _Fr(1, 2)), ((), (_Fr(1, 2),)), (_Fr(0), _Fr(1))),
    "heun": (2, (_Fr(0), _Fr(1)), ((), (_Fr(1),)), (_Fr(1, 2), _Fr(1, 2))),
    "rk4": (4, (_Fr(0), _Fr(1, 2), _Fr(1, 2), _Fr(1)),
            ((), (_Fr(1, 2),), (_Fr(0), _Fr(1, 2)), (_Fr(0), _Fr(0), _Fr(1))),
            (_Fr(1, 6), _Fr(1, 3), _Fr(1, 3), _Fr(1, 6))),
    "rk4_38": (4, (_Fr(0), _Fr(1, 3), _Fr(2, 3), _Fr(1)),
               ((), (_Fr(1, 3),), (_Fr(-1, 3), _Fr(1)), (_Fr(1), _Fr(-1), _Fr(1))),
               (_Fr(1, 8), _Fr(3, 8), _Fr(3, 8), _Fr(1, 8))),
}
FIXED_STEP_METHODS = tuple(_RK_TABLEAUS)
SOLVER_METHODS = ("dopri5",) + FIXED_STEP_METHODS


def _check_fixed_step(method: str, num_steps) -> int:
    if method not in _RK_TABLEAUS:
        raise ValueError(f"fixed-step method must be one of {', '.join(map(repr, FIXED_STEP_METHODS))}, got {method!r}")
    import operator
    num_steps = operator.index(num_steps)
    if num_steps < 1:
        raise ValueError(f"num_steps must be >= 1, got {num_steps}")
    return num_steps


def fixed_step_evaluations(method: str, num_steps: int) -> int:
    """Network evaluations of a ``num_steps``-step solve: ``num_steps`` times the number of stages."""
    return _check_fixed_step(method, num_steps) * len(_RK_TABLEAUS[method][1])


def fixed_step_coefficients(method: str, num_steps: int):
    """(stage rows, weights) as the kernels get them: the non-zero entries ``(j, float(h * a_ij))`` of every row of A and
    ``(j, float(h * b_j))`` of b, ascending j, h = 1 / num_steps; each product is formed in double (the launch rounds it
    to fp32 once, as ``ops.axpy_`` rounds its scalar)."""
    num_steps = _check_fixed_step(method, num_steps)
    _, _, A, b = _RK_TABLEAUS[method]
    h = 1.0 / num_steps
    rows = [[(j, float(h * float(a))) for j, a in enumerate(row) if a != 0] for row in A]
    return rows, [(j, float(h * float(w))) for j, w in enumerate(b) if w != 0]


def fixed_step_node_times(method: str, num_steps: int) -> torch.Tensor:
    """The fp32 table [num_steps * stages] of node times on the host: entry (k, i) is ``k * h + c_i * h`` formed in
    double and rounded once, as the Euler path forms ``k * dt``."""
    num_steps = _check_fixed_step(method, num_steps)
    c = _RK_TABLEAUS[method][1]
    h = 1.0 / num_steps
    return torch.tensor([k * h + float(ci) * h for k in range(num_steps) for ci in c], dtype=torch.float32)


class _FixedStepRK:
    """A fixed-step explicit Runge-Kutta solve of ``dx/dt = f(t, x)`` on the grid of the Euler path (``num_steps`` steps
    of h = 1 / num_steps from 0 to 1) with the fused kernels of csrc/ode.hip: per step one
    stage launch and one evaluation per stage, then one combine launch.  The node times sit in a device table that the
    stage launches index with a device-side step counter, which only the combine launch advances, so ``step`` takes no
    host-side argument, allocates nothing outside ``f`` and never synchronises: ``_FixedStepGraph`` captures it whole.
    ``f`` must return a tensor of its own on every call (the k_j of one step are read together)."""

    def __init__(self, f, x: torch.Tensor, num_steps: int, method: str):
        num_steps = _check_fixed_step(method, num_steps)
        if not x.is_cuda:
            raise RuntimeError("stain2stain_amd: the fixed-step samplers need GPU tensors (there is no CPU path)")
        if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() < 2 or x.numel() == 0 or (x[0].numel() % 4):
            raise RuntimeError("stain2stain_amd: the fixed-step samplers want contiguous fp32 [B, ...] samples of a "
                               "multiple of 4 elements")
        self.f, self.x, self.num_steps, self.method = f, x, num_steps, method
        self.stages = len(_RK_TABLEAUS[method][1])
        self.rows, self.weights = fixed_step_coefficients(method, num_steps)
        self.xs = torch.empty_like(x) if self.stages > 1 else None
        self.t = torch.zeros((x.shape[0],), dtype=torch.float32, device=x.device)
        self.table = fixed_step_node_times(method, num_steps).to(x.device)
        self.counter = torch.zeros((1,), dtype=torch.int32, device=x.device)

    def step(self) -> List[torch.Tensor]:
        """One step: x advanced in place, the counter moved on; returns the k_j."""
        ks: List[torch.Tensor] = []
        for i, row in enumerate(self.rows):
            terms = [(c, ks[j]) for j, c in row]
            out = self.xs if terms else None              # a row of zeros evaluates on x itself: the node time alone
            ops.rk_stage_(self.x, terms, out, self.t, self.table, self.counter, self.stages, i)
            ks.append(self.f(self.t, self.x if out is None else out).contiguous())
        ops.rk_combine_(self.x, [(c, ks[j]) for j, c in self.weights], self.counter)
        return ks

    def solve(self) -> torch.Tensor:
        self.counter.zero_()
        for _ in range(self.num_steps):
            self.step()
        return self.x


@torch.no_grad()
def fixed_step_integrate(f, x: torch.Tensor, num_steps: int, method: str = "rk4") -> torch.Tensor:
    """``num_steps`` steps of the explicit Runge-Kutta scheme ``method`` (one of ``FIXED_STEP_METHODS``) from t = 0 to
    t = 1 for a callable ``f(t[B], x)``; ``x`` (contiguous fp32 on the GPU) is advanced in place and returned, like
    ``euler_integrate``, to which ``method="euler"`` delegates.  ``num_steps`` evaluations per stage of the scheme: 2 per
    step for ``midpoint`` and ``heun``, 4 for ``rk4`` (classical) and ``rk4_38`` (3/8 rule).  Every sample is stepped
    on the same grid, so a sample's result does not depend on its batch mates.  The stage and combine arithmetic is the
    chain ``clone`` + ``ops.axpy_`` per non-zero coefficient, bit for bit, in one launch each."""
    num_steps = _check_fixed_step(method, num_steps)
    if method == "euler":
        return euler_integrate(f, x, num_steps)
    return _FixedStepRK(f, x, num_steps, method).solve()



@torch.no_grad()
def dopri5_integrate(net, y: torch.Tensor, atol: float = 1e-4, rtol: float = 1e-4, max_steps: int = 1000,
                     return_stats: bool = False, per_sample: bool = False):
    """Adaptive sampler for a callable ``net(t[B], x)``: x(1) of dx/dt = v(t, x), x(0) = source, eval-mode network, by the Dormand-Prince 5(4) pair.

    The reference integrates with torchdyn's ``NeuralODE(solver="dopri5", atol=1e-4, rtol=1e-4)``
    (conditional_flow_matching.py:157-170); torchdyn is absent, so the step-size control here is the textbook one
    (the same as scipy's ``RK45``: scaled RMS error, factor 0.9 err^(-1/5) clamped to [0.2, 10], no growth right
    after a rejection, Hairer's initial-step heuristic) -- parity with torchdyn's controller is unpinned, the
    solution agrees with any dopri5 to the tolerances.  Stage combinations and the error norm run in HIP
    (``s2s_axpy``, ``s2s_ode_error_norm``); one host read of the error norm per attempted step.

    The error norm, ``t`` and ``h`` are shared by the whole batch, so a sample's result depends on its batch mates.
    ``per_sample=True`` steps every sample as if it were alone in a batch of one (its own norm, initial step, ``t`` and
    ``h``, all on the device: ``_PerSampleDopri5``); a sample that reaches t = 1 is frozen until the batch is done.  Its
    stats are per-sample ``accepted`` / ``rejected`` lists plus ``attempted``, ``evaluations`` and ``host_reads``."""
    if per_sample:
        return _PerSampleDopri5(net, y, atol, rtol, max_steps).solve(y, return_stats)
    B = y.shape[0]

    def f(t, x):
        return net(torch.full((B,), float(t), device=x.device, dtype=torch.float32), x).contiguous()

    def rms_scaled(e, a, b):
        return float(ops.ode_error_norm(e, a, b, atol, rtol))

    t, t1 = 0.0, 1.0
    k1 = f(t, y)
    # initial step (Hairer, Norsett, Wanner II.4; scipy's select_initial_step)
    d0 = rms_scaled(y, y, y)
    d1 = rms_scaled(k1, y, y)
    h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    ya = y.clone()
    ops.axpy_(ya, k1, h0)
    fa = f(t + h0, ya)
    ops.axpy_(fa, k1, -1.0)
    d2 = rms_scaled(fa, y, y) / h0
    h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** (1.0 / 5.0)
    h = min(100 * h0, h1, t1 - t)
    n_acc = n_rej = 0
    rejected = False
    for _ in range(max_steps):
        if t >= t1:
            break
        h = min(h, t1 - t)
        ks = [k1]
        for i in range(1, 7):
            yi = y.clone()
            for j, a in enumerate(_DP_A[i]):
                if a != 0.0:
                    ops.axpy_(yi, ks[j], h * a)
            if i == 6:
                y_new = yi
            ks.append(f(t + _DP_C[i] * h, yi))
        err = torch.zeros_like(y)
        for j, e in enumerate(_DP_E):
            if e != 0.0:
                ops.axpy_(err, ks[j], h * e)
        en = rms_scaled(err, y, y_new)
        if en < 1.0:
            factor = 10.0 if en == 0.0 else min(10.0, 0.9 * en ** -0.2)
            if rejected:
                factor = min(1.0, factor)
            t, y, k1 = t + h, y_new, ks[6]
            h *= factor
            rejected = False
            n_acc += 1
        else:
            h *= max(0.2, 0.9 * en ** -0.2)
            rejected = True
            n_rej += 1
    else:
        raise RuntimeError("dopri5_generate: max_steps reached before t = 1")
    return (y, {"accepted": n_acc, "rejected": n_rej}) if return_stats else y


class _PerSampleDopri5:
    """The per-sample Dormand-Prince solver (csrc/ode.hip): device-resident per-sample state
    (fp64 t, h, counters, flags), fused stage / error / control / commit kernels and every workspace they need.

    One attempted step is ``step()``: stage kernels 1..6 each followed by a network evaluation (the last stage is y_new),
    the error partials, the controller and the commit; nothing in it allocates outside the network or synchronises, so
    ``_Dopri5Graph`` captures it whole.  The host reads the 16-byte status word once per attempted step (a non-blocking
    copy into pinned memory and an event), and the per-sample state once at the end."""

    def __init__(self, net, x_like: torch.Tensor, atol: float, rtol: float, max_steps: int):
        if not x_like.is_cuda:
            raise RuntimeError("stain2stain_amd: the per-sample dopri5 solver needs GPU tensors (there is no CPU path)")
        if x_like.dtype != torch.float32 or x_like.numel() == 0 or (x_like[0].numel() % 4):
            raise RuntimeError("stain2stain_amd: per-sample dopri5 wants fp32 samples of a multiple of 4 elements")
        dev, B = x_like.device, x_like.shape[0]
        self.net, self.atol, self.rtol, self.max_steps = net, float(atol), float(rtol), int(max_steps)
        self.B, self.n = B, x_like[0].numel()
        e = lambda: torch.empty_like(x_like, memory_format=torch.contiguous_format)
        self.y, self.k1, self.xs, self.y_new = e(), e(), e(), e()
        self.t = torch.empty((B,), dtype=torch.float32, device=dev)
        self.state = torch.empty((B, 8), dtype=torch.float64, device=dev)
        self.part = torch.empty((2 * B * ops.dp_partials(self.n),), dtype=torch.float64, device=dev)
        self.status = torch.empty((4,), dtype=torch.int32, device=dev)
        self.status_host = torch.empty((4,), dtype=torch.int32, pin_memory=True)
        self.state_host = torch.empty((B, 8), dtype=torch.float64, pin_memory=True)
        self.event = torch.cuda.Event()
        self.host_reads = 0

    def f(self, x: torch.Tensor) -> torch.Tensor:
        return self.net(self.t, x).contiguous()

    def init(self, source: torch.Tensor) -> None:
        """y = source, k1 = v(0, y), Hairer's initial step per sample (two evaluations)."""
        self.y.copy_(source)
        self.t.zero_()
        self.k1.copy_(self.f(self.y))
        ops.dp_init_(0, self.y, self.k1, None, self.state, self.part, self.xs, self.t, self.status, self.atol, self.rtol)
        fa = self.f(self.xs)
        ops.dp_init_(1, self.y, self.k1, fa, self.state, self.part, self.xs, self.t, self.status, self.atol, self.rtol)

    def step(self):
        """One attempted step of every sample; returns k1..k7 (k2..k7 the network's own outputs)."""
        ks = [self.k1]
        for i in range(1, 7):
            out = self.y_new if i == 6 else self.xs
            ops.dp_stage_(i, self.y, ks, self.state, out, self.t)
            ks.append(self.f(out))
        ops.dp_error_(ks, self.y, self.y_new, self.state, self.part, self.atol, self.rtol)
        ops.dp_control_(self.state, self.part, self.status, min(self.max_steps, 2 ** 31 - 1), self.B, self.n)
        ops.dp_commit_(self.y, self.y_new, self.k1, ks[6], self.state)
        return ks

    def _read(self, dev: torch.Tensor, host: torch.Tensor) -> torch.Tensor:
        host.copy_(dev, non_blocking=True)
        self.event.record()
        self.event.synchronize()
        self.host_reads += 1
        return host

    def solve(self, source: torch.Tensor, return_stats: bool, replay=None):
        if self.max_steps < 1:
            raise RuntimeError("dopri5_generate: max_steps reached before t = 1")
        self.host_reads = 0
        self.init(source)
        attempted = 0
        while True:
            if replay is None:
                self.step()
            else:
                replay()
            attempted += 1
            active, limit = self._read(self.status, self.status_host).tolist()[:2]
            if limit:
                raise RuntimeError("dopri5_generate: max_steps reached before t = 1")
            if active == 0:
                break
        y = self.y if replay is None else self.y.clone()
        if not return_stats:
            return y
        st = self._read(self.state, self.state_host)
        return y, {"accepted": [int(v) for v in st[:, 2].tolist()], "rejected": [int(v) for v in st[:, 3].tolist()],
                   "attempted": attempted, "evaluations": 2 + 6 * attempted, "host_reads": self.host_reads}


class _GraphedStep:
    """One step of a solve captured as a hipGraph on one stream, and everything its three kinds share: the key a cache
    compares, the warm-up, the capture and the lifetime.  A subclass names its ``slot`` (the attribute a cache keeps it
    under), builds its buffers in ``_buffers(x_like, *settings)`` -- which returns the ``(t, x)`` the warm-up forward
    runs on -- issues one step in ``_step()`` (what it returns is kept as ``self.out``: the network outputs the capture
    allocated) and replays it in ``solve``.

    Everything the forward touches has a fixed address inside the capture (torch's graph-private memory pool owns the
    intermediates; weights, packed operands and folded BatchNorm constants are warmed up before capture), so a replay
    recomputes the same kernels on whatever the buffers currently hold.  The network must be in eval mode and its
    parameters must not change while the graph is alive: ``matches`` tells a cache when to rebuild."""

    slot: str

    def __init__(self, net, x_like: torch.Tensor, *settings):
        self.net, self.holder = net, None
        self.key = self._key(net, x_like, settings)
        t, x = self._buffers(x_like, *settings)
        side = torch.cuda.Stream(device=x_like.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                   # warm-up: packed weights, folded BN constants, LDS attributes
            for _ in range(2):
                net(t, x)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with ops.capture_graph(self.graph):
            self.out = self._step()

    @staticmethod
    def _key(net, x, settings):
        from . import engine
        return tuple(x.shape), settings, engine.mutation_epoch[0], tuple(p._version for p in _params(net))

    def matches(self, net, x: torch.Tensor, *settings) -> bool:
        return self.graph is not None and net is self.net and self.key == self._key(net, x, settings)

    @classmethod
    def cached(cls, holder, net, x: torch.Tensor, *settings):
        """The instance kept as ``holder.<slot>``, captured again when it no longer ``matches``."""
        g = getattr(holder, cls.slot, None)
        if g is None or not g.matches(net, x, *settings):
            if g is not None:
                g.close()                  # the superseded graph goes now, not whenever the cyclic collector finds it
            g = cls(net, x, *settings)
            try:
                object.__setattr__(holder, cls.slot, g)         # a plain attribute, not a registered sub-module
                g.holder = holder
            except Exception:  # noqa: BLE001 -- a callable that takes no attributes: rebuild next time
                pass
        return g

    def _replay(self, times: int = 1) -> None:
        if self.graph is None:
            raise RuntimeError("stain2stain_amd: this captured step has been closed")
        for _ in range(times):
            self.graph.replay()

    def close(self) -> None:
        """Release the graph and its private pool now (a cached instance sits in a cycle with its network; see
        CFMTrainer.close)."""
        self.graph = self.out = None
        if getattr(self.holder, self.slot, None) is self:
            try:
                object.__delattr__(self.holder, self.slot)
            except Exception:  # noqa: BLE001
                pass


class GraphedVelocity(_GraphedStep):
    """``v = net(t, x)`` as a replayed hipGraph (one ``hipGraphLaunch`` per evaluation instead of ~60 kernel launches).

    The reference samples ONE tile at a time (src/infer_simple_flowmatching.py:73-83); at batch 1 the eval-mode forward
    is ~60 short kernels and the eager path is bound by host launch time (~2.3 ms of launches per evaluation, round-1
    measurement).

    With ``dt`` the capture is a whole Euler step -- ``t <- t_k`` (device-side table walk), ``v``, ``x += dt * v``: a
    whole fixed-step solve is then ``num_steps`` graph launches and nothing else (``solve``; cached as
    ``net._s2s_euler_graph`` until the batch shape, ``dt``, the parameters or ``engine.mutation_epoch`` change).  Without
    it the object is called like the network, which is how the batch-wide dopri5 loop evaluates its stages."""

    slot = "_s2s_euler_graph"

    def __init__(self, net, x_like: torch.Tensor, dt: Optional[float] = None):
        super().__init__(net, x_like, dt)

    def _buffers(self, x_like: torch.Tensor, dt: Optional[float]):
        if not x_like.is_cuda:
            raise RuntimeError("stain2stain_amd: GraphedVelocity needs GPU tensors (there is no CPU path)")
        self.dt = dt
        self.x = _prep_source(x_like)
        self.t = torch.zeros((x_like.shape[0],), dtype=torch.float32, device=x_like.device)
        if dt is not None:
            # node times exactly as the eager loop forms them (k * dt in double, rounded once); the captured step
            # reads table[counter] and advances the counter on the device
            n = int(round(1.0 / dt))
            self._table = torch.tensor([k * dt for k in range(n + 2)], dtype=torch.float32, device=x_like.device)
            self._counter = torch.zeros((1,), dtype=torch.int32, device=x_like.device)
        return self.t, self.x

    def _step(self) -> torch.Tensor:
        if self.dt is not None:
            ops.euler_tick_(self.t, self._table, self._counter)
        v = self.net(self.t, self.x).contiguous()
        if self.dt is not None:
            ops.axpy_(self.x, v, self.dt)
        return v

    def __call__(self, t: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """v(t, x): copies the arguments into the graph's buffers, replays, returns the graph's output buffer (valid
        until the next call)."""
        self.x.copy_(x)
        self.t.copy_(t.to(torch.float32).expand(self.t.shape[0]) if t.dim() <= 1 and t.numel() == 1 else t)
        self._replay()
        return self.out

    def solve(self, source: torch.Tensor, num_steps: int) -> torch.Tensor:
        if self.dt is None or abs(self.dt * num_steps - 1.0) > 1e-9:
            raise ValueError("this graph was captured for a different step size")
        self.x.copy_(source)
        self._counter.zero_()
        self._replay(num_steps)
        return self.x.clone()

    solve_euler = solve                    # the name it had before every captured step had a ``solve``


class _FixedStepGraph(_GraphedStep):
    """One whole step of ``_FixedStepRK`` (no forked branches): the s evaluations, the stage launches and the combine;
    the k_j are the network outputs the capture allocated, read in place.  A solve is ``num_steps`` replays.  Cached on
    the network as ``net._s2s_rk_graph`` until the batch shape, ``num_steps``, the method, the parameters or
    ``engine.mutation_epoch`` change; ``close()`` releases it."""

    slot = "_s2s_rk_graph"

    def _buffers(self, x_like: torch.Tensor, num_steps: int, method: str):
        self.solver = s = _FixedStepRK(self.net, _prep_source(x_like), num_steps, method)
        return s.t, s.x

    def _step(self):
        return self.solver.step()

    def solve(self, source: torch.Tensor) -> torch.Tensor:
        s = self.solver
        s.x.copy_(source)
        s.counter.zero_()
        self._replay(s.num_steps)
        return s.x.clone()


class _Dopri5Graph(_GraphedStep):
    """One attempted step of ``_PerSampleDopri5`` (no forked branches): the stage inputs, y_new, k1 and the state live in
    the solver's buffers; k2..k7 are the network outputs the capture allocated, read in place.  Cached on the network as
    ``net._s2s_dopri5_graph`` until the batch shape, the tolerances, the step limit, the parameters or
    ``engine.mutation_epoch`` change; ``close()`` releases it."""

    slot = "_s2s_dopri5_graph"

    def _buffers(self, x_like: torch.Tensor, atol: float, rtol: float, max_steps: int):
        self.solver = s = _PerSampleDopri5(self.net, x_like, atol, rtol, max_steps)
        s.t.zero_()
        s.xs.copy_(x_like)
        return s.t, s.xs

    def _step(self):
        return self.solver.step()

    def solve(self, source: torch.Tensor, return_stats: bool = False):
        return self.solver.solve(source, return_stats, replay=self._replay)


def close_cached(holder) -> None:
    """Close every captured step ``_GraphedStep.cached`` keeps on ``holder`` (whatever kinds exist)."""
    for kind in _GraphedStep.__subclasses__():
        g = getattr(holder, kind.slot, None)
        if g is not None:
            g.close()


def solve(f, x: torch.Tensor, method: str, num_steps: Optional[int] = None, atol: float = 1e-4, rtol: float = 1e-4,
          max_steps: int = 1000, graph: bool = False, per_sample: bool = False, return_stats: bool = False,
          cache_on=None):
    """x(1) for a callable ``f(t[B], x)`` from a prepared ``x`` (``_prep_source``), by ``method`` (``SOLVER_METHODS``):
    the one place that maps (method, graph, per_sample) to a solver.  ``num_steps`` counts for the fixed-step methods,
    ``atol`` / ``rtol`` / ``max_steps`` / ``return_stats`` / ``per_sample`` for dopri5.  ``graph=True`` replays a
    captured step: kept as an attribute of ``cache_on`` from one call to the next when that is given (see
    ``_GraphedStep.cached``), else captured for this solve and closed when it ends.  The velocity-only capture under the
    batch-wide dopri5 loop is never kept.  The caller sets the network's mode and the grad mode."""
    if method == "dopri5":
        if not graph:
            return dopri5_integrate(f, x, atol, rtol, max_steps, return_stats, per_sample)
        if not per_sample:                              # every stage evaluation = one replay of the captured forward
            gv = GraphedVelocity(f, x, None)
            try:
                return dopri5_integrate(lambda t, y: gv(t, y).clone(), x, atol, rtol, max_steps, return_stats)
            finally:
                gv.close()
        kind, settings, args = _Dopri5Graph, (atol, rtol, max_steps), (return_stats,)
    elif per_sample:
        raise ValueError("per_sample=True needs the dopri5 solver")
    elif method == "euler":                             # its own kernels, not the one-stage tableau
        if not graph:
            return euler_integrate(f, x, num_steps)
        kind, settings, args = GraphedVelocity, (1.0 / num_steps,), (num_steps,)
    else:
        if not graph:
            return fixed_step_integrate(f, x, num_steps, method)
        kind, settings, args = _FixedStepGraph, (num_steps, method), ()
    g = kind(f, x, *settings) if cache_on is None else kind.cached(cache_on, f, x, *settings)
    try:
        return g.solve(x, *args)
    finally:
        if cache_on is None:
            g.close()


@torch.no_grad()
def euler_generate(net, source_img: torch.Tensor, num_steps: int = 50, graph: bool = False) -> torch.Tensor:
    """x(0) = source, x <- x + v(t_k, x)/n at t_k = k/n, network in eval mode (its mode is restored); returns x(1).
    ``graph=True`` replays one captured Euler step ``num_steps`` times (GraphedVelocity; cached on the network until its
    parameters, the batch shape or the step size change): same kernels, same results, no per-kernel launch cost."""
    with _eval_mode(net):
        return solve(net, _prep_source(source_img), "euler", num_steps, graph=graph, cache_on=net)


@torch.no_grad()
def fixed_step_generate(net, source_img: torch.Tensor, num_steps: int, method: str = "rk4",
                        graph: bool = False) -> torch.Tensor:
    """x(0) = source, ``num_steps`` steps of the Runge-Kutta scheme ``method`` (``FIXED_STEP_METHODS``) to t = 1, network
    in eval mode (its mode is restored); returns x(1).  ``graph=True`` replays one captured whole step ``num_steps``
    times (``_FixedStepGraph``, cached on the network until its parameters, the batch shape, ``num_steps`` or the method
    change): same kernels, same results.  ``method="euler"`` is ``euler_generate``."""
    num_steps = _check_fixed_step(method, num_steps)
    with _eval_mode(net):
        return solve(net, _prep_source(source_img), method, num_steps, graph=graph, cache_on=net)


@torch.no_grad()
def dopri5_generate(net, source_img: torch.Tensor, atol: float = 1e-4, rtol: float = 1e-4, max_steps: int = 1000,
                    return_stats: bool = False, graph: bool = False, per_sample: bool = False):
    """``dopri5_integrate`` on a network put in eval mode for the solve (mode restored, also when it raises).
    ``graph=True``: every stage evaluation is a replay of one captured forward (GraphedVelocity); with
    ``per_sample=True`` one whole attempted step (6 stage kernels, 6 evaluations, error, control, commit) is one replayed
    capture, cached on the network like the Euler graph (``net._s2s_dopri5_graph``)."""
    with _eval_mode(net):
        return solve(net, _prep_source(source_img), "dopri5", None, atol, rtol, max_steps, graph, per_sample,
                     return_stats, cache_on=net)
