"""Flow-matching step logic around the network, mirroring the reference's LightningModule surface.

  reference                                                               here
  ----------------------------------------------------------------------  ---------------------------
  torchcfm.ConditionalFlowMatcher.sample_location_and_conditional_flow    ConditionalFlowMatcher
    (third-party, call site src/models/conditional_flow_matching.py:66)
  ConditionalFlowMatchingLitModule.model_step / training_step /           ConditionalFlowMatchingModule
    configure_optimizers / generate (conditional_flow_matching.py:53-170)
  NeuralODE(dopri5).trajectory in generate (:157-170, torchdyn, absent)   euler_generate (fixed step,
                                                                          BASELINE.json config 4)

``ConditionalFlowMatchingModule`` subclasses ``lightning.LightningModule`` when Lightning is
importable and ``torch.nn.Module`` otherwise (this image has no Lightning), with the same method
names, argument meaning and return values, so the reference's training loop can drive it.
"""
from __future__ import annotations

from fractions import Fraction as _Fr
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import evaluation, ops

try:  # pragma: no cover - Lightning is not installed in the build image
    from lightning import LightningModule as _Base
except Exception:  # noqa: BLE001
    class _Base(torch.nn.Module):
        def log(self, *args, **kwargs) -> None:
            pass


class ConditionalFlowMatcher:
    """Independent-coupling conditional flow matching: xt = t x1 + (1-t) x0 + sigma eps, ut = x1 - x0."""

    def __init__(self, sigma: float = 0.0):
        self.sigma = float(sigma)

    def sample_location_and_conditional_flow(self, x0: torch.Tensor, x1: torch.Tensor,
                                             t: Optional[torch.Tensor] = None, return_noise: bool = False):
        if t is None:
            t = torch.rand(x0.shape[0], device=x0.device, dtype=torch.float32)
        eps = torch.randn_like(x0) if (self.sigma != 0.0 or return_noise) else None
        xt, ut = ops.cfm_sample(x0.contiguous().float(), x1.contiguous().float(), t.contiguous().float(),
                                self.sigma, eps)
        return (t, xt, ut, eps) if return_noise else (t, xt, ut)


class _MSE(torch.autograd.Function):
    """mean((v-u)^2) with the fused loss/gradient kernel."""

    @staticmethod
    def forward(ctx, v: torch.Tensor, u: torch.Tensor):
        loss, dv = ops.mse_loss(v.detach().contiguous(), u.detach().contiguous(), want_grad=True)
        ctx.save_for_backward(dv)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        (dv,) = ctx.saved_tensors
        return dv * gloss, None


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


@torch.no_grad()
def euler_generate(net, source_img: torch.Tensor, num_steps: int = 50, graph: bool = False) -> torch.Tensor:
    """x(0) = source, x <- x + v(t_k, x)/n at t_k = k/n, network in eval mode (its mode is restored); returns x(1).
    ``graph=True`` replays one captured Euler step ``num_steps`` times (GraphedVelocity; cached on the network until its
    parameters, the batch shape or the step size change): same kernels, same results, no per-kernel launch cost."""
    with _eval_mode(net):
        x = _prep_source(source_img)
        if not graph:
            return euler_integrate(net, x, num_steps)
        dt = 1.0 / num_steps
        g = getattr(net, "_s2s_euler_graph", None)
        if g is None or not g.matches(net, x, dt):
            if g is not None:
                g.close()                  # the superseded graph goes now, not whenever the cyclic collector finds it
            g = GraphedVelocity(net, x, dt)
            try:
                object.__setattr__(net, "_s2s_euler_graph", g)      # a plain attribute, not a registered sub-module
            except Exception:  # noqa: BLE001 -- a callable that takes no attributes: rebuild next time
                pass
        return g.solve_euler(x, num_steps)


class GraphedVelocity:
    """``v = net(t, x)`` as a replayed hipGraph (one ``hipGraphLaunch`` per evaluation instead of ~60 kernel launches).

    The reference samples ONE tile at a time (src/infer_simple_flowmatching.py:73-83); at batch 1 the eval-mode forward
    is ~60 short kernels and the eager path is bound by host launch time (~2.3 ms of launches per evaluation, round-1
    measurement).  Everything the forward touches has a fixed address inside the capture (torch's graph-private memory
    pool owns the intermediates; weights, packed operands and folded BatchNorm constants are warmed up before capture),
    so a replay recomputes the same kernels on whatever ``t`` / ``x`` currently hold.

    With ``dt`` the capture is a whole Euler step -- ``t <- t_k`` (device-side table walk), ``v``, ``x += dt * v``: a whole fixed-step solve is then ``num_steps``
    graph launches and nothing else.  The network must be in eval mode and its parameters must not change while the
    graph is alive (``GraphedVelocity.matches`` tells a cache when to rebuild)."""

    def __init__(self, net, x_like: torch.Tensor, dt: Optional[float] = None):
        if not x_like.is_cuda:
            raise RuntimeError("stain2stain_amd: GraphedVelocity needs GPU tensors (there is no CPU path)")
        from . import engine
        B = x_like.shape[0]
        self.net, self.dt = net, dt
        self.key = (tuple(x_like.shape), dt, engine.mutation_epoch[0], tuple(p._version for p in _params(net)))
        self.x = x_like.detach().float().contiguous().clone()
        self.t = torch.zeros((B,), dtype=torch.float32, device=x_like.device)
        if dt is not None:
            # node times exactly as the eager loop forms them (k * dt in double, rounded once); the captured step
            # reads table[counter] and advances the counter on the device
            n = int(round(1.0 / dt))
            self._table = torch.tensor([k * dt for k in range(n + 2)], dtype=torch.float32, device=x_like.device)
            self._counter = torch.zeros((1,), dtype=torch.int32, device=x_like.device)
        side = torch.cuda.Stream(device=x_like.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                   # warm-up: packed weights, folded BN constants, LDS attributes
            for _ in range(2):
                net(self.t, self.x)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with ops.capture_graph(self.graph):
            if dt is not None:
                ops.euler_tick_(self.t, self._table, self._counter)
            self.v = net(self.t, self.x).contiguous()
            if dt is not None:
                ops.axpy_(self.x, self.v, dt)

    def close(self) -> None:
        """Release the graph and its private pool now (the object sits in a cycle with its network through
        ``net._s2s_euler_graph``; see CFMTrainer.close)."""
        self.graph = None
        self.v = None
        if getattr(self.net, "_s2s_euler_graph", None) is self:
            try:
                object.__delattr__(self.net, "_s2s_euler_graph")
            except Exception:  # noqa: BLE001
                pass

    def matches(self, net, x: torch.Tensor, dt: Optional[float]) -> bool:
        from . import engine
        return net is self.net and self.key == (tuple(x.shape), dt, engine.mutation_epoch[0],
                                                tuple(p._version for p in _params(net)))

    def __call__(self, t: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """v(t, x): copies the arguments into the graph's buffers, replays, returns the graph's output buffer (valid
        until the next call)."""
        self.x.copy_(x)
        self.t.copy_(t.to(torch.float32).expand(self.t.shape[0]) if t.dim() <= 1 and t.numel() == 1 else t)
        self.graph.replay()
        return self.v

    def solve_euler(self, source: torch.Tensor, num_steps: int) -> torch.Tensor:
        if self.dt is None or abs(self.dt * num_steps - 1.0) > 1e-9:
            raise ValueError("this graph was captured for a different step size")
        self.x.copy_(source)
        self._counter.zero_()
        for _ in range(num_steps):
            self.graph.replay()
        return self.x.clone()


def _params(net):
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


class _FixedStepGraph:
    """One whole step of ``_FixedStepRK`` captured as a hipGraph on one stream (no forked branches): the s evaluations,
    the stage launches and the combine; the k_j are the network outputs the capture allocated, read in place.  A solve
    is ``num_steps`` replays.  Cached on the network as ``net._s2s_rk_graph`` until the batch shape, ``num_steps``, the
    method, the parameters or ``engine.mutation_epoch`` change; ``close()`` releases it."""

    def __init__(self, net, x_like: torch.Tensor, num_steps: int, method: str):
        self.net = net
        self.key = self._key(net, x_like, num_steps, method)
        self.solver = s = _FixedStepRK(net, x_like.detach().float().contiguous().clone(), num_steps, method)
        side = torch.cuda.Stream(device=x_like.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                   # warm-up: packed weights, folded BN constants, LDS attributes
            for _ in range(2):
                net(s.t, s.x)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with ops.capture_graph(self.graph):
            self.ks = s.step()

    @staticmethod
    def _key(net, x, num_steps, method):
        from . import engine
        return (tuple(x.shape), int(num_steps), str(method), engine.mutation_epoch[0],
                tuple(p._version for p in _params(net)))

    def matches(self, net, x, num_steps, method) -> bool:
        return self.graph is not None and net is self.net and self.key == self._key(net, x, num_steps, method)

    def solve(self, source: torch.Tensor) -> torch.Tensor:
        if self.graph is None:
            raise RuntimeError("stain2stain_amd: this fixed-step graph has been closed")
        s = self.solver
        s.x.copy_(source)
        s.counter.zero_()
        for _ in range(s.num_steps):
            self.graph.replay()
        return s.x.clone()

    def close(self) -> None:
        """Release the graph and its private pool now (it sits in a cycle with its network)."""
        self.graph = None
        self.ks = None
        if getattr(self.net, "_s2s_rk_graph", None) is self:
            try:
                object.__delattr__(self.net, "_s2s_rk_graph")
            except Exception:  # noqa: BLE001
                pass


def _cached_fixed_step_graph(net, x: torch.Tensor, num_steps: int, method: str) -> _FixedStepGraph:
    g = getattr(net, "_s2s_rk_graph", None)
    if g is None or not g.matches(net, x, num_steps, method):
        if g is not None:
            g.close()                      # the superseded graph goes now, not whenever the cyclic collector finds it
        g = _FixedStepGraph(net, x, num_steps, method)
        try:
            object.__setattr__(net, "_s2s_rk_graph", g)        # a plain attribute, not a registered sub-module
        except Exception:  # noqa: BLE001 -- a callable that takes no attributes: rebuild next time
            pass
    return g


@torch.no_grad()
def fixed_step_generate(net, source_img: torch.Tensor, num_steps: int, method: str = "rk4",
                        graph: bool = False) -> torch.Tensor:
    """x(0) = source, ``num_steps`` steps of the Runge-Kutta scheme ``method`` (``FIXED_STEP_METHODS``) to t = 1, network
    in eval mode (its mode is restored); returns x(1).  ``graph=True`` replays one captured whole step ``num_steps``
    times (``_FixedStepGraph``, cached on the network until its parameters, the batch shape, ``num_steps`` or the method
    change): same kernels, same results.  ``method="euler"`` is ``euler_generate``."""
    num_steps = _check_fixed_step(method, num_steps)
    if method == "euler":
        return euler_generate(net, source_img, num_steps, graph=graph)
    with _eval_mode(net):
        x = _prep_source(source_img)
        if not graph:
            return fixed_step_integrate(net, x, num_steps, method)
        return _cached_fixed_step_graph(net, x, num_steps, method).solve(x)


@torch.no_grad()
def dopri5_generate(net, source_img: torch.Tensor, atol: float = 1e-4, rtol: float = 1e-4, max_steps: int = 1000,
                    return_stats: bool = False, graph: bool = False, per_sample: bool = False):
    """``dopri5_integrate`` on a network put in eval mode for the solve (mode restored, also when it raises).
    ``graph=True``: every stage evaluation is a replay of one captured forward (GraphedVelocity); with
    ``per_sample=True`` one whole attempted step (6 stage kernels, 6 evaluations, error, control, commit) is one replayed
    capture, cached on the network like the Euler graph (``net._s2s_dopri5_graph``)."""
    with _eval_mode(net):
        x = _prep_source(source_img)
        if per_sample:
            if not graph:
                return dopri5_integrate(net, x, atol, rtol, max_steps, return_stats, per_sample=True)
            return _cached_dopri5_graph(net, x, atol, rtol, max_steps).solve(x, return_stats)
        if not graph:
            return dopri5_integrate(net, x, atol, rtol, max_steps, return_stats)
        gv = GraphedVelocity(net, x, None)
        try:
            return dopri5_integrate(lambda t, y: gv(t, y).clone(), x, atol, rtol, max_steps, return_stats)
        finally:
            gv.close()


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


class _Dopri5Graph:
    """One attempted step of ``_PerSampleDopri5`` captured as a hipGraph on one stream (no forked branches): the stage
    inputs, y_new, k1 and the state live in the solver's buffers; k2..k7 are the network outputs the capture allocated,
    read in place.  Cached on the network as ``net._s2s_dopri5_graph`` until the batch shape, the tolerances, the step
    limit, the parameters or ``engine.mutation_epoch`` change; ``close()`` releases it."""

    def __init__(self, net, x_like: torch.Tensor, atol: float, rtol: float, max_steps: int):
        self.net = net
        self.key = self._key(net, x_like, atol, rtol, max_steps)
        self.solver = s = _PerSampleDopri5(net, x_like, atol, rtol, max_steps)
        s.t.zero_()
        s.xs.copy_(x_like)
        side = torch.cuda.Stream(device=x_like.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                   # warm-up: packed weights, folded BN constants, LDS attributes
            for _ in range(2):
                net(s.t, s.xs)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with ops.capture_graph(self.graph):
            self.ks = s.step()

    @staticmethod
    def _key(net, x, atol, rtol, max_steps):
        from . import engine
        return (tuple(x.shape), float(atol), float(rtol), int(max_steps), engine.mutation_epoch[0],
                tuple(p._version for p in _params(net)))

    def matches(self, net, x, atol, rtol, max_steps) -> bool:
        return self.graph is not None and net is self.net and self.key == self._key(net, x, atol, rtol, max_steps)

    def solve(self, source: torch.Tensor, return_stats: bool = False):
        return self.solver.solve(source, return_stats, replay=self.graph.replay)

    def close(self) -> None:
        """Release the graph and its private pool now (it sits in a cycle with its network)."""
        self.graph = None
        self.ks = None
        if getattr(self.net, "_s2s_dopri5_graph", None) is self:
            try:
                object.__delattr__(self.net, "_s2s_dopri5_graph")
            except Exception:  # noqa: BLE001
                pass


def _cached_dopri5_graph(net, x: torch.Tensor, atol: float, rtol: float, max_steps: int) -> _Dopri5Graph:
    g = getattr(net, "_s2s_dopri5_graph", None)
    if g is None or not g.matches(net, x, atol, rtol, max_steps):
        if g is not None:
            g.close()
        g = _Dopri5Graph(net, x, atol, rtol, max_steps)
        try:
            object.__setattr__(net, "_s2s_dopri5_graph", g)    # a plain attribute, not a registered sub-module
        except Exception:  # noqa: BLE001 -- a callable that takes no attributes: rebuild next time
            pass
    return g


class SolverConfig:
    """Stand-in for the reference's ``solver:`` entry (a partial of torchdyn's ``NeuralODE``,
    configs/model/conditional_flow_matching.yaml:32-38): the attributes ``generate`` reads from it."""

    def __init__(self, solver: str = "dopri5", sensitivity: str = "adjoint", atol: float = 1e-4, rtol: float = 1e-4):
        self.solver, self.sensitivity, self.atol, self.rtol = solver, sensitivity, atol, rtol


def _solver_setting(solver, name: str, default):
    """``solver.<name>`` as the reference reads it (conditional_flow_matching.py:158-163: attribute if present, else
    the default); the keyword of a ``functools.partial`` -- what Hydra's ``_partial_: true`` builds -- is honoured too."""
    if hasattr(solver, name):
        return getattr(solver, name)
    kw = getattr(solver, "keywords", None)
    if isinstance(kw, dict) and name in kw:
        return kw[name]
    return default


def _solver_method(solver, method: Optional[str] = None) -> str:
    """The solver name a ``generate`` call runs: ``method`` when given, else ``solver.solver`` (attribute or keyword of a
    partial), else dopri5; a name outside ``SOLVER_METHODS`` raises ValueError before anything touches the GPU."""
    method = method or _solver_setting(solver, "solver", "dopri5")
    if not isinstance(method, str) or method not in SOLVER_METHODS:
        raise ValueError(f"solver method must be one of {', '.join(map(repr, SOLVER_METHODS))}, got {method!r}")
    return method


def _solve(module, f, source_img: torch.Tensor, num_steps: int, method: Optional[str], atol: Optional[float],
           rtol: Optional[float], graph: bool = False, per_sample: bool = False) -> torch.Tensor:
    """The ODE solve shared by every ``generate``: like the reference it refuses to run without a solver, puts the
    module in eval mode and LEAVES it there (``self.eval()``, conditional_flow_matching.py:147-150), integrates with
    the solver's method / tolerances (dopri5, 1e-4 when it names none) and returns the end point x(1).  ``method``
    overrides the solver's choice: "euler" is the ``num_steps`` fixed-step solve of BASELINE.json configs[3], the other
    names of ``FIXED_STEP_METHODS`` ("midpoint", "heun", "rk4", "rk4_38") ``num_steps`` steps of that Runge-Kutta scheme.
    ``per_sample=True`` (dopri5 only): every sample gets its own step size, so it does not depend on its batch mates."""
    if module.solver is None:
        raise ValueError("Solver is not initialized. Cannot perform inference.")
    module.eval()
    method = _solver_method(module.solver, method)
    atol = _solver_setting(module.solver, "atol", 1e-4) if atol is None else atol
    rtol = _solver_setting(module.solver, "rtol", 1e-4) if rtol is None else rtol
    x = _prep_source(source_img)
    if method == "dopri5":
        if per_sample:
            if not graph:
                return dopri5_integrate(f, x, atol, rtol, per_sample=True)
            g = _Dopri5Graph(f, x, atol, rtol, 1000)
            try:
                return g.solve(x)
            finally:
                g.close()
        if graph:           # every stage evaluation = one replay of the captured forward
            gv = GraphedVelocity(f, x, None)
            return dopri5_integrate(lambda t, y: gv(t, y).clone(), x, atol, rtol)
        return dopri5_integrate(f, x, atol, rtol)
    if per_sample:
        raise ValueError("per_sample=True needs the dopri5 solver")
    if method == "euler":
        if graph:
            return GraphedVelocity(f, x, 1.0 / num_steps).solve_euler(x, num_steps)
        return euler_integrate(f, x, num_steps)
    if isinstance(method, str) and method in _RK_TABLEAUS:
        if not graph:
            return fixed_step_integrate(f, x, num_steps, method)
        g = _FixedStepGraph(f, x, num_steps, method)
        try:
            return g.solve(x)
        finally:
            g.close()
    raise ValueError(f"solver method must be one of {', '.join(map(repr, SOLVER_METHODS))}, got {method!r}")


class ConditionalFlowMatchingModule(_Base):
    """Same surface as the reference's ConditionalFlowMatchingLitModule (logging hooks left out)."""

    def __init__(self, net: torch.nn.Module, flow_matcher: Optional[ConditionalFlowMatcher] = None, solver=None,
                 optimizer=None, scheduler=None, compile: bool = False, log_images: bool = False,
                 n_images_log: int = 5):
        super().__init__()
        self.net = net
        self.flow_matcher = flow_matcher or ConditionalFlowMatcher(0.0)
        self.solver, self.optimizer, self.scheduler = solver, optimizer, scheduler
        self.log_images, self.n_images_log = log_images, n_images_log

    def forward(self, t: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        return self.net(t, x)

    def model_step(self, batch: Tuple[torch.Tensor, ...]) -> torch.Tensor:
        x0, x1 = batch[:2]
        t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(x0, x1)
        vt = self.forward(t, xt)
        return _MSE.apply(vt, ut)

    def training_step(self, batch, batch_idx: int) -> torch.Tensor:
        loss = self.model_step(batch)
        self.log("train/loss", loss, on_step=True, on_epoch=True, prog_bar=True, sync_dist=True)
        return loss

    def validation_step(self, batch, batch_idx: int) -> None:
        self.log("val/loss", self.model_step(batch), on_step=False, on_epoch=True, prog_bar=True, sync_dist=True)

    def test_step(self, batch, batch_idx: int) -> None:
        self.log("test/loss", self.model_step(batch), on_step=False, on_epoch=True, prog_bar=True, sync_dist=True)

    def configure_optimizers(self) -> Dict[str, Any]:
        optimizer = self.optimizer(params=self.parameters())
        if self.scheduler is not None:
            return {"optimizer": optimizer,
                    "lr_scheduler": {"scheduler": self.scheduler(optimizer=optimizer), "monitor": "val/loss",
                                     "interval": "epoch", "frequency": 1}}
        return {"optimizer": optimizer}

    @torch.no_grad()
    def generate(self, source_img: torch.Tensor, num_steps: int = 100, method: Optional[str] = None,
                 atol: Optional[float] = None, rtol: Optional[float] = None, graph: bool = False,
                 per_sample: bool = False) -> torch.Tensor:
        """x(1) of dx/dt = net(t, x), x(0) = source (conditional_flow_matching.py:133-170): the solver's method --
        adaptive dopri5 at atol = rtol = 1e-4 unless ``self.solver`` says otherwise; ``num_steps`` only defined the
        reference's output grid and plays no role for the end point -- or, with ``method="euler"``, ``num_steps``
        fixed Euler steps.  Raises without a solver and leaves the module in eval mode, as the reference does.
        ``graph=True`` replays the network evaluation as a captured hipGraph (the reference samples one tile at a time,
        infer_simple_flowmatching.py:73-83, where the eager path is launch-bound).  ``per_sample=True``: dopri5 with a
        step size per sample (``dopri5_integrate``), each result independent of its batch mates."""
        return _solve(self, self.net, source_img, num_steps, method, atol, rtol, graph, per_sample)


class _WeightedMSE(torch.autograd.Function):
    """sum(w (v-u)^2) / (sum(w) + 1e-8), w = 1 + lam * mask, with the fused loss/gradient kernels."""

    @staticmethod
    def forward(ctx, v: torch.Tensor, u: torch.Tensor, mask: torch.Tensor, lam: float):
        loss, dv = ops.weighted_mse(v.detach().float(), u.detach().float(), mask.detach(), lam, want_grad=True)
        ctx.save_for_backward(dv)
        return loss[0]

    @staticmethod
    def backward(ctx, gloss):
        (dv,) = ctx.saved_tensors
        return dv * gloss, None, None, None


class ROIWeightedFlowMatchingModule(ConditionalFlowMatchingModule):
    """conditional_flow_matching_masked.py:60-91 -- batches are (source, target, mask); pixels inside the mask
    count ``1 + roi_lambda`` times in the flow-matching MSE (``roi_lambda`` attribute, default 10 as :78)."""

    roi_lambda: float = 10.0

    def model_step(self, batch) -> torch.Tensor:
        x0, x1, mask = batch
        t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(x0, x1)
        return _WeightedMSE.apply(self.forward(t, xt), ut, mask, float(getattr(self, "roi_lambda", 10.0)))


class ROICharbonnierFlowMatchingModule(ConditionalFlowMatchingModule):
    """conditional_flow_matching_ROI_loss.py:64-97 -- flow-matching MSE plus ``lambda_roi`` times the Charbonnier
    distance between xt and x1 inside the mask (a data-only term: it shifts the logged loss, not the gradients)."""

    lambda_roi: float = 1.0

    def model_step(self, batch) -> torch.Tensor:
        x0, x1, mask = batch
        t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(x0, x1)
        loss_fm = _MSE.apply(self.forward(t, xt), ut)
        roi = ops.charbonnier_roi(xt, x1.float(), mask, 1e-3, 1e-8)[0]
        return loss_fm + float(getattr(self, "lambda_roi", 1.0)) * roi


class MaskConditionedFlowMatchingModule(ConditionalFlowMatchingModule):
    """conditional_flow_matching_conditional_mask.py:54-82 (``mask_toggle=False``) and
    conditional_flow_matching_conditional_toggle_mask.py:54-103 (``mask_toggle=True``: the training step zeroes the
    mask with probability 1/2, drawn with ``torch.rand(1).item()`` like the reference).  The mask is the fourth
    input channel of ``net`` (``in_channels: 4``)."""

    def __init__(self, *args, mask_toggle: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.mask_toggle = mask_toggle

    def forward(self, t: torch.Tensor, x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        return self.net(t, torch.cat([x, mask.to(x.dtype)], dim=1))

    def model_step(self, batch, use_mask_toggle: bool = False) -> torch.Tensor:
        x0, x1, mask = batch
        if use_mask_toggle and torch.rand(1).item() < 0.5:
            mask = torch.zeros_like(mask)
        t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(x0, x1)
        return _MSE.apply(self.forward(t, xt, mask), ut)

    def training_step(self, batch, batch_idx: int) -> torch.Tensor:
        loss = self.model_step(batch, use_mask_toggle=self.mask_toggle)
        self.log("train/loss", loss, on_step=True, on_epoch=True, prog_bar=True, sync_dist=True)
        return loss

    @torch.no_grad()
    def generate(self, source_img: torch.Tensor, mask: torch.Tensor, num_steps: int = 100,
                 method: Optional[str] = None, atol: Optional[float] = None, rtol: Optional[float] = None,
                 per_sample: bool = False) -> torch.Tensor:
        """conditional_flow_matching_conditional_mask.py:143-199: the mask rides along as a constant fourth channel."""
        if source_img.dim() == 3:
            source_img, mask = source_img.unsqueeze(0), mask.unsqueeze(0)
        return _solve(self, lambda t, x: self.forward(t, x, mask), source_img, num_steps, method, atol, rtol,
                      per_sample=per_sample)


class ClassConditionalFlowMatchingModule(ConditionalFlowMatchingModule):
    """class_conditional_flow_matching.py:39-71,130-190 -- batches are (source, target, target_label); the label
    conditions the network call ``net(t, x, y=y)``; ``generate(source, target_class, num_steps)``."""

    def forward(self, t: torch.Tensor, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return self.net(t, x, y=y)

    def model_step(self, batch) -> torch.Tensor:
        x0, x1, label = batch
        t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(x0, x1)
        return _MSE.apply(self.forward(t, xt, label.long()), ut)

    @torch.no_grad()
    def generate(self, source_img: torch.Tensor, target_class, num_steps: int = 100, method: Optional[str] = None,
                 atol: Optional[float] = None, rtol: Optional[float] = None, per_sample: bool = False) -> torch.Tensor:
        """class_conditional_flow_matching.py:130-190: ``target_class`` an int or a [B] tensor."""
        if source_img.dim() == 3:
            source_img = source_img.unsqueeze(0)
        B, dev = source_img.shape[0], source_img.device
        y = (torch.tensor([target_class] * B, device=dev) if isinstance(target_class, int)
             else target_class.to(dev))

        def f(t, x):
            return self.net(t, x, y=(y.expand(x.shape[0]) if y.dim() == 0 else y[:x.shape[0]]))

        return _solve(self, f, source_img, num_steps, method, atol, rtol, per_sample=per_sample)


class _SegLoss(torch.autograd.Function):
    """dw * Dice(sigmoid(z), g) + (1-dw) * BCEWithLogits(z, g) with the fused two-pass kernel."""

    @staticmethod
    def forward(ctx, z: torch.Tensor, g: torch.Tensor, smooth: float, dice_weight: float):
        out, dz = ops.seg_loss(z.detach().float(), g.detach(), smooth, dice_weight, want_grad=True)
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(out[1], out[2])
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, gseg, gdice, gbce):
        (dz,) = ctx.saved_tensors
        return dz * gseg, None, None, None


class _SegLossMulticlass(torch.autograd.Function):
    """dw * softmax-Dice + (1-dw) * CrossEntropy on class-index targets."""

    @staticmethod
    def forward(ctx, z: torch.Tensor, target: torch.Tensor, ignore_index: int, smooth: float, dice_weight: float):
        out, dz = ops.seg_loss_multiclass(z.detach().float(), target, ignore_index, smooth, dice_weight,
                                          want_grad=True)
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(out[1], out[2])
        return out[0], out[1], out[2]

    @staticmethod
    def backward(ctx, gseg, gdice, gce):
        (dz,) = ctx.saved_tensors
        return dz * gseg, None, None, None, None


class MultiTaskFlowMatchingModule(_Base):
    """Same surface as the reference's MultiTaskFlowMatchingLitModule
    (src/models/conditional_flow_matching_multitask.py:57-257,391-417): shared encoder, flow head A, mask head B,
    L = L_FM + seg_loss_weight * (dice_weight * Dice + (1 - dice_weight) * BCE).  Logging hooks left out."""

    def __init__(self, encoder, flow_decoder, seg_decoder, flow_matcher: Optional[ConditionalFlowMatcher] = None,
                 solver=None, optimizer=None, scheduler=None, compile: bool = False, log_images: bool = False,
                 seg_loss_weight: float = 1.0, dice_weight: float = 0.5, n_images_log: int = 5,
                 time_emb_dim: int = 256, num_classes: Optional[int] = None, ignore_index: int = -100):
        """``num_classes`` None: binary mask head, Dice + BCE (conditional_flow_matching_multitask.py).  An integer
        selects the multiclass form, softmax Dice + CrossEntropy on class-index masks
        (conditional_flow_matching_multitask_multiclassloss.py:92-159)."""
        super().__init__()
        self.num_classes, self.ignore_index = num_classes, ignore_index
        from .components import TimeEmbedding
        self.encoder, self.flow_decoder, self.seg_decoder = encoder, flow_decoder, seg_decoder
        self.time_embedding = TimeEmbedding(time_emb_dim)
        self.flow_matcher = flow_matcher or ConditionalFlowMatcher(0.0)
        self.solver, self.optimizer, self.scheduler = solver, optimizer, scheduler
        self.seg_loss_weight, self.dice_weight = seg_loss_weight, dice_weight
        self.dice_smooth = 1.0

    def forward_flow(self, t: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        bottleneck, skips = self.encoder(x)
        return self.flow_decoder(bottleneck, skips, self.time_embedding(t))

    def forward_segmentation(self, x: torch.Tensor) -> torch.Tensor:
        bottleneck, skips = self.encoder(x)
        return self.seg_decoder(bottleneck, skips)

    def compute_segmentation_loss(self, pred_mask: torch.Tensor, target_mask: torch.Tensor):
        if self.num_classes is not None:
            if target_mask.dim() == 4 and target_mask.shape[1] == 1:
                target_mask = target_mask.squeeze(1)
            seg, dice, ce = _SegLossMulticlass.apply(pred_mask, target_mask.long(), self.ignore_index,
                                                     self.dice_smooth, self.dice_weight)
            return seg, {"dice": dice, "ce": ce, "seg_total": seg}
        seg, dice, bce = _SegLoss.apply(pred_mask, target_mask.float(), self.dice_smooth, self.dice_weight)
        return seg, {"dice": dice, "bce": bce, "seg_total": seg}

    def model_step(self, batch):
        source_img, target_img, gt_mask = batch
        t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(source_img, target_img)
        flow_loss = _MSE.apply(self.forward_flow(t, xt), ut)
        seg_loss, d = self.compute_segmentation_loss(self.forward_segmentation(source_img), gt_mask)
        total = flow_loss + self.seg_loss_weight * seg_loss
        second = "ce" if self.num_classes is not None else "bce"
        return total, {"total": total, "flow": flow_loss, "seg": seg_loss, "seg_dice": d["dice"],
                       "seg_" + second: d[second]}

    def training_step(self, batch, batch_idx: int) -> torch.Tensor:
        loss, d = self.model_step(batch)
        for k, v in d.items():
            self.log(f"train/{k}_loss", v, on_step=True, on_epoch=True, prog_bar=(k == "total"), sync_dist=True)
        return loss

    # the reference's validation / test logging: (key suffix, value key, prog_bar); every call is on_step=False,
    # on_epoch=True, sync_dist=True (conditional_flow_matching_multitask.py:306-343, 359-381,
    # conditional_flow_matching_multitask_multiclassloss.py:348-371, 424-476)
    _LOSS_KEYS = (("loss", "total", True), ("flow_loss", "flow", False), ("seg_loss", "seg", True))
    _METRIC_KEYS = (("dice_coef", "dice_coef", True), ("iou", "iou", True))

    def _log_keys(self, stage: str):
        keys = list(self._LOSS_KEYS)
        if stage == "val":
            second = "seg_ce" if self.num_classes is not None else "seg_bce"
            keys += [("seg_dice", "seg_dice", False), (second, second, False)]
            if self.num_classes is None:         # the multiclass reference has its validation metrics commented out
                keys += list(self._METRIC_KEYS)
        else:
            keys += list(self._METRIC_KEYS)
        return keys

    def evaluation_values(self, batch) -> Dict[str, torch.Tensor]:
        """Every value of the validation / test steps for one batch as device scalars: {"total", "flow", "seg",
        "seg_dice", "seg_bce" | "seg_ce", "dice_coef", "iou"}.  The networks run in the mode they are in (Lightning sets
        eval mode: BatchNorm from the running statistics), through the forward-only head + MSE and segmentation
        metric kernels; the mask head runs once (the reference's second forward_segmentation is the same in eval mode)."""
        source_img, target_img, gt_mask = batch
        with evaluation.eval_grad_mode():
            t, xt, ut = self.flow_matcher.sample_location_and_conditional_flow(source_img, target_img)
            return evaluation.multitask_values(
                self.encoder, self.flow_decoder, self.seg_decoder, self.time_embedding.dim, source_img, xt, t, ut,
                gt_mask, self.num_classes, self.ignore_index, self.dice_smooth, self.dice_weight, self.seg_loss_weight)

    def _eval_step(self, batch, stage: str) -> None:
        d = self.evaluation_values(batch)
        for suffix, key, bar in self._log_keys(stage):
            self.log(f"{stage}/{suffix}", d[key], on_step=False, on_epoch=True, prog_bar=bar, sync_dist=True)

    def validation_step(self, batch, batch_idx: int) -> None:
        self._eval_step(batch, "val")

    def test_step(self, batch, batch_idx: int) -> None:
        self._eval_step(batch, "test")

    def configure_optimizers(self) -> Dict[str, Any]:
        params = (list(self.encoder.parameters()) + list(self.flow_decoder.parameters())
                  + list(self.seg_decoder.parameters()))
        optimizer = self.optimizer(params=params)
        if self.scheduler is not None:
            return {"optimizer": optimizer,
                    "lr_scheduler": {"scheduler": self.scheduler(optimizer=optimizer), "monitor": "val/loss",
                                     "interval": "epoch", "frequency": 1}}
        return {"optimizer": optimizer}

    @torch.no_grad()
    def generate(self, source_img: torch.Tensor, num_steps: int = 100, method: Optional[str] = None,
                 atol: Optional[float] = None, rtol: Optional[float] = None, per_sample: bool = False):
        """(generated image, mask probabilities / class map) like the reference's generate (:419-484): the module goes
        to eval mode and stays there, the mask head runs once on the source, the flow is integrated with the solver's
        method (dopri5 at 1e-4 by default; ``method="euler"`` = ``num_steps`` fixed steps)."""
        if self.solver is None:
            raise ValueError("Solver is not initialized. Cannot perform inference.")
        self.eval()
        if source_img.dim() == 3:
            source_img = source_img.unsqueeze(0)
        logits = self.forward_segmentation(source_img)
        if self.num_classes is not None:       # class map, as the multiclass reference returns (:536-537)
            pred_mask = torch.argmax(torch.softmax(logits, dim=1), dim=1, keepdim=True)
        else:
            pred_mask = torch.sigmoid(logits)
        return (_solve(self, self.forward_flow, source_img, num_steps, method, atol, rtol, per_sample=per_sample),
                pred_mask)
