"""What a fixed-step sampler costs and how far its end point is from a tight solution.

Default mode: for a network (random weights, or ``--ckpt PATH``), one batch of tiles and a list of ``method:num_steps``
pairs, one JSON line per pair with the number of network evaluations, the median time per solve
(``fixed_step_generate(..., graph=True)``; device events around solves that end in a synchronise; the pairs take turns
within one run), the RMS and maximum deviation of x(1) from ``dopri5_generate(per_sample=True, atol=rtol=1e-6)`` and the
same deviation after the save conversion to uint8, in grey levels.  With random weights the table shows the cost per
evaluation and the mechanics; which step count a TRAINED model needs is a property of that model (``--ckpt``).

``--kernels``: the fused stage + combine launches of one step against the ``clone`` + ``ops.axpy_`` chain for the same
tableau, on fixed k tensors without a network, taking turns; every variant is timed ``--reps`` times, identical runs,
and the line carries median, minimum and maximum, so the spread of repeated runs is in the same output.  Eager launches
at batch 1 are bound by the host; ``--graph`` times hipGraph replays of the same launches, as ``graph=True`` issues them.

``--trace``: one eager solve per method and one step of the chain per method, for a separate
``rocprofv3 --kernel-trace --stats -- python scripts/sampler_tradeoff.py --trace`` run that times rk_stage_kernel /
rk_combine_kernel against axpy_kernel and the copy kernel.

Every mode first prints the algorithmic bytes per step of each tableau (T = B * 3 * H * W * 4 bytes)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

DEFAULT_PAIRS = "euler:50,euler:25,midpoint:25,midpoint:12,heun:25,rk4:12,rk4:6,rk4_38:12"


def step_bytes_in_T(method):
    """(fused, chain) bytes per step in units of T, from the tableau: a fused stage with m non-zero coefficients reads x
    and m k's and writes out (2 + m; a row of zeros launches nothing that scales with T), the fused combine reads and
    writes x and reads its m k's (2 + m); the chain clones x (2) and runs one axpy (3) per non-zero coefficient."""
    from stain2stain_amd.samplers import fixed_step_coefficients
    rows, weights = fixed_step_coefficients(method, 1)
    fused = sum(2 + len(r) for r in rows if r) + 2 + len(weights)
    chain = sum(2 + 3 * len(r) for r in rows if r) + 3 * len(weights)
    return fused, chain


def to_u8(x):
    """The reference's save conversion: trunc(clamp((x * 0.5 + 0.5) * 255, 0, 255))."""
    return torch.clamp((x * 0.5 + 0.5) * 255.0, 0, 255).to(torch.uint8)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def chain_step(x, ks, rows, weights, xs):
    """One step's stage inputs and update by clone + axpy_ (kernels that predate the fused ones); k's held fixed."""
    from stain2stain_amd import ops
    for r in rows:
        if r:
            xi = x.clone()
            for j, c in r:
                ops.axpy_(xi, ks[j], c)
    for j, c in weights:
        ops.axpy_(x, ks[j], c)


def fused_step(x, ks, rows, weights, xs, t, table, counter):
    from stain2stain_amd import ops
    s = len(rows)
    for i, r in enumerate(rows):
        terms = [(c, ks[j]) for j, c in r]
        ops.rk_stage_(x, terms, xs if terms else None, t, table, counter, s, i)
    ops.rk_combine_(x, [(c, ks[j]) for j, c in weights], counter)


def kernels_mode(a, methods):
    from stain2stain_amd.samplers import fixed_step_coefficients, fixed_step_node_times
    inner = a.inner
    for B in [int(v) for v in a.batches.split(",")]:
        g = torch.Generator().manual_seed(a.seed + B)
        mk = lambda: (torch.rand(B, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
        x0, ks, xs = mk(), [mk() * 1e-3 for _ in range(4)], mk()
        T = x0.numel() * 4
        t = torch.zeros(B, device="cuda")
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        runs = {}
        for m in methods:
            rows, weights = fixed_step_coefficients(m, inner)
            table = fixed_step_node_times(m, inner).cuda()

            def fused(rows=rows, weights=weights, table=table):
                counter.zero_()
                for _ in range(inner):
                    fused_step(x0, ks, rows, weights, xs, t, table, counter)

            def chain(rows=rows, weights=weights):
                for _ in range(inner):
                    chain_step(x0, ks, rows, weights, xs)
            runs[(m, "fused")], runs[(m, "chain")] = fused, chain
        for fn in runs.values():
            fn()
        if a.graph:                                           # the launches as graph=True replays them: no host time
            from stain2stain_amd import ops
            graphs = {}
            for k, fn in runs.items():
                graphs[k] = torch.cuda.CUDAGraph()
                with ops.capture_graph(graphs[k]):
                    fn()
            runs = {k: g.replay for k, g in graphs.items()}
            for fn in runs.values():
                fn()
        times = {k: [] for k in runs}
        for _ in range(a.reps):                               # the variants take turns within one run
            for k, fn in runs.items():
                times[k].append(timed(fn)[0] * 1e3 / inner)    # us per step
        for m in methods:
            fb, cb = step_bytes_in_T(m)
            row = {"mode": "kernels", "launch": "graph" if a.graph else "eager", "batch": B, "size": a.size, "method": m, "reps": a.reps, "steps_per_rep": inner}
            for kind, nb in (("fused", fb), ("chain", cb)):
                v = times[(m, kind)]
                med = statistics.median(v)
                row[kind] = {"us_per_step_median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2),
                             "bytes_T": nb, "TB_per_s": round(nb * T / med / 1e6, 3)}
            row["chain_over_fused"] = round(row["chain"]["us_per_step_median"] / row["fused"]["us_per_step_median"], 3)
            print(json.dumps(row), flush=True)


def trace_mode(a, net, methods):
    from stain2stain_amd import fixed_step_generate
    from stain2stain_amd.samplers import fixed_step_coefficients
    B = int(a.batches.split(",")[-1])
    g = torch.Generator().manual_seed(a.seed)
    x = (torch.rand(B, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
    ks = [torch.rand_like(x) * 1e-3 for _ in range(4)]
    for m in methods:
        ms, _ = timed(lambda: fixed_step_generate(net, x, a.trace_steps, m))
        rows, weights = fixed_step_coefficients(m, a.trace_steps)
        for _ in range(a.trace_steps):
            chain_step(x.clone(), ks, rows, weights, None)
        torch.cuda.synchronize()
        print(json.dumps({"mode": "trace", "batch": B, "method": m, "num_steps": a.trace_steps,
                          "eager_solve_ms": round(ms, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default=DEFAULT_PAIRS, help="comma-separated method:num_steps")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batches", default="1,32", help="--kernels / --trace: batch sizes (trace uses the last)")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="--kernels: steps between two events")
    ap.add_argument("--seed", type=int, default=1984)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--ckpt", default=None, help="a checkpoint of the default FlowUNet (stain2stain_amd.checkpoint)")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--graph", action="store_true", help="--kernels: time hipGraph replays of the same launches")
    ap.add_argument("--trace-steps", type=int, default=2)
    a = ap.parse_args()
    from stain2stain_amd import FIXED_STEP_METHODS, FlowUNet, checkpoint, dopri5_generate, fixed_step_generate
    from stain2stain_amd.samplers import fixed_step_evaluations
    rk = [m for m in FIXED_STEP_METHODS if m != "euler"]
    for m in FIXED_STEP_METHODS:
        fb, cb = step_bytes_in_T(m)
        print(json.dumps({"mode": "bytes", "method": m, "fused_bytes_per_step_T": fb, "chain_bytes_per_step_T": cb}))
    if a.kernels:
        return kernels_mode(a, rk)
    torch.manual_seed(a.seed)
    net = FlowUNet(precision=a.precision)
    if a.ckpt:
        ckpt = checkpoint.read_checkpoint(a.ckpt)         # a Lightning checkpoint keeps the network under "net."
        keys = checkpoint.extract_state_dict(ckpt)
        checkpoint.load_weights(net, ckpt, strip_prefix="net." if any(k.startswith("net.") for k in keys) else None)
    net = net.cuda().eval()
    if a.trace:
        return trace_mode(a, net, rk)
    pairs = [(p.split(":")[0], int(p.split(":")[1])) for p in a.pairs.split(",")]
    g = torch.Generator().manual_seed(a.seed + a.batch)
    x = (torch.rand(a.batch, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
    tight, st = dopri5_generate(net, x, atol=1e-6, rtol=1e-6, per_sample=True, graph=True, return_stats=True)
    net._s2s_dopri5_graph.close()
    tight_u8 = to_u8(tight).float()
    print(json.dumps({"mode": "tight", "weights": a.ckpt or "random", "batch": a.batch, "evaluations": st["evaluations"],
                      "attempted": st["attempted"]}), flush=True)
    times = {p: [] for p in pairs}
    outs = {}
    for p in pairs:                                           # warm-up: one capture per pair, not timed
        outs[p] = fixed_step_generate(net, x, p[1], p[0], graph=True)
    for _ in range(a.reps):                                   # the pairs take turns; each turn re-captures (the cache
        for p in pairs:                                       # holds one graph), so time the replays of a second solve
            fixed_step_generate(net, x, p[1], p[0], graph=True)
            times[p].append(timed(lambda: fixed_step_generate(net, x, p[1], p[0], graph=True))[0])
    for p in pairs:
        d = (outs[p] - tight).double()
        du = (to_u8(outs[p]).float() - tight_u8).double()
        ms = statistics.median(times[p])
        ev = fixed_step_evaluations(p[0], p[1])
        print(json.dumps({"mode": "tradeoff", "weights": a.ckpt or "random", "precision": a.precision, "batch": a.batch,
                          "method": p[0], "num_steps": p[1], "evaluations": ev, "ms_per_solve": round(ms, 3),
                          "ms_min": round(min(times[p]), 3), "ms_max": round(max(times[p]), 3),
                          "ms_per_evaluation": round(ms / ev, 4), "rms_dev": float(d.pow(2).mean().sqrt()),
                          "max_dev": float(d.abs().max()), "u8_rms_dev": round(float(du.pow(2).mean().sqrt()), 4),
                          "u8_max_dev": int(du.abs().max())}), flush=True)
    for name in ("_s2s_rk_graph", "_s2s_euler_graph"):
        g = getattr(net, name, None)
        if g is not None:
            g.close()


if __name__ == "__main__":
    main()
