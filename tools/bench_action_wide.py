"""
bench_action_wide.py - GPU-BOX TOOLING: the wide matrix-free route (knob "action" = 2,
qoc_amd/csrc/qocx_action4.hip) against the Pade route of the same build (knob "action" = 1, which above
n = 32 launches what it always launched), in turns in ONE process.

    python tools/bench_action_wide.py [--dims 40 48 64] [--out profiles/action_wide.jsonl]

Problem per size: bench.py's GUE operators (unit spectral norm) with FOUR real controls of amplitude
0.1, one state, one final TargetStateInfidelity, 256 seeds x 1000 steps, forward + gradient, controls
resident. Per size three runs; a run times 20 evaluations of each route (host clock around
eval_resident + the download of costs and gradients, which ends in a synchronise), the routes taking
turns evaluation by evaluation. One JSON line per (size, run, route): median / min / max ms per
evaluation, propagator-steps per second, the Taylor degrees the wide route executed, and the sums
that show both routes computed the same thing.

Per-kernel times come from a run of its own, profiler off everywhere else:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python tools/bench_action_wide.py --trace-child --dims 64
which evaluates with "action" = 2 only: no Pade, LU or K3 kernel may appear in its trace.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

K_CTRL, SEEDS, N_EVAL, AMPLITUDE = 4, 256, 1001, 0.1


def make_problem(n):
    rng = np.random.default_rng(2003 + n)
    h0 = bench.gue(rng, n)
    g = [bench.gue(rng, n) for _ in range(K_CTRL)]
    psi0 = np.eye(n, dtype=np.complex128)[:1]
    target = np.eye(n, dtype=np.complex128)[1:2]
    controls = np.empty((SEEDS, N_EVAL, K_CTRL))
    for b in range(SEEDS):
        controls[b] = AMPLITUDE * np.random.default_rng(1000 + b).standard_normal((N_EVAL, K_CTRL))
    return h0, g, psi0, target, controls


def setup(engine, n):
    from qoc_amd.engine import COST_TARGET_COHERENT
    h0, g, psi0, target, controls = make_problem(n)
    engine.set_schroedinger_problem(
        n, 1, K_CTRL, N_EVAL, N_EVAL, bench.DT * (N_EVAL - 1), h0[None], np.stack(g)[None], psi0,
        costs=[dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=target)])
    engine.upload_controls(controls)


def evaluate(engine):
    engine.eval_resident(True)
    return engine.download_results(want_grad=True, want_final=False)


def trace_child(dims):
    from qoc_amd.engine import Engine
    engine = Engine(0)
    engine.set_knob("action", 2)
    for n in dims:
        setup(engine, n)
        for _ in range(5):
            evaluate(engine)
        degrees = {m: c for m, c in engine.action_degrees().items() if c}
        assert degrees and engine.action_reruns() == 0, (n, degrees)
    engine.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[40, 48, 64])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "action_wide.jsonl"))
    ap.add_argument("--trace-child", action="store_true")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child(args.dims)
    from qoc_amd.engine import Engine
    engine = Engine(0)
    routes = (("wide", 2), ("pade", 1))
    lines = []
    for n in args.dims:
        setup(engine, n)
        for _, knob in routes:  # warm both routes: code objects, buffers
            engine.set_knob("action", knob)
            for _ in range(3):
                evaluate(engine)
        for run in range(args.runs):
            ms = {name: [] for name, _ in routes}
            check, degrees = {}, {}
            for rep in range(args.reps):
                for name, knob in (routes if rep % 2 == 0 else routes[::-1]):
                    engine.set_knob("action", knob)
                    engine.synchronize()
                    t0 = time.perf_counter()
                    cost, grads, _ = evaluate(engine)
                    ms[name].append((time.perf_counter() - t0) * 1e3)
                    check[name] = dict(sum_cost=float(np.sum(cost)), grad_l2=float(np.linalg.norm(grads)))
                    degrees[name] = {int(m): int(c) for m, c in engine.action_degrees().items() if c}
            for name, _ in routes:
                med = float(np.median(ms[name]))
                lines.append(dict(
                    n=n, run=run, route=name, seeds=SEEDS, steps=N_EVAL - 1, controls=K_CTRL, reps=args.reps,
                    ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                    propagator_steps_per_s=round(SEEDS * (N_EVAL - 1) / (med * 1e-3)),
                    degrees=degrees[name], reruns=int(engine.action_reruns()), check=check[name]))
                print(json.dumps(lines[-1]), flush=True)
    engine.set_knob("action", 1)
    engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
