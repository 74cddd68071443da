"""
bench_action_costs.py - GPU-BOX TOOLING: the matrix-free route under a step cost (knob "action_costs" = 1,
qoc_amd/csrc/qocx_action_costs.hip) against the Pade route of the same build (knob 0, which launches what
it always launched), in turns in ONE process.

    python tools/bench_action_costs.py [--cost-eval-steps 1 10] [--out profiles/action_costs.jsonl]

Problem: the headline shape with four controls - n = 32, bench.py's GUE operators (unit spectral norm),
FOUR real controls of amplitude 0.1, one state (psi0 = e_0), 256 seeds x 1000 steps, forward + gradient,
controls resident - under one final TargetStateInfidelity (target e_1) plus one ForbidStates with two
forbidden vectors (e_2, e_3; scale 1 / evaluations), at cost_eval_step 1 and 10. Per cost_eval_step three
runs; a run times 20 evaluations of each knob value (host clock around eval_resident + the download of
costs and gradients, which ends in a synchronise), the two taking turns evaluation by evaluation. One JSON
line per (cost_eval_step, run, route): median / min / max ms per evaluation, the Taylor degrees executed,
and the sums that show both routes computed the same thing.

Per-kernel times come from a run of its own, profiler off everywhere else:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python tools/bench_action_costs.py --trace-child --cost-eval-steps 1
which evaluates with the knob at 1 only: no Pade, LU or K3 kernel may appear in its trace.

That the change leaves everything else alone:
    python tools/bench_action_costs.py --gate --parent-library PATH [--out profiles/action_costs_gate.jsonl]
runs this build and the parent commit's library in fresh processes, alternating, two visits each with
the order swapped (parent, this; this, parent). A process times bench.py's headline shape and the step-cost
problem above (cost_eval_step 10) with every knob at its default - the Pade route -, three runs of 20
evaluations each. The check lines compare this build's median run against the parent's slowest run.
"""

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

DIM, K_CTRL, SEEDS, N_EVAL, AMPLITUDE = 32, 4, 256, 1001, 0.1


def make_problem():
    rng = np.random.default_rng(2003 + DIM)
    h0 = bench.gue(rng, DIM)
    g = [bench.gue(rng, DIM) for _ in range(K_CTRL)]
    eye = np.eye(DIM, dtype=np.complex128)
    controls = np.empty((SEEDS, N_EVAL, K_CTRL))
    for b in range(SEEDS):
        controls[b] = AMPLITUDE * np.random.default_rng(1000 + b).standard_normal((N_EVAL, K_CTRL))
    return h0, g, eye[:1], eye[1:2], eye[2:4], controls


def setup(engine, ces):
    from qoc_amd.engine import COST_FORBID, COST_TARGET_COHERENT
    h0, g, psi0, target, forbidden, controls = make_problem()
    count = (N_EVAL - 1) // ces
    engine.set_schroedinger_problem(
        DIM, 1, K_CTRL, N_EVAL, N_EVAL, bench.DT * (N_EVAL - 1), h0[None], np.stack(g)[None], psi0,
        costs=[dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=target),
               dict(kind=COST_FORBID, step_cost=1, scale=1.0 / count, vectors=forbidden, counts=[2])],
        cost_eval_step=ces)
    engine.upload_controls(controls)


def evaluate(engine):
    engine.eval_resident(True)
    return engine.download_results(want_grad=True, want_final=False)


def executed(engine):
    return {int(m): int(c) for m, c in engine.action_degrees().items() if c}


def trace_child(steps):
    from qoc_amd.engine import Engine
    engine = Engine(0)
    engine.set_knob("action_costs", 1)
    for ces in steps:
        setup(engine, ces)
        for _ in range(5):
            evaluate(engine)
        assert executed(engine) and engine.action_reruns() == 0, ces
    engine.close()


def gate_child(library):
    """The two shapes on the library at `library`, no knob touched: three runs of 20 evaluations each."""
    from qoc_amd import engine as engine_mod
    from qoc_amd.engine import COST_TARGET_COHERENT
    engine_mod.load_library(library)
    engine = engine_mod.Engine(0)
    out = dict(library=library)
    for what in ("headline", "step_cost"):
        if what == "headline":
            h0, g, psi0, target = bench.make_problem()
            engine.set_schroedinger_problem(
                bench.DIM, 1, bench.K_CTRL, bench.N_EVAL, bench.N_EVAL, bench.DT * (bench.N_EVAL - 1), h0[None],
                np.stack(g)[None], psi0, costs=[dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=target)])
            engine.upload_controls(bench.make_controls(0, bench.SEEDS_PER_GPU))
        else:
            setup(engine, 10)
        for _ in range(5):
            evaluate(engine)
        runs = []
        for _ in range(3):
            engine.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                cost, grads, _ = evaluate(engine)
            runs.append(round((time.perf_counter() - t0) / 20 * 1e3, 4))
        out[what] = dict(runs_ms=runs, degrees=executed(engine),
                         check=dict(sum_cost=float(np.sum(cost)), grad_l2=float(np.linalg.norm(grads))))
    engine.close()
    print(json.dumps(out), flush=True)


def gate(parent_library, out_path):
    from qoc_amd import engine as engine_mod
    libraries = [("parent", os.path.abspath(parent_library)), ("this build", engine_mod.LIBRARY_PATH)]
    lines, pooled = [], {}
    for visit in range(2):
        for label, path in (libraries if visit == 0 else libraries[::-1]):
            got = subprocess.run([sys.executable, os.path.abspath(__file__), "--gate-child", path],
                                 check=True, capture_output=True, text=True, timeout=300).stdout
            got = json.loads(got.strip().splitlines()[-1])
            for what in ("headline", "step_cost"):
                lines.append(dict(what=what, build=label, visit=["parent first", "this build first"][visit],
                                  **got[what]))
                print(json.dumps(lines[-1]), flush=True)
                pooled.setdefault((what, label), []).extend(got[what]["runs_ms"])
    for what in ("headline", "step_cost"):
        parent, this = pooled[(what, "parent")], pooled[(what, "this build")]
        lines.append(dict(check="{}: this build's median run against the parent's slowest run".format(what),
                          this_median_ms=float(np.median(this)), parent_median_ms=float(np.median(parent)),
                          parent_max_ms=max(parent), passed=bool(np.median(this) <= max(parent))))
        print(json.dumps(lines[-1]), flush=True)
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost-eval-steps", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--gate", action="store_true")
    ap.add_argument("--gate-child", default=None, metavar="LIBRARY")
    ap.add_argument("--parent-library", default=None)
    args = ap.parse_args()
    if args.gate_child:
        return gate_child(args.gate_child)
    if args.gate:
        if not args.parent_library:
            ap.error("--gate needs --parent-library")
        return gate(args.parent_library, args.out or os.path.join(ROOT, "profiles", "action_costs_gate.jsonl"))
    args.out = args.out or os.path.join(ROOT, "profiles", "action_costs.jsonl")
    if args.trace_child:
        return trace_child(args.cost_eval_steps)
    from qoc_amd.engine import Engine
    engine = Engine(0)
    routes = (("matrix_free", 1), ("knob_0", 0))
    lines = []
    for ces in args.cost_eval_steps:
        setup(engine, ces)
        for _, knob in routes:  # warm both routes: code objects, buffers
            engine.set_knob("action_costs", knob)
            for _ in range(3):
                evaluate(engine)
        for run in range(args.runs):
            ms = {name: [] for name, _ in routes}
            check, degrees = {}, {}
            for rep in range(args.reps):
                for name, knob in (routes if rep % 2 == 0 else routes[::-1]):
                    engine.set_knob("action_costs", knob)
                    engine.synchronize()
                    t0 = time.perf_counter()
                    cost, grads, _ = evaluate(engine)
                    ms[name].append((time.perf_counter() - t0) * 1e3)
                    check[name] = dict(sum_cost=float(np.sum(cost)), grad_l2=float(np.linalg.norm(grads)))
                    degrees[name] = executed(engine)
            for name, _ in routes:
                lines.append(dict(
                    n=DIM, cost_eval_step=ces, run=run, route=name, seeds=SEEDS, steps=N_EVAL - 1, controls=K_CTRL,
                    reps=args.reps, ms_median=round(float(np.median(ms[name])), 4), ms_min=round(min(ms[name]), 4),
                    ms_max=round(max(ms[name]), 4), degrees=degrees[name], reruns=int(engine.action_reruns()),
                    check=check[name]))
                print(json.dumps(lines[-1]), flush=True)
    engine.set_knob("action_costs", 0)
    engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
