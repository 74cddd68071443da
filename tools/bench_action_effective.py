"""
bench_action_effective.py - GPU-BOX TOOLING: the matrix-free route on effective controls (knob "action_eff" =
1, qoc_amd/csrc/qocx_action_eff.hip) against the Pade route of the same build (knob 0, which launches what it
always launched), in turns in ONE process.

    python tools/bench_action_effective.py [--out profiles/action_effective.jsonl]

Problems, forward + gradient, controls resident, one state and one coherent final TargetStateInfidelity:
  - MagnusPolicy M4 on bench.py's GUE operators (unit spectral norm), 256 seeds x 1000 steps, real controls of
    amplitude 0.1: n = 32 with two controls (Ke = 5: the register-resident sweep AND the streamed one, knob
    "action_eff_exact" 1 / 0) and with four (Ke = 14, streamed); the same two control counts at n = 8
    ("action_small" = 1) and at n = 48 ("action" = 2);
  - the Piccolo-shaped problem of tools/bench_quadratic.py (n = 24, six real controls, the AC-Stark term as
    two quadratic terms, M2), 64 seeds x 1000 steps as in profiles/quadratic_hamiltonian.jsonl mode b.
Per problem three runs; a run times 20 evaluations of each route (host clock around eval_resident + the
download of costs and gradients, which ends in a synchronise), the routes taking turns evaluation by
evaluation with the order reversed every other turn. One JSON line per (problem, run, route): median / min /
max ms per evaluation, the Taylor degrees executed, and the sums that show the routes computed the same
thing; then one summary line per problem: the median of the three run medians per route and the range of the
run medians.

That the change leaves everything else alone:
    python tools/bench_action_effective.py --gate --parent-library PATH [--out profiles/action_effective_gate.jsonl]
runs this build and the parent commit's library in fresh processes, alternating, two visits each with the
order swapped (parent, this; this, parent). A process times bench.py's headline evaluation (n = 32, one
state, two controls, 256 seeds x 1000 steps, M2: what `bench.py --gpus 1` measures per step) and the 256-seed
M4 evaluation at n = 32 above with every knob at its default - "action_eff" = 0, the Pade route -, three runs
of 20 evaluations after 3 warm-up evaluations. The check lines compare this build's median run against the
parent's slowest run.
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

SEEDS, N_EVAL, AMPLITUDE = 256, 1001, 0.1
PADE = dict(action_eff=0)
ROUTE = dict(action_eff=1, action_eff_exact=1)
STREAMED = dict(action_eff=1, action_eff_exact=0)


def setup_m4(engine, n, k, seeds=SEEDS):
    from qoc_amd.engine import COST_TARGET_COHERENT
    rng = np.random.default_rng(2003 + n)
    h0 = bench.gue(rng, n)
    g = [bench.gue(rng, n) for _ in range(k)]
    psi0 = np.eye(n, dtype=np.complex128)[:1]
    target = np.eye(n, dtype=np.complex128)[1:2]
    controls = np.empty((seeds, N_EVAL, k))
    for b in range(seeds):
        controls[b] = AMPLITUDE * np.random.default_rng(1000 + b).standard_normal((N_EVAL, k))
    engine.set_schroedinger_problem(
        n, 1, k, N_EVAL, N_EVAL, bench.DT * (N_EVAL - 1), h0[None], np.stack(g)[None], psi0,
        costs=[dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=target)], magnus_policy="M4")
    engine.upload_controls(controls)


def setup_piccolo(engine):
    """tools/bench_quadratic.py's problem through the evaluator, which sets the problem and its terms on
    `engine`; one evaluate_batch leaves the 64 seeds' controls resident."""
    from tools import bench_quadratic as bq
    from qoc_amd.core import device
    from qoc_amd.standard import QuadraticHamiltonian, TargetStateInfidelity
    linear, terms, psi0, target = bq.piccolo()
    N = bq.N_STEPS + 1
    ev = device.SchroedingerEvaluator(bq.T, QuadraticHamiltonian(linear, terms), psi0, N, control_count=3,
                                      control_eval_count=N, complex_controls=True,
                                      costs=[TargetStateInfidelity(target)], backend=engine)
    ev.evaluate_batch(bq.starts(bq.SEEDS, real=False))
    return ev


def evaluate(engine):
    engine.eval_resident(True)
    return engine.download_results(want_grad=True, want_final=False)


def executed(engine):
    return {int(m): int(c) for m, c in engine.action_degrees().items() if c}


def set_knobs(engine, knobs):
    for name, value in knobs.items():
        engine.set_knob(name, value)


def measure(engine, what, routes, runs, reps, lines):
    """`routes`: [(name, knobs)], taking turns evaluation by evaluation."""
    for _, knobs in routes:  # warm every route: code objects, buffers
        set_knobs(engine, knobs)
        for _ in range(3):
            evaluate(engine)
    medians = {name: [] for name, _ in routes}
    for run in range(runs):
        ms = {name: [] for name, _ in routes}
        check, degrees = {}, {}
        for rep in range(reps):
            for name, knobs in (routes if rep % 2 == 0 else routes[::-1]):
                set_knobs(engine, knobs)
                engine.synchronize()
                t0 = time.perf_counter()
                cost, grads, _ = evaluate(engine)
                ms[name].append((time.perf_counter() - t0) * 1e3)
                check[name] = dict(sum_cost=float(np.sum(cost)), grad_l2=float(np.linalg.norm(grads)))
                degrees[name] = executed(engine)
        for name, _ in routes:
            med = float(np.median(ms[name]))
            medians[name].append(med)
            lines.append(dict(what, run=run, route=name, reps=reps, ms_median=round(med, 4),
                              ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                              degrees=degrees[name], reruns=int(engine.action_reruns()), check=check[name]))
            print(json.dumps(lines[-1]), flush=True)
    lines.append(dict(what, summary={name: dict(ms_median=round(float(np.median(m)), 4),
                                                runs_min=round(min(m), 4), runs_max=round(max(m), 4))
                                     for name, m in medians.items()}))
    print(json.dumps(lines[-1]), flush=True)
    set_knobs(engine, PADE)


def gate_child(library):
    """The two evaluations on the library at `library`, no knob touched."""
    from qoc_amd import engine as engine_mod
    from qoc_amd.engine import COST_TARGET_COHERENT
    engine_mod.load_library(library)
    engine = engine_mod.Engine(0)
    out = dict(library=library)
    for what in ("headline", "m4_n32"):
        if what == "headline":
            h0, g, psi0, target = bench.make_problem()
            engine.set_schroedinger_problem(
                bench.DIM, 1, bench.K_CTRL, bench.N_EVAL, bench.N_EVAL, bench.DT * (bench.N_EVAL - 1), h0[None],
                np.stack(g)[None], psi0, costs=[dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=target)])
            engine.upload_controls(bench.make_controls(0, bench.SEEDS_PER_GPU))
        else:
            setup_m4(engine, 32, 2)
        for _ in range(3):
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
            for what in ("headline", "m4_n32"):
                lines.append(dict(what=what, build=label, visit=["parent first", "this build first"][visit],
                                  **got[what]))
                print(json.dumps(lines[-1]), flush=True)
                pooled.setdefault((what, label), []).extend(got[what]["runs_ms"])
    for what in ("headline", "m4_n32"):
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
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gate", action="store_true")
    ap.add_argument("--gate-child", default=None, metavar="LIBRARY")
    ap.add_argument("--parent-library", default=None)
    args = ap.parse_args()
    if args.gate_child:
        return gate_child(args.gate_child)
    if args.gate:
        if not args.parent_library:
            ap.error("--gate needs --parent-library")
        return gate(args.parent_library, args.out or os.path.join(ROOT, "profiles", "action_effective_gate.jsonl"))
    args.out = args.out or os.path.join(ROOT, "profiles", "action_effective.jsonl")
    from qoc_amd.engine import Engine
    engine = Engine(0)
    lines = []
    for n, size_knobs in ((32, {}), (8, dict(action_small=1)), (48, dict(action=2))):
        set_knobs(engine, size_knobs)
        for k in (2, 4):
            setup_m4(engine, n, k)
            routes = [("matrix_free", ROUTE), ("pade", PADE)]
            if n == 32 and k == 2:
                routes.insert(1, ("matrix_free_streamed", STREAMED))
            what = dict(problem="M4", n=n, controls=k, Ke=2 * k + k * (k - 1) // 2, seeds=SEEDS, steps=N_EVAL - 1)
            measure(engine, what, routes, args.runs, args.reps, lines)
        set_knobs(engine, dict(action_small=0, action=1))
    setup_piccolo(engine)
    measure(engine, dict(problem="Piccolo-shaped quadratic, M2", n=24, controls=6, Ke=8, seeds=64, steps=1000),
            [("matrix_free", ROUTE), ("pade", PADE)], args.runs, args.reps, lines)
    engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
