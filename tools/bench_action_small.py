"""
bench_action_small.py - GPU-BOX TOOLING: the matrix-free route at n <= 16 (knob "action_small" = 1,
qoc_amd/csrc/qocx_action16.hip) against the Pade route of the same build (knob 0, which launches what it
always launched), in turns in ONE process.

    python tools/bench_action_small.py [--sizes 4 8 16] [--controls 2 4] [--out profiles/action_small.jsonl]

Problem: bench.py's GUE operators (unit spectral norm) at n = 4, 8, 16 with two and four real controls of
amplitude 0.1, one state (psi0 = e_0, target e_1), one coherent final TargetStateInfidelity, 256 seeds x
1000 steps, forward + gradient, controls resident. Per (n, K) three runs; a run times 20 evaluations of
each knob value (host clock around eval_resident + the download of costs and gradients, which ends in a
synchronise), the two taking turns evaluation by evaluation. One JSON line per (n, K, run, route): median /
min / max ms per evaluation, the Taylor degrees executed, and the sums that show both routes computed the
same thing. One further shape: 2048 seeds at n = 16, two controls - the regime in which four seeds to a
wave might be the better kernel (not built).

That the change leaves everything else alone:
    python tools/bench_action_small.py --gate --parent-library PATH [--out profiles/action_small_gate.jsonl]
runs this build and the parent commit's library in fresh processes, alternating, two visits each with the
order swapped (parent, this; this, parent). A process times bench.py's headline shape (n = 32, one state,
two controls) and the 256-seed n = 8 evaluation above with every knob at its default, three runs of 20
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

SEEDS, MANY_SEEDS, N_EVAL, AMPLITUDE = 256, 2048, 1001, 0.1


def make_problem(n, k, seeds):
    rng = np.random.default_rng(2003 + n)
    h0 = bench.gue(rng, n)
    g = [bench.gue(rng, n) for _ in range(k)]
    psi0 = np.eye(n, dtype=np.complex128)[:1]
    target = np.eye(n, dtype=np.complex128)[1:2]
    controls = np.empty((seeds, N_EVAL, k))
    for b in range(seeds):
        controls[b] = AMPLITUDE * np.random.default_rng(1000 + b).standard_normal((N_EVAL, k))
    return h0, g, psi0, target, controls


def setup(engine, n, k, seeds=SEEDS):
    from qoc_amd.engine import COST_TARGET_COHERENT
    h0, g, psi0, target, controls = make_problem(n, k, seeds)
    engine.set_schroedinger_problem(
        n, 1, k, N_EVAL, N_EVAL, bench.DT * (N_EVAL - 1), h0[None], np.stack(g)[None], psi0,
        costs=[dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=target)])
    engine.upload_controls(controls)


def evaluate(engine):
    engine.eval_resident(True)
    return engine.download_results(want_grad=True, want_final=False)


def executed(engine):
    return {int(m): int(c) for m, c in engine.action_degrees().items() if c}


def gate_child(library):
    """The two shapes on the library at `library`, no knob touched: three runs of 20 evaluations each."""
    from qoc_amd import engine as engine_mod
    from qoc_amd.engine import COST_TARGET_COHERENT
    engine_mod.load_library(library)
    engine = engine_mod.Engine(0)
    out = dict(library=library)
    for what in ("headline", "n8"):
        if what == "headline":
            h0, g, psi0, target = bench.make_problem()
            engine.set_schroedinger_problem(
                bench.DIM, 1, bench.K_CTRL, bench.N_EVAL, bench.N_EVAL, bench.DT * (bench.N_EVAL - 1), h0[None],
                np.stack(g)[None], psi0, costs=[dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=target)])
            engine.upload_controls(bench.make_controls(0, bench.SEEDS_PER_GPU))
        else:
            setup(engine, 8, 2)
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
            for what in ("headline", "n8"):
                lines.append(dict(what=what, build=label, visit=["parent first", "this build first"][visit],
                                  **got[what]))
                print(json.dumps(lines[-1]), flush=True)
                pooled.setdefault((what, label), []).extend(got[what]["runs_ms"])
    for what in ("headline", "n8"):
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--controls", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-many-seeds", action="store_true", help="skip the 2048-seed shape")
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
        return gate(args.parent_library, args.out or os.path.join(ROOT, "profiles", "action_small_gate.jsonl"))
    args.out = args.out or os.path.join(ROOT, "profiles", "action_small.jsonl")
    from qoc_amd.engine import Engine
    engine = Engine(0)
    routes = (("matrix_free", 1), ("pade", 0))
    shapes = [(n, k, SEEDS) for n in args.sizes for k in args.controls]
    if not args.no_many_seeds:
        shapes.append((16, 2, MANY_SEEDS))
    lines = []
    for n, k, seeds in shapes:
        setup(engine, n, k, seeds)
        for _, knob in routes:  # warm both routes: code objects, buffers
            engine.set_knob("action_small", knob)
            for _ in range(3):
                evaluate(engine)
        for run in range(args.runs):
            ms = {name: [] for name, _ in routes}
            check, degrees = {}, {}
            for rep in range(args.reps):
                for name, knob in (routes if rep % 2 == 0 else routes[::-1]):
                    engine.set_knob("action_small", knob)
                    engine.synchronize()
                    t0 = time.perf_counter()
                    cost, grads, _ = evaluate(engine)
                    ms[name].append((time.perf_counter() - t0) * 1e3)
                    check[name] = dict(sum_cost=float(np.sum(cost)), grad_l2=float(np.linalg.norm(grads)))
                    degrees[name] = executed(engine)
            for name, _ in routes:
                med = float(np.median(ms[name]))
                lines.append(dict(
                    n=n, controls=k, run=run, route=name, seeds=seeds, steps=N_EVAL - 1, reps=args.reps,
                    ms_median=round(med, 4), ms_min=round(min(ms[name]), 4), ms_max=round(max(ms[name]), 4),
                    msteps_per_s=round(seeds * (N_EVAL - 1) / med / 1e3, 2), degrees=degrees[name],
                    reruns=int(engine.action_reruns()), check=check[name]))
                print(json.dumps(lines[-1]), flush=True)
    engine.set_knob("action_small", 0)
    engine.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
