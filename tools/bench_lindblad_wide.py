"""
bench_lindblad_wide.py - secondary measurement: the Lindblad engine at 33 <= n <= 64 (knob
lindblad_wide, qoc_amd/csrc/qocx_lindblad16t.hip). For n = 40, 48, 64 at 64 seeds x 200 steps, two
operators (a, a^H a), two controls, one final target cost, forward + gradient, three runs each: ms per
evaluation, the sub-interval count, the CUs in use (one workgroup per seed) and the fraction of the FP64
matrix peak under the complex operation count of bench.py's `secondary` for configs[3]
(12 x ((2 + 2 L) x 2 + 2) n^3 complex multiply-adds of 8 flops per sub-interval).

    python tools/bench_lindblad_wide.py             # -> profiles/lindblad_wide.jsonl
    python tools/bench_lindblad_wide.py --cpu --out profiles/lindblad_wide_cpu.jsonl
        no GPU: the NumPy model of the same scheme on this host's CPU, one seed, 10 steps, forward +
        gradient, scaled to the problem on 16 processes
    python tools/bench_lindblad_wide.py --gate --parent-library PATH
        "changes nothing at n <= 32": the plain 64-seed configs[3] evaluation and an n = 24 evaluation
        (64 seeds x 200 steps) in fresh processes alternating between the parent commit's library and
        this build's, the order swapped between the two visits; this build's median run against the
        parent's slowest run -> profiles/lindblad_wide_gate.jsonl
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

SEEDS, STEPS, OPS, K = 64, 200, 2, 2


def system(n):
    rng = np.random.default_rng(7)
    h0 = bench.gue(rng, n)
    g = [bench.gue(rng, n) for _ in range(K)]
    a = np.diag(np.sqrt(np.arange(1, n)), 1).astype(np.complex128)
    ops = np.stack([a, a.conj().T @ a])
    gam = np.array([0.05, 0.02])
    rho0 = np.zeros((1, n, n), complex)
    rho0[0, 0, 0] = 1
    tgt = np.zeros((1, n, n), complex)
    tgt[0, 1, 1] = 1
    return h0, g, gam, ops, rho0, tgt


def controls(steps, seeds):
    return np.stack([0.1 * np.random.default_rng(1000 + b).standard_normal((steps + 1, K))
                     for b in range(seeds)])


def device(n, runs):
    from qoc_amd.engine import COST_TARGET_DENSITY, Engine
    engine = Engine(0)
    engine.set_knob("lindblad_wide", 1)
    h0, g, gam, ops, rho0, tgt = system(n)
    N = STEPS + 1
    engine.set_lindblad_problem(n, 1, K, N, N, bench.DT * STEPS, h0, g, gam, ops, rho0,
                                costs=[dict(kind=COST_TARGET_DENSITY, step_cost=0, scale=1.0, vectors=tgt)])
    u = controls(STEPS, SEEDS)
    engine.evaluate_lindblad(u)
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        cost, grads, final = engine.evaluate_lindblad(u)
        ms.append((time.perf_counter() - t0) * 1e3)
    subs = engine.lindblad_last_subintervals()
    cus = SEEDS  # one workgroup of sixteen waves per seed, one per CU (its LDS leaves no room for a second)
    engine.close()
    flops = 8.0 * 12 * ((2 + 2 * OPS) * 2 + 2) * n ** 3 * subs
    med = float(np.median(ms))
    return dict(n=n, seeds=SEEDS, steps=STEPS, operators=OPS, controls=K, ms=[round(x, 2) for x in ms],
                ms_median=round(med, 2), subintervals=int(subs),
                subintervals_per_step=subs / SEEDS / STEPS, cus_in_use=int(cus),
                ms_per_subinterval_of_a_seed=round(med / (subs / SEEDS), 4),
                check=dict(sum_cost=float(np.sum(cost)), grad_l2=float(np.linalg.norm(grads)),
                           trace=float(np.trace(final[0, 0]).real)),
                tflops=round(flops / (med * 1e-3) / 1e12, 3),
                fraction_of_fp64_matrix_peak=round(flops / (med * 1e-3) / 1e12 / bench.FP64_MFMA_PEAK_TFLOPS, 4))


def cpu(n, steps=10, cpus=16):
    """The NumPy model of the same scheme (tests/lindblad_model.py), one seed, `steps` steps, forward +
    gradient, scaled to 64 seeds x 200 steps spread over `cpus` processes."""
    from oracle import qoc_lindblad_numpy as ol
    from tests import lindblad_wide_cases as wc
    h0, g, gam, ops, rho0, tgt = system(n)
    u = controls(steps, 1)[0]
    t0 = time.perf_counter()
    wc.lm.evaluate_with_grad(wc.WideLindblad(h0, g, gam, ops), u, rho0, bench.DT * steps, steps + 1,
                             [ol.TargetDensityInfidelity(tgt)])
    one = time.perf_counter() - t0
    return dict(n=n, cpu_model_seconds_one_seed=round(one, 2), cpu_model_steps=steps,
                cpu_seconds_scaled=round(one * STEPS / steps * SEEDS / cpus, 1), cpus=cpus)


GATE_CASES = ("configs[3]", "n24")


def gate_child(library):
    """One process on `library`: three runs of each gate case (10 evaluations a run), one JSON line."""
    from qoc_amd import engine as engine_mod
    from qoc_amd.engine import COST_TARGET_DENSITY
    engine_mod.load_library(library)
    engine = engine_mod.Engine(0)
    out = dict(library=library)
    for what in GATE_CASES:
        if what == "configs[3]":
            h0, g, gam, ops, rho0, tgt = bench.lindblad_problem()
            n, N, seeds = bench.LB_DIM, bench.LB_EVAL, bench.LB_SEEDS
        else:
            h0, g, gam, ops, rho0, tgt = system(24)
            n, N, seeds = 24, STEPS + 1, SEEDS
        engine.set_lindblad_problem(n, 1, K, N, N, bench.DT * (N - 1), h0, g, gam, ops, rho0,
                                    costs=[dict(kind=COST_TARGET_DENSITY, step_cost=0, scale=1.0, vectors=tgt)])
        u = controls(N - 1, seeds)
        for _ in range(3):
            cost, grads, _ = engine.evaluate_lindblad(u)
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(10):
                cost, grads, _ = engine.evaluate_lindblad(u)
            runs.append(round((time.perf_counter() - t0) / 10 * 1e3, 4))
        out[what] = dict(runs_ms=runs, check=dict(sum_cost=float(np.sum(cost)), grad_l2=float(np.linalg.norm(grads))))
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
            for what in GATE_CASES:
                lines.append(dict(what=what, build=label, visit=["parent first", "this build first"][visit],
                                  **got[what]))
                print(json.dumps(lines[-1]), flush=True)
                pooled.setdefault((what, label), []).extend(got[what]["runs_ms"])
    for what in GATE_CASES:
        parent, this = pooled[(what, "parent")], pooled[(what, "this build")]
        lines.append(dict(check="{}: this build's median run against the parent's slowest run".format(what),
                          this_median_ms=float(np.median(this)), parent_median_ms=float(np.median(parent)),
                          parent_max_ms=max(parent), passed=bool(np.median(this) <= max(parent))))
        print(json.dumps(lines[-1]), flush=True)
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "lindblad_wide.jsonl"))
    parser.add_argument("--runs", type=int, default=3)
    parser.add_argument("--sizes", type=int, nargs="*", default=[40, 48, 64])
    parser.add_argument("--cpu", action="store_true")
    parser.add_argument("--gate", action="store_true")
    parser.add_argument("--gate-child", default=None, metavar="LIBRARY")
    parser.add_argument("--parent-library", default=None)
    args = parser.parse_args()
    if args.gate_child:
        return gate_child(args.gate_child)
    if args.gate:
        if not args.parent_library:
            parser.error("--gate needs --parent-library")
        return gate(args.parent_library, os.path.join(ROOT, "profiles", "lindblad_wide_gate.jsonl"))
    lines = []
    for n in args.sizes:
        line = cpu(n) if args.cpu else device(n, args.runs)
        lines.append(line)
        print(json.dumps(line), flush=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
