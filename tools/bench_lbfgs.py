"""
bench_lbfgs.py - GPU-BOX TOOLING: what LBFGS costs and buys in grape_schroedinger_discrete_batch at
the headline shape (bench.py's problem - dim 32, 1000 propagator steps, 256 seeds - with four real
controls, P = 4004 parameters per seed), on one MI355X:

  - wall time per iteration of the device-resident LBFGS (qocx_lbfgs.hip), of LBFGS on the host loop
    (a subclass counts as "another plugin": one state machine per seed in NumPy) and of the
    device-resident Adam: the difference of the first and the last is what the L-BFGS step kernel
    and its B finished flags add to an iteration;
  - the evaluations LBFGS and Adam need to bring the MEDIAN seed's best error below each of a few
    stated errors (one evaluation per iteration for both), from the same starts.

    python tools/bench_lbfgs.py [--out profiles/lbfgs.jsonl]
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
import qoc_amd  # noqa: E402
from qoc_amd.engine import Engine  # noqa: E402
from qoc_amd.standard import LBFGS, Adam, TargetStateInfidelity  # noqa: E402

K = 4
TARGET_ERRORS = (0.5, 0.1, 1e-2, 1e-3)
ADAM_LEARNING_RATE = 1e-2  # (tools/bench_multistart.py's)


class HostLBFGS(LBFGS):  # not type(...) is LBFGS: the host loop
    pass


def problem():
    h0, g, psi0, target = bench.make_problem()
    rng = np.random.default_rng(2004)
    g = list(g) + [bench.gue(rng, bench.DIM) for _ in range(K - len(g))]

    def hamiltonian(u, t):
        out = h0
        for k in range(K):
            out = out + u[k] * g[k]
        return out
    u0 = np.stack([0.1 * np.random.default_rng(1000 + b).standard_normal((bench.N_EVAL, K))
                   for b in range(bench.SEEDS_PER_GPU)])
    args = (K, bench.N_EVAL, [TargetStateInfidelity(target[:, :, None])],
            bench.DT * (bench.N_EVAL - 1), hamiltonian, psi0[:, :, None], bench.N_EVAL)
    return args, u0


def run(args, u0, optimizer, count):
    t0 = time.perf_counter()
    result = qoc_amd.grape_schroedinger_discrete_batch(
        *args, u0.copy(), iteration_count=count, log_iteration_step=0, optimizer=optimizer,
        max_control_norms=np.ones(K))
    return time.perf_counter() - t0, result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbfgs.jsonl"))
    parser.add_argument("--iterations", type=int, default=12)
    parser.add_argument("--convergence-iterations", type=int, default=200)
    opts = parser.parse_args()
    args, u0 = problem()
    lines = []

    def emit(**record):
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)

    shape = dict(dim=bench.DIM, steps=bench.N_EVAL - 1, seeds=bench.SEEDS_PER_GPU, controls=K,
                 parameters_per_seed=bench.N_EVAL * K)
    per_iteration = {}
    for label, make, iterations in (
            ("resident LBFGS", LBFGS, opts.iterations),
            ("resident Adam", lambda: Adam(learning_rate=ADAM_LEARNING_RATE), opts.iterations),
            ("host-loop LBFGS", HostLBFGS, max(2, opts.iterations // 3))):
        run(args, u0, make(), 2)  # warm
        # set-up (probing the callable at every quadrature time, ...) cancels in the difference
        short, _ = run(args, u0, make(), iterations)
        long, result = run(args, u0, make(), 3 * iterations)
        per_iteration[label] = (long - short) / (2 * iterations) * 1e3
        emit(measurement="ms_per_iteration", route=label, iterations=iterations,
             ms_per_iteration=round(per_iteration[label], 3),
             best_error_after=3 * iterations, best_error=float(result.best.best_error), **shape)
    emit(measurement="lbfgs_overhead_over_resident_adam",
         ms_per_iteration=round(per_iteration["resident LBFGS"] - per_iteration["resident Adam"], 3),
         relative=round(per_iteration["resident LBFGS"] / per_iteration["resident Adam"] - 1, 4),
         **shape)

    # evaluations to a stated error: every iteration's B costs as the resident loop reads them
    seen = []
    download = Engine.download_costs

    def record(self):
        costs = download(self)
        seen.append(costs.copy())
        return costs
    Engine.download_costs = record
    try:
        for label, optimizer in (("LBFGS", LBFGS()),
                                 ("Adam", Adam(learning_rate=ADAM_LEARNING_RATE))):
            del seen[:]
            _, result = run(args, u0, optimizer, opts.convergence_iterations)
            best = np.minimum.accumulate(np.array(seen), axis=0)  # [iteration, seed]
            median = np.median(best, axis=1)
            needed = {}
            for target in TARGET_ERRORS:
                below = np.nonzero(median < target)[0]
                needed[str(target)] = int(below[0]) + 1 if len(below) else None
            emit(measurement="evaluations_until_median_best_error_below", optimizer=label,
                 evaluations=needed, evaluations_run=len(seen),
                 median_best_error_at_end=float(median[-1]),
                 seeds_finished_early=int(np.sum(result.iterations_run < len(seen))), **shape)
    finally:
        Engine.download_costs = download
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "w") as handle:
        handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
