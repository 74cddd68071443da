"""
bench_lindblad_grape.py - GPU-BOX TOOLING: wall time per iteration of multi-start Lindblad GRAPE at
BASELINE.json configs[3]'s shape (bench.lindblad_problem: n = 16, 501 evaluation points, two
Lindblad operators, K = 2 real controls, the benchmark's 64 seeds), Adam, 10 iterations:

    (a) grape_lindblad_discrete_batch, device-resident route, B = 64;
    (b) the same on the host loop (a subclass of Adam is "another plugin"), B = 64;
    (c) 64 sequential grape_lindblad_discrete runs, timed over 4 seeds and scaled by 16.

One JSON line per mode. Set-up (structure probing, evaluator construction) cancels: each mode runs
10 and 20 iterations and reports the difference per iteration.

    python tools/bench_lindblad_grape.py > profiles/lindblad_grape_batch.jsonl
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import qoc_amd  # noqa: E402
from qoc_amd.standard import Adam, TargetDensityInfidelity  # noqa: E402

ITERATIONS = 10
TIMED_SEEDS = 4  # of mode (c)


class PluginAdam(Adam):
    pass


def main():
    h0, g, gam, ops, rho0, target = bench.lindblad_problem()
    ham = lambda u, t: h0 + u[0] * g[0] + u[1] * g[1]  # noqa: E731
    data = lambda t: (gam, ops)  # noqa: E731
    B, N, K = bench.LB_SEEDS, bench.LB_EVAL, bench.K_CTRL
    T = bench.DT * (N - 1)
    u0 = np.stack([0.1 * np.random.default_rng(1000 + b).standard_normal((N, K)) for b in range(B)])
    common = dict(hamiltonian=ham, lindblad_data=data, log_iteration_step=0,
                  max_control_norms=np.ones(K))

    def costs():
        return [TargetDensityInfidelity(target)]

    def batch(optimizer_class):
        def run(count):
            return qoc_amd.grape_lindblad_discrete_batch(
                K, N, costs(), T, rho0, N, u0.copy(), iteration_count=count,
                optimizer=optimizer_class(learning_rate=1e-3), **common)
        return run

    def sequential(count):
        for b in range(TIMED_SEEDS):
            qoc_amd.grape_lindblad_discrete(K, N, costs(), T, rho0, N, initial_controls=u0[b].copy(),
                                            iteration_count=count,
                                            optimizer=Adam(learning_rate=1e-3), **common)

    modes = [("a", "grape_lindblad_discrete_batch, device resident, B = 64", batch(Adam), 1),
             ("b", "grape_lindblad_discrete_batch, host loop (Adam subclass), B = 64",
              batch(PluginAdam), 1),
             ("c", "64 x grape_lindblad_discrete in sequence, timed over {} seeds and scaled by {}"
              .format(TIMED_SEEDS, B // TIMED_SEEDS), sequential, B // TIMED_SEEDS)]
    per_iteration = {}
    for key, label, run, scale in modes:
        run(2)  # warm: code objects, buffers, grid tables
        t0 = time.perf_counter()
        run(ITERATIONS)
        t1 = time.perf_counter()
        run(2 * ITERATIONS)
        t2 = time.perf_counter()
        ms = ((t2 - t1) - (t1 - t0)) / ITERATIONS * 1e3 * scale
        per_iteration[key] = ms
        print(json.dumps(dict(mode=key, route=label, seeds=B, iterations=ITERATIONS,
                              ms_per_iteration=round(ms, 3),
                              seed_iterations_per_s=round(B / ms * 1e3, 1),
                              setup_ms=round((2 * (t1 - t0) - (t2 - t1)) * scale * 1e3, 1))),
              flush=True)
    print(json.dumps(dict(ratio_a_over_c=round(per_iteration["c"] / per_iteration["a"], 1),
                          ratio_a_over_b=round(per_iteration["b"] / per_iteration["a"], 3),
                          note="ratios of throughput (seed-iterations per second)")), flush=True)


if __name__ == "__main__":
    main()
