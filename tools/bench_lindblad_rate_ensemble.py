"""
bench_lindblad_rate_ensemble.py - GPU-BOX TOOLING: a Lindblad ensemble with per-member dissipation
rates (HamiltonianEnsemble(..., rate_scales=c), qocx_lindblad_set_ensemble_rates) against the same
ensemble without rates and against the way to get its numbers without the feature, and the gate
that runs without rates cost what they cost on the parent commit.

The problem and the ensemble of tools/bench_lindblad_ensemble.py (bench.py's BASELINE configs[3]:
n = 16, 501 system evaluations, two Lindblad operators, two real controls, 64 seeds; M = 9 members =
3 detunings x 3 drive amplitude scales, J = 1). The rates: member m scales (T1 decay, dephasing) by
factors from {0.5, 1, 2}, every pair of factors once. Forward + gradient, three runs per line (each
the mean over its timed evaluations), ranges reported.

    (p)  a plain 64-seed evaluation, no ensemble                        } fresh process per library:
    (g)  the ensemble WITHOUT rates: stand-alone evaluation             } this build and - with
         (want_final=False) and one resident multi-start iteration      } --parent-library PATH - the
                                                                        } parent commit's, alternating,
                                                                        } the order swapped per visit
    (a)  the ensemble with rates, stand-alone evaluation (want_final=False)
    (a0) the same ensemble without rates, same process
    (e)  9 separate evaluations of 64 seeds, one problem per member with its own dissipators
         (what per-member rates cost without the feature)
    (c)  one multi-start GRAPE iteration with rates, device resident
    (c0) the same without rates
    (d)  (c) on the host loop (a subclass of Adam is "another plugin")

Runs without rates launch the kernels they launched before (the rates have kernels of their own,
in files and code objects of their own, behind an argument of their own), so (p) and (g) of this
build must lie within the parent's own run-to-run scatter: the check lines.

    python tools/bench_lindblad_rate_ensemble.py [--parent-library PATH] \
        > profiles/lindblad_rate_ensemble.jsonl
    python tools/bench_lindblad_rate_ensemble.py --parent-library PATH --gate-only 5 \
        > profiles/lindblad_rate_ensemble_gate.jsonl
"""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import bench_lindblad_ensemble as base  # noqa: E402
from qoc_amd import engine as engine_mod  # noqa: E402

RUNS = base.RUNS
GRAPE_ITERATIONS = base.GRAPE_ITERATIONS
SEEDS = base.SEEDS
NEW_SYMBOLS = ("qocx_lindblad_set_ensemble_rates",)


def rate_scales():
    """(9, 2): every pair of factors from {0.5, 1, 2} for (decay, dephasing) once."""
    f = np.array([0.5, 1.0, 2.0])
    return np.stack([np.tile(f, 3)[[1, 2, 0, 2, 0, 1, 0, 1, 2]], np.repeat(f, 3)], axis=1)


def grape_setup(rates):
    """The evaluator and the two loops of grape_lindblad_discrete_batch on it."""
    from qoc_amd.core import batch as batch_mod
    from qoc_amd.core import device
    from qoc_amd.core.lindbladdiscrete import GrapeLindbladBatchResult, _ResidentOps
    from qoc_amd.standard import Adam, HamiltonianEnsemble, TargetDensityInfidelity

    class PluginAdam(Adam):
        pass

    h0, g, gam, ops, rho0, target = bench.lindblad_problem()
    number, offsets, scales, weights = base.ensemble_parts()

    def linear(c, t):
        return h0 + c[0] * g[0] + c[1] * g[1]
    ens = HamiltonianEnsemble(linear, perturbations=number[None], offsets=offsets,
                              control_scales=scales, weights=weights, rate_scales=rates)
    T = bench.DT * (bench.LB_EVAL - 1)
    norms = np.full(2, 1.0)
    comm, pstate, params = batch_mod.prepare_seeds(base.seeds(), False, 2, bench.LB_EVAL, T, norms,
                                                   None, None)
    ev = device.LindbladEvaluator(T, rho0, bench.LB_EVAL, hamiltonian=ens,
                                  lindblad_data=lambda t: (gam, ops), control_count=2,
                                  control_eval_count=bench.LB_EVAL,
                                  costs=[TargetDensityInfidelity(target)], control_bounds=norms)
    assert ev.resident_capable()

    def resident(count):
        batch_mod.run_batch_resident(_ResidentOps(ev.backend), Adam(learning_rate=1e-3),
                                     params.copy(), pstate, count, 0, 0, comm,
                                     GrapeLindbladBatchResult(SEEDS))

    def host(count):
        batch_mod.run_batch_host(ev, None, PluginAdam(learning_rate=1e-3), params.copy(), pstate,
                                 count, 0, 0, comm, GrapeLindbladBatchResult(SEEDS))
    return ev, resident, host


def iteration_runs(run):
    """ms per iteration, RUNS times: the difference of 2 I and I iterations (the driver's one-time
    setup is left out)."""
    def timed(count):
        gc.collect()
        t0 = time.perf_counter()
        run(count)
        return time.perf_counter() - t0
    run(1)  # warm
    runs = []
    for _ in range(RUNS):
        t1, t2 = timed(GRAPE_ITERATIONS), timed(2 * GRAPE_ITERATIONS)
        runs.append(round((t2 - t1) / GRAPE_ITERATIONS * 1e3, 3))
    return runs


def iteration_line(mode, route, runs, **more):
    row = dict(mode=mode, route=route, seeds=SEEDS, members=9, n=bench.LB_DIM,
               system_evals=bench.LB_EVAL, iterations=GRAPE_ITERATIONS, runs_ms_per_iteration=runs,
               ms_min=min(runs), ms_max=max(runs), **more)
    print(json.dumps(row), flush=True)
    return row


def gate_child(library):
    """Modes (p) and (g) in this process, on the library at `library`: nothing here sets rates."""
    try:
        engine_mod.load_library(library)
    except AttributeError:  # the parent commit's library: no rates symbol to bind
        for name in NEW_SYMBOLS:
            engine_mod.SIGNATURES.pop(name, None)
        engine_mod.load_library(library)
    h0, g = bench.lindblad_problem()[:2]
    number, offsets, scales, weights = base.ensemble_parts()
    u = base.seeds()
    engine = engine_mod.Engine(0)
    base.set_problem(engine, h0, g)
    plain = base.runs_of(lambda: engine.evaluate_lindblad(u))
    base.set_problem(engine, h0, list(g) + [number])
    engine.set_lindblad_ensemble(scales, offsets, weights)
    alone = base.runs_of(lambda: engine.evaluate_lindblad(u, want_final=False))
    engine.close()
    ev, resident, _ = grape_setup(None)
    iteration = iteration_runs(resident)
    ev.backend.close()
    print(json.dumps(dict(library=library, plain=plain, ensemble=alone, iteration=iteration)),
          flush=True)


def gate(parent_library):
    """This build and the parent's library in fresh processes, alternating, two visits each; the second
    visit in the opposite order, so that neither library is always the one that runs second."""
    results = {}
    libraries = [("this build", engine_mod.LIBRARY_PATH)]
    if parent_library:
        libraries.insert(0, ("parent commit", os.path.abspath(parent_library)))
    for visit in range(2):
        for label, path in (libraries if visit == 0 else libraries[::-1]):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--gate-library", path],
                                 check=True, capture_output=True, text=True, timeout=400).stdout
            got = json.loads(out.strip().splitlines()[-1])
            for key in ("plain", "ensemble", "iteration"):
                results.setdefault((key, label), []).extend(got[key])
    names = dict(plain=("p", "plain qocx_eval_lindblad, no ensemble"),
                 ensemble=("g", "ensemble without rates, qocx_eval_lindblad, want_final=False"),
                 iteration=("g", "ensemble without rates, resident multi-start iteration"))
    for (key, label), runs in results.items():
        base.line(names[key][0], "{}, {} (fresh processes)".format(names[key][1], label), runs,
                  seeds=SEEDS)
    if parent_library:
        for key in ("plain", "ensemble", "iteration"):
            parent, this = results[(key, "parent commit")], results[(key, "this build")]
            # within the parent's scatter: the median of this build's runs is no slower than the
            # slowest of the parent's (a median, so that one stray run on either side decides nothing)
            print(json.dumps(dict(
                check="{}: this build against the parent commit's library".format(names[key][1]),
                parent_ms=[min(parent), max(parent)], this_ms=[min(this), max(this)],
                parent_median_ms=float(np.median(parent)), this_median_ms=float(np.median(this)),
                visit_order=["parent, this", "this, parent"],  # (the runs of a line are in visit order)
                within_parent_scatter=bool(np.median(this) <= max(parent)))), flush=True)
    return results


def gates(parent_library, count):
    """The gate alone, `count` times over, and the runs of all of them pooled per library: a single gate
    has six runs per library, two of them a process's faster first resident iteration."""
    pooled = {}
    for _ in range(count):
        for key, runs in gate(parent_library).items():
            pooled.setdefault(key, []).extend(runs)
    for (what, label), runs in sorted(pooled.items()):
        print(json.dumps(dict(pooled=what, library=label, runs=len(runs), median_ms=float(np.median(runs)),
                              ms_min=min(runs), ms_max=max(runs))), flush=True)


def main(parent_library):
    gate(parent_library)  # (before this process opens the device)
    h0, g, gam, ops, rho0, target = bench.lindblad_problem()
    number, offsets, scales, weights = base.ensemble_parts()
    rates = rate_scales()
    M = offsets.shape[0]
    u = base.seeds()
    engine = engine_mod.Engine(0)
    base.set_problem(engine, h0, list(g) + [number])
    engine.set_lindblad_ensemble(scales, offsets, weights)
    a0 = base.line("a0", "ensemble without rates, want_final=False",
                   base.runs_of(lambda: engine.evaluate_lindblad(u, want_final=False)),
                   seeds=SEEDS, members=M, subintervals=engine.lindblad_last_subintervals())
    engine.set_lindblad_ensemble_rates(rates)
    a = base.line("a", "ensemble with rates (qocx_lindblad_set_ensemble_rates), want_final=False",
                  base.runs_of(lambda: engine.evaluate_lindblad(u, want_final=False)),
                  seeds=SEEDS, members=M, subintervals=engine.lindblad_last_subintervals())
    print(json.dumps(dict(check="ensemble with rates against the same ensemble without (reported, "
                                "not asserted)",
                          without_ms=[a0["ms_min"], a0["ms_max"]], with_ms=[a["ms_min"], a["ms_max"]],
                          subintervals=[a0["subintervals"], a["subintervals"]])), flush=True)
    engine.evaluate_lindblad(u, want_grad=False, want_final=False)
    e_members = engine.lindblad_ensemble_member_costs()

    # (e) one problem per member: its own dissipators, delta D folded into H0, scaled controls
    def set_member(m):
        engine.set_lindblad_problem(
            bench.LB_DIM, 1, len(g), bench.LB_EVAL, bench.LB_EVAL, bench.DT * (bench.LB_EVAL - 1),
            h0 + offsets[m, 0] * number, g, rates[m] * gam, ops, rho0,
            costs=[dict(kind=engine_mod.COST_TARGET_DENSITY, step_cost=0, scale=1.0, vectors=target)])

    def members():
        for m in range(M):
            set_member(m)
            engine.evaluate_lindblad(scales[m][None, None, :] * u)
    base.line("e", "9 separate evaluations of 64 seeds (one problem per member, own dissipators)",
              base.runs_of(members), seeds=SEEDS, members=M)
    worst = 0.0
    for m in range(M):
        set_member(m)
        cost = engine.evaluate_lindblad(scales[m][None, None, :] * u, want_grad=False)[0]
        worst = max(worst, float(np.max(np.abs(cost - e_members[:, m]))))
    print(json.dumps(dict(check="member costs of the ensemble with rates vs the separate problems "
                                "(D folded into H0: another grid, two converged integrations)",
                          max_abs_diff=worst)), flush=True)
    engine.close()

    # (c), (c0), (d): multi-start GRAPE
    ev, resident, host = grape_setup(rates)
    iteration_line("c", "grape_lindblad_discrete_batch loop + ensemble with rates, device resident",
                   iteration_runs(resident))
    iteration_line("d", "grape_lindblad_discrete_batch loop + ensemble with rates, host loop (Adam "
                        "subclass)", iteration_runs(host))
    ev.backend.close()
    ev, resident, _ = grape_setup(None)
    iteration_line("c0", "grape_lindblad_discrete_batch loop + ensemble without rates, device "
                         "resident", iteration_runs(resident))
    ev.backend.close()


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--parent-library", default=None,
                        help="libqocx.so built from the parent commit: the gate times it too")
    parser.add_argument("--gate-only", type=int, default=0, metavar="COUNT",
                        help="the gate alone, COUNT times, with the runs pooled per library")
    parser.add_argument("--gate-library", default=None, help=argparse.SUPPRESS)
    args = parser.parse_args()
    if args.gate_library:
        gate_child(args.gate_library)
    elif args.gate_only:
        gates(args.parent_library, args.gate_only)
    else:
        main(args.parent_library)
