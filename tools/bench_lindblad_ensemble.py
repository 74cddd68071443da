"""
bench_lindblad_ensemble.py - GPU-BOX TOOLING: robust GRAPE over a Hamiltonian ensemble on the
Lindblad path (qoc_amd.standard.HamiltonianEnsemble, qocx_lindblad_set_ensemble) against the ways to
get the same numbers without it.

The problem of bench.py's BASELINE configs[3] (bench.lindblad_problem(): n = 16, 501 system
evaluations, two Lindblad operators, two real controls, one final TargetDensityInfidelity), 64
seeds. The ensemble has M = 9 members: 3 detunings (delta in {-0.05, 0, 0.05} on the number
operator a^H a, J = 1) x 3 drive amplitude scales (0.97, 1, 1.03). Modes, forward + gradient, three
runs per line (each the mean over its timed evaluations):

    (a) the ensemble, 64 seeds (expansion + 576 items + reduction)
    (b) the same 576 items as a plain (K_r + J)-channel problem, host-expanded controls
    (c) one multi-start GRAPE iteration with the ensemble (the loop of
        grape_lindblad_discrete_batch, Adam), device resident
    (d) the same on the host loop (a subclass of Adam is "another plugin")
        (both on one evaluator, timed as the difference of 2 I and I iterations: the driver's
        one-time setup is left out)
    (e) 9 separate evaluations of 64 seeds, one per member (delta D folded into H0, the seeds'
        controls scaled on the host)
    (p) a plain evaluation WITHOUT an ensemble (configs[3] as bench.py times it), in a fresh
        process per library: this build, and - with --parent-library PATH - the library of the
        parent commit, alternating. Runs without an ensemble must launch what they launched before,
        so the two must agree within the parent's own run-to-run scatter.

One JSON line per mode and one check line.

    python tools/bench_lindblad_ensemble.py [--parent-library PATH] > profiles/lindblad_ensemble.jsonl
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
import bench  # noqa: E402
from qoc_amd import engine as engine_mod  # noqa: E402

REPEATS = 3          # timed evaluations per run
RUNS = 3             # runs per line
GRAPE_ITERATIONS = 4
SEEDS = bench.LB_SEEDS
NEW_SYMBOLS = ("qocx_lindblad_set_ensemble", "qocx_lindblad_ensemble_download_members")


def seeds():
    return np.stack([0.1 * np.random.default_rng(1000 + b).standard_normal(
        (bench.LB_EVAL, bench.K_CTRL)) for b in range(SEEDS)])


def ensemble_parts():
    deltas = np.array([-0.05, 0.0, 0.05])
    amps = np.array([0.97, 1.0, 1.03])
    offsets = np.repeat(deltas, 3)[:, None]                          # member 3 i + j: delta_i, amp_j
    scales = np.tile(amps, 3)[:, None].repeat(bench.K_CTRL, axis=1)
    a = np.diag(np.sqrt(np.arange(1, bench.LB_DIM)), 1).astype(np.complex128)
    return a.conj().T @ a, offsets, scales, np.full(9, 1.0 / 9)


def set_problem(engine, h0, g):
    _, _, gam, ops, rho0, target = bench.lindblad_problem()
    engine.set_lindblad_problem(
        bench.LB_DIM, 1, len(g), bench.LB_EVAL, bench.LB_EVAL, bench.DT * (bench.LB_EVAL - 1), h0, g,
        gam, ops, rho0, costs=[dict(kind=engine_mod.COST_TARGET_DENSITY, step_cost=0, scale=1.0,
                                    vectors=target)])


def runs_of(call):
    """RUNS means over REPEATS calls each, after one warm call; ms."""
    call()
    out = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        for _ in range(REPEATS):
            call()
        out.append(round((time.perf_counter() - t0) / REPEATS * 1e3, 3))
    return out


def line(mode, route, runs, **more):
    row = dict(mode=mode, route=route, n=bench.LB_DIM, system_evals=bench.LB_EVAL, runs_ms=runs,
               ms_min=min(runs), ms_max=max(runs), timed_evaluations_per_run=REPEATS, **more)
    print(json.dumps(row), flush=True)
    return row


def plain_child(library):
    """Mode (p) in this process: the library at `library`, no ensemble anywhere."""
    try:
        engine_mod.load_library(library)
    except AttributeError:  # the parent commit's library: it has no ensemble symbols to bind
        for name in NEW_SYMBOLS:
            engine_mod.SIGNATURES.pop(name, None)
        engine_mod.load_library(library)
    engine = engine_mod.Engine(0)
    h0, g = bench.lindblad_problem()[:2]
    set_problem(engine, h0, g)
    u = seeds()
    runs = runs_of(lambda: engine.evaluate_lindblad(u))
    engine.close()
    print(json.dumps(dict(library=library, runs_ms=runs)), flush=True)


def plain_comparison(parent_library):
    """This build and the parent's library in fresh processes, alternating, two visits each."""
    results = {}
    libraries = [("this build", engine_mod.LIBRARY_PATH)]
    if parent_library:
        libraries.insert(0, ("parent commit", os.path.abspath(parent_library)))
    for _ in range(2):
        for label, path in libraries:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-library", path],
                                 check=True, capture_output=True, text=True, timeout=300).stdout
            results.setdefault(label, []).extend(json.loads(out.strip().splitlines()[-1])["runs_ms"])
    for label, runs in results.items():
        line("p", "plain qocx_eval_lindblad, no ensemble, {} (fresh processes)".format(label), runs,
             seeds=SEEDS)
    if parent_library:
        parent, this = results["parent commit"], results["this build"]
        print(json.dumps(dict(
            check="no-ensemble evaluation, this build against the parent commit's library",
            parent_ms=[min(parent), max(parent)], this_ms=[min(this), max(this)],
            within_parent_scatter=bool(min(this) <= max(parent)))), flush=True)


def main(parent_library):
    from qoc_amd.core import batch as batch_mod
    from qoc_amd.core import device
    from qoc_amd.core.lindbladdiscrete import GrapeLindbladBatchResult, _ResidentOps
    from qoc_amd.standard import Adam, HamiltonianEnsemble, TargetDensityInfidelity

    class PluginAdam(Adam):
        pass

    plain_comparison(parent_library)  # (before this process opens the device)
    h0, g, gam, ops, rho0, target = bench.lindblad_problem()
    number, offsets, scales, weights = ensemble_parts()
    M = offsets.shape[0]
    u = seeds()
    engine = engine_mod.Engine(0)
    # (a) the ensemble
    set_problem(engine, h0, list(g) + [number])
    engine.set_lindblad_ensemble(scales, offsets, weights)
    line("a", "HamiltonianEnsemble (qocx_lindblad_set_ensemble)",
         runs_of(lambda: engine.evaluate_lindblad(u)), seeds=SEEDS, members=M, real_controls=2,
         fixed_channels=1)
    engine.evaluate_lindblad(u, want_grad=False)
    e_members = engine.lindblad_ensemble_member_costs()
    # (b) the plain 3-channel problem on host-expanded controls
    set_problem(engine, h0, list(g) + [number])
    r = np.empty((SEEDS, M, bench.LB_EVAL, 3))
    r[..., :2] = scales[None, :, None, :] * u[:, None]
    r[..., 2] = offsets[None, :, None, 0]
    r = r.reshape(SEEDS * M, bench.LB_EVAL, 3)
    line("b", "plain (K_r + J)-channel problem, host-expanded controls",
         runs_of(lambda: engine.evaluate_lindblad(r)), seeds=SEEDS * M, real_controls=3)
    p_errors = engine.evaluate_lindblad(r, want_grad=False)[0]
    print(json.dumps(dict(check="ensemble members vs plain items",
                          bitwise_equal=bool(np.array_equal(e_members.reshape(-1), p_errors)),
                          max_abs_diff=float(np.max(np.abs(e_members.reshape(-1) - p_errors))))),
          flush=True)

    # (e) one problem per member, 64 seeds each, one after the other
    def members():
        for m in range(M):
            set_problem(engine, h0 + offsets[m, 0] * number, g)
            engine.evaluate_lindblad(scales[m][None, None, :] * u)
    line("e", "9 separate evaluations of 64 seeds (one problem per member)", runs_of(members),
         seeds=SEEDS, members=M, real_controls=2)
    engine.close()

    # (c), (d) multi-start GRAPE
    def linear(c, t):
        return h0 + c[0] * g[0] + c[1] * g[1]
    ens = HamiltonianEnsemble(linear, perturbations=number[None], offsets=offsets,
                              control_scales=scales, weights=weights)
    T = bench.DT * (bench.LB_EVAL - 1)
    norms = np.full(2, 1.0)
    comm, pstate, params = batch_mod.prepare_seeds(u, False, 2, bench.LB_EVAL, T, norms, None, None)
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

    def timed(run, count):
        gc.collect()
        t0 = time.perf_counter()
        run(count)
        return time.perf_counter() - t0
    for key, label, run in (("c", "grape_lindblad_discrete_batch loop + ensemble, device resident",
                             resident),
                            ("d", "grape_lindblad_discrete_batch loop + ensemble, host loop (Adam "
                                  "subclass)", host)):
        run(1)  # warm
        runs = []
        for _ in range(RUNS):
            t1, t2 = timed(run, GRAPE_ITERATIONS), timed(run, 2 * GRAPE_ITERATIONS)
            runs.append(round((t2 - t1) / GRAPE_ITERATIONS * 1e3, 3))
        print(json.dumps(dict(mode=key, route=label, seeds=SEEDS, members=M, n=bench.LB_DIM,
                              system_evals=bench.LB_EVAL, iterations=GRAPE_ITERATIONS,
                              runs_ms_per_iteration=runs, ms_min=min(runs), ms_max=max(runs))),
              flush=True)
    ev.backend.close()


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--parent-library", default=None,
                        help="libqocx.so built from the parent commit: mode (p) times it too")
    parser.add_argument("--plain-library", default=None, help=argparse.SUPPRESS)
    args = parser.parse_args()
    if args.plain_library:
        plain_child(args.plain_library)
    else:
        main(args.parent_library)
