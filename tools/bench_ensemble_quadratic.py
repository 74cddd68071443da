"""
bench_ensemble_quadratic.py - GPU-BOX TOOLING: robust GRAPE over an ensemble of QUADRATIC
Hamiltonians (HamiltonianEnsemble(QuadraticHamiltonian(...)): qocx_set_quadratic_terms +
qocx_set_ensemble) against the way to get the same numbers without the combination.

The Piccolo-shaped problem of tools/bench_quadratic.py WITH its two quadratic terms (the AC-Stark
term in |eps_sb|^2): n = 24, three complex controls (K_r = 6 real channels), 1000 steps,
MagnusPolicy.M2, one final TargetStateInfidelity. The ensemble of tools/bench_ensemble.py: M = 9
members, 3 qubit detunings (J = 1) x 3 drive amplitude scales. 64 seeds. Modes:

    (a)  the ensemble, 64 seeds, forward + gradient (expansion + 576 items + reduction)
    (a2) the same with a per-member scale of the Stark terms (quadratic_scales)
    (b)  9 separate 64-seed QuadraticHamiltonian evaluations on host-scaled controls, the detuning
         folded into H0, combined on the host (what a user does without the combination)
    (c)  one multi-start GRAPE iteration with the ensemble (the loop of
         grape_schroedinger_discrete_batch, Adam), device resident (real controls)
    (d)  the same on the host loop (a subclass of Adam is "another plugin")
         (both timed as in tools/bench_ensemble.py: the difference of 2 I and I iterations)

Every evaluation mode is timed RUNS times (each the mean of REPEATS evaluations): the line carries
all the runs, so the run-to-run scatter can be read off it. --commit LABEL is recorded in every line.
--baseline-library PATH runs mode (b) alone on another build of libqocx.so (an earlier commit's, to
keep the comparison from resting on the code under test).

    python tools/bench_ensemble_quadratic.py --commit LABEL > profiles/ensemble_quadratic.jsonl
"""
import argparse
import ctypes
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qoc_amd import engine  # noqa: E402
from qoc_amd.core import batch as batch_mod  # noqa: E402
from qoc_amd.core import device  # noqa: E402
from qoc_amd.core.schroedingerdiscrete import (GrapeSchroedingerBatchResult,  # noqa: E402
                                               _ResidentOps)
from qoc_amd.standard import (Adam, HamiltonianEnsemble, QuadraticHamiltonian,  # noqa: E402
                              TargetStateInfidelity)
from tools.bench_ensemble import ensemble_parts  # noqa: E402
from tools.bench_quadratic import NC, NT, N_STEPS, SEEDS, T, piccolo, starts  # noqa: E402

REPEATS = 10
RUNS = 3
GRAPE_ITERATIONS = 10


class PluginAdam(Adam):
    pass


def timed_runs(evaluate):
    evaluate()  # warm: code objects, buffers
    runs = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        for _ in range(REPEATS):
            evaluate()
        runs.append(round((time.perf_counter() - t0) / REPEATS * 1e3, 3))
    return dict(ms_per_evaluation=sorted(runs)[len(runs) // 2], ms_per_evaluation_runs=runs,
                timed_evaluations=REPEATS)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--commit", default="unknown")
    parser.add_argument("--baseline-library", default=None)
    opts = parser.parse_args()
    if opts.baseline_library is not None:
        # an earlier build: bind the symbols it has (mode (b) needs none of the later ones)
        lib = ctypes.CDLL(opts.baseline_library)
        for name in [s for s in engine.SIGNATURES if not hasattr(lib, s)]:
            del engine.SIGNATURES[name]
        engine.load_library(opts.baseline_library)

    linear, number, offsets, scales, psi0, target = ensemble_parts()
    _, terms, _, _ = piccolo()
    M, N, n = offsets.shape[0], N_STEPS + 1, NT * NC
    weights = np.full(M, 1.0 / M)
    costs = [TargetStateInfidelity(target)]
    kw = dict(control_eval_count=N, costs=costs)
    u = starts(SEEDS, real=False)
    common = dict(seeds=SEEDS, members=M, n=n, steps=N_STEPS, real_controls=6, fixed_channels=1,
                  quadratic_terms=len(terms), commit=opts.commit,
                  library=opts.baseline_library or "this build")

    def emit(row):
        print(json.dumps(dict(row, **common)), flush=True)

    # (b) one evaluator per member: controls scaled on the host, the detuning folded into H0
    def member_base(m):
        return QuadraticHamiltonian(lambda c, t: linear(c, t) + offsets[m, 0] * number, terms)
    evs = [device.SchroedingerEvaluator(T, member_base(m), psi0, N, control_count=3,
                                        complex_controls=True, **kw) for m in range(M)]
    scaled = [scales[m][None, None, :] * u for m in range(M)]
    separate = {}

    def run_separate():
        cost, grad, members = 0.0, 0.0, []
        for m, ev in enumerate(evs):
            e_m, g_m, _, _ = ev.evaluate_batch(scaled[m])
            members.append(e_m)
            cost = cost + weights[m] * e_m
            grad = grad + (weights[m] * scales[m])[None, None, :] * g_m
        separate.update(cost=cost, grad=grad, members=np.stack(members, axis=1))
    emit(dict(mode="b", route="9 separate QuadraticHamiltonian evaluations of 64 seeds, host-scaled "
                               "controls, detuning in H0, host-combined", **timed_runs(run_separate)))
    for ev in evs:
        ev.backend.close()
    del evs
    if opts.baseline_library is not None:
        return

    # (a), (a2) the ensemble over the quadratic base
    base = QuadraticHamiltonian(linear, terms)
    ens = HamiltonianEnsemble(base, perturbations=number[None], offsets=offsets,
                              control_scales=scales)
    ev_e = device.SchroedingerEvaluator(T, ens, psi0, N, control_count=3, complex_controls=True,
                                        **kw)
    assert ev_e.quadratic_terms is not None and ev_e.ensemble is ens
    emit(dict(mode="a", route="HamiltonianEnsemble(QuadraticHamiltonian) (qocx_set_quadratic_terms + "
                               "qocx_set_ensemble)", **timed_runs(lambda: ev_e.evaluate_batch(u))))
    # the members of (a) against the separate evaluations of (b) (reported, not asserted)
    e_cost, e_grad, _, _ = ev_e.evaluate_batch(u)
    e_members = ev_e.member_errors()
    print(json.dumps(dict(
        check="ensemble vs separate member evaluations",
        members_max_abs_diff=float(np.max(np.abs(e_members - separate["members"]))),
        cost_max_abs_diff=float(np.max(np.abs(e_cost - separate["cost"]))),
        grad_rel_diff=float(np.max(np.abs(e_grad - separate["grad"]))
                            / np.max(np.abs(separate["grad"]))))), flush=True)
    ev_e.backend.close()
    del ev_e
    stark = np.tile(np.array([0.9, 1.0, 1.1]), 3)[:, None].repeat(len(terms), axis=1)
    ens_c = HamiltonianEnsemble(base, perturbations=number[None], offsets=offsets,
                                control_scales=scales, quadratic_scales=stark)
    ev_c = device.SchroedingerEvaluator(T, ens_c, psi0, N, control_count=3, complex_controls=True,
                                        **kw)
    emit(dict(mode="a2", route="the same with quadratic_scales (qocx_set_ensemble_quadratic_scales)",
              **timed_runs(lambda: ev_c.evaluate_batch(u))))
    ev_c.backend.close()
    del ev_c

    # (c), (d) multi-start GRAPE on real controls (Re / Im as six real controls)
    def linear_real(rr, t):
        return linear(rr[0::2] + 1j * rr[1::2], t)
    ens_real = HamiltonianEnsemble(QuadraticHamiltonian(linear_real, terms),
                                   perturbations=number[None], offsets=offsets,
                                   control_scales=np.repeat(scales, 2, axis=1))
    u_real = np.empty((SEEDS, N, 6))
    u_real[..., 0::2], u_real[..., 1::2] = u.real, u.imag
    comm, pstate, params = batch_mod.prepare_seeds(u_real, False, 6, N, T, np.full(6, 0.5), None,
                                                   None)
    ev_g = device.SchroedingerEvaluator(T, ens_real, psi0, N, control_count=6,
                                        latency_mode=SEEDS * M <= 128, **kw)  # as the driver
    assert ev_g.resident_capable() and ev_g.quadratic_terms is not None

    def resident(count):
        batch_mod.run_batch_resident(_ResidentOps(ev_g.backend), Adam(learning_rate=1e-3),
                                     params.copy(), pstate, count, 0, 0, comm,
                                     GrapeSchroedingerBatchResult(SEEDS))

    def host(count):
        batch_mod.run_batch_host(ev_g, None, PluginAdam(learning_rate=1e-3), params.copy(), pstate,
                                 count, 0, 0, comm, GrapeSchroedingerBatchResult(SEEDS))

    def best_of(run, count, tries=3):
        out = None
        for _ in range(tries):
            gc.collect()
            t0 = time.perf_counter()
            run(count)
            dt = time.perf_counter() - t0
            out = dt if out is None else min(out, dt)
        return out
    for key, label, run in (("c", "grape_schroedinger_discrete_batch loop, device resident", resident),
                            ("d", "grape_schroedinger_discrete_batch loop, host loop (Adam subclass)",
                             host)):
        run(1)  # warm
        runs = []
        for _ in range(RUNS):
            t1 = best_of(run, GRAPE_ITERATIONS)
            t2 = best_of(run, 2 * GRAPE_ITERATIONS)
            runs.append(round((t2 - t1) / GRAPE_ITERATIONS * 1e3, 3))
        emit(dict(mode=key, route=label, iterations=GRAPE_ITERATIONS,
                  ms_per_iteration=sorted(runs)[len(runs) // 2], ms_per_iteration_runs=runs))
    ev_g.backend.close()


if __name__ == "__main__":
    main()
