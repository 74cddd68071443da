"""
bench_ensemble.py - GPU-BOX TOOLING: robust GRAPE over a Hamiltonian ensemble
(qoc_amd.standard.HamiltonianEnsemble, qocx_set_ensemble) against the ways to get the same numbers
without it.

The Piccolo-shaped problem of tools/bench_quadratic.py without its quadratic terms: n = 24, three
complex controls (K_r = 6 real channels), 1000 steps, MagnusPolicy.M2, one final
TargetStateInfidelity. The ensemble has M = 9 members: 3 qubit detunings (delta in {-1, 0, 1} x
2 pi 50 kHz on the transmon number operator, J = 1) x 3 drive amplitude scales (0.97, 1, 1.03).
64 seeds. Modes, forward + gradient:

    (a) the ensemble, 64 seeds (expansion + 576 items + reduction)
    (b) the plain (K_r + J)-channel problem at 64 x 9 seeds, host-expanded controls
    (c) one multi-start GRAPE iteration with the ensemble (the loop of
        grape_schroedinger_discrete_batch, Adam), device resident (real controls: Re / Im of the
        complex ones as 6 real controls)
    (d) the same on the host loop (a subclass of Adam is "another plugin")
        (both on one evaluator, timed as the difference of 2 I and I iterations, best of 3: the
        driver's one-time setup - the evaluator, HBM buffers for 576 items - is left out)
    (e) 9 separate evaluations of 64 seeds, one per member (the plain base Hamiltonian of each
        member, its own evaluator)

One JSON line per mode, and one check line.

    python tools/bench_ensemble.py > profiles/ensemble.jsonl
"""
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qoc_amd.core import batch as batch_mod  # noqa: E402
from qoc_amd.core import device  # noqa: E402
from qoc_amd.core.schroedingerdiscrete import (GrapeSchroedingerBatchResult,  # noqa: E402
                                               _ResidentOps)
from qoc_amd.standard import Adam, HamiltonianEnsemble, TargetStateInfidelity  # noqa: E402
from tools.bench_quadratic import NC, NT, N_STEPS, SEEDS, T, piccolo, starts  # noqa: E402

REPEATS = 10
GRAPE_ITERATIONS = 10
DETUNING = 2 * np.pi * 5e-5  # rad / ns: 50 kHz


class PluginAdam(Adam):
    pass


def ensemble_parts():
    linear, _, psi0, target = piccolo()
    number = np.kron(np.diag(np.arange(NT, dtype=np.float64)), np.eye(NC)).astype(np.complex128)
    deltas = np.array([-1.0, 0.0, 1.0]) * DETUNING
    amps = np.array([0.97, 1.0, 1.03])
    offsets = np.repeat(deltas, 3)[:, None]          # member 3 i + j: delta_i, amp_j
    scales = np.tile(amps, 3)[:, None].repeat(3, axis=1)
    return linear, number, offsets, scales, psi0, target


def time_evaluations(ev, controls, repeats):
    ev.evaluate_batch(controls)  # warm: code objects, buffers
    t0 = time.perf_counter()
    for _ in range(repeats):
        ev.evaluate_batch(controls)
    return (time.perf_counter() - t0) / repeats * 1e3


def main():
    linear, number, offsets, scales, psi0, target = ensemble_parts()
    M, N, n = offsets.shape[0], N_STEPS + 1, NT * NC
    ens = HamiltonianEnsemble(linear, perturbations=number[None], offsets=offsets,
                              control_scales=scales)
    costs = [TargetStateInfidelity(target)]
    kw = dict(control_eval_count=N, costs=costs)
    ev_e = device.SchroedingerEvaluator(T, ens, psi0, N, control_count=3, complex_controls=True,
                                        **kw)
    u = starts(SEEDS, real=False)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
    ms = time_evaluations(ev_e, u, REPEATS)
    emit(dict(mode="a", route="HamiltonianEnsemble (qocx_set_ensemble)", seeds=SEEDS, members=M,
              n=n, steps=N_STEPS, real_controls=6, fixed_channels=1, timed_evaluations=REPEATS,
              ms_per_evaluation=round(ms, 3)))

    # (b) the plain 7-channel problem (Re / Im of the 3 drives, then the detuning channel)
    def plain(r, t):
        return linear(r[0:6:2] + 1j * r[1:6:2], t) + r[6] * number
    ev_p = device.SchroedingerEvaluator(T, plain, psi0, N, control_count=7, **kw)
    r = np.empty((SEEDS, M, N, 7))
    r[..., 0:6:2] = scales[None, :, None, :] * u.real[:, None]
    r[..., 1:6:2] = scales[None, :, None, :] * u.imag[:, None]
    r[..., 6] = offsets[None, :, None, 0]
    r = r.reshape(SEEDS * M, N, 7)
    ms = time_evaluations(ev_p, r, REPEATS)
    emit(dict(mode="b", route="plain (K_r + J)-channel problem, host-expanded controls",
              seeds=SEEDS * M, n=n, steps=N_STEPS, real_controls=7, timed_evaluations=REPEATS,
              ms_per_evaluation=round(ms, 3)))
    # the members of (a) are the items of (b) (reported, not asserted)
    ev_e.evaluate_batch(u, want_grad=False)
    e_members = ev_e.member_errors()
    p_errors, _, _, _ = ev_p.evaluate_batch(r, want_grad=False)
    print(json.dumps(dict(check="ensemble members vs plain items",
                          bitwise_equal=bool(np.array_equal(e_members.reshape(-1), p_errors)),
                          max_abs_diff=float(np.max(np.abs(e_members.reshape(-1) - p_errors))))),
          flush=True)

    ev_p.backend.close()
    del ev_p

    # (c), (d) multi-start GRAPE on real controls (Re / Im as six real controls)
    def linear_real(rr, t):
        return linear(rr[0::2] + 1j * rr[1::2], t)
    ens_real = HamiltonianEnsemble(linear_real, perturbations=number[None], offsets=offsets,
                                   control_scales=np.repeat(scales, 2, axis=1))
    u_real = np.empty((SEEDS, N, 6))
    u_real[..., 0::2], u_real[..., 1::2] = u.real, u.imag
    comm, pstate, params = batch_mod.prepare_seeds(u_real, False, 6, N, T, np.full(6, 0.5), None,
                                                   None)
    ev_g = device.SchroedingerEvaluator(T, ens_real, psi0, N, control_count=6,
                                        latency_mode=SEEDS * M <= 128, **kw)  # as the driver
    assert ev_g.resident_capable()

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
    for key, label, run in (("c", "grape_schroedinger_discrete_batch loop + ensemble, device "
                                  "resident", resident),
                            ("d", "grape_schroedinger_discrete_batch loop + ensemble, host loop "
                                  "(Adam subclass)", host)):
        run(1)  # warm
        t1 = best_of(run, GRAPE_ITERATIONS)
        t2 = best_of(run, 2 * GRAPE_ITERATIONS)
        ms = (t2 - t1) / GRAPE_ITERATIONS * 1e3
        emit(dict(mode=key, route=label, seeds=SEEDS, members=M, n=n, steps=N_STEPS,
                  real_controls=6, iterations=GRAPE_ITERATIONS, ms_per_iteration=round(ms, 3)))
    ev_g.backend.close()
    del ev_g

    # (e) one evaluator per member, 64 seeds each, evaluated one after the other
    evs = [device.SchroedingerEvaluator(T, ens.member(m), psi0, N, control_count=3,
                                        complex_controls=True, **kw) for m in range(M)]
    for ev in evs:
        ev.evaluate_batch(u)  # warm
    t0 = time.perf_counter()
    for _ in range(REPEATS):
        for ev in evs:
            ev.evaluate_batch(u)
    ms = (time.perf_counter() - t0) / REPEATS * 1e3
    emit(dict(mode="e", route="9 separate evaluations of 64 seeds (one evaluator per member)",
              seeds=SEEDS, members=M, n=n, steps=N_STEPS, real_controls=6,
              timed_evaluations=REPEATS, ms_per_evaluation=round(ms, 3)))


if __name__ == "__main__":
    main()
