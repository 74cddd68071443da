"""
bench_quadratic.py - GPU-BOX TOOLING: Hamiltonians quadratic in the controls on the device
(qoc_amd.standard.QuadraticHamiltonian) against today's opaque route for the same function.

A Piccolo-shaped problem (report.tex:22-32, rotating frame): a transmon with 3 levels (g, e, f) x a
cavity with 8 levels, n = 24; three complex controls eps_ge, eps_ef, eps_sb (K_r = 6 real
controls); the AC-Stark term |eps_sb|^2 (eta_e |e><e| + eta_f |f><f|) as two quadratic terms;
1000 steps, MagnusPolicy.M2, one final TargetStateInfidelity. Modes, forward + gradient:

    (a) quadratic route, 1 seed            (b) quadratic route, 64 seeds
    (c) opaque route, 1 seed               (d) opaque route, 64 seeds
        (the same function wrapped in a plain lambda: the host samples every step generator and
        forms the chain rule from finite differences of the callable)
    (e) one multi-start GRAPE iteration at 64 seeds (grape_schroedinger_discrete_batch, Adam):
        device-resident route (real controls: Re / Im of the complex ones as 6 real controls)
    (f) the same on the host loop (a subclass of Adam is "another plugin")

One JSON line per mode.

    python tools/bench_quadratic.py > profiles/quadratic_hamiltonian.jsonl
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qoc_amd  # noqa: E402
from qoc_amd.core import device  # noqa: E402
from qoc_amd.standard import Adam, QuadraticHamiltonian, TargetStateInfidelity  # noqa: E402

NT, NC = 3, 8            # transmon levels, cavity levels
N_STEPS = 1000
T = 0.5 * N_STEPS        # ns, dt = 0.5
SEEDS = 64
REPEATS = 10             # timed evaluations per quadratic-route mode
GRAPE_ITERATIONS = 5


class PluginAdam(Adam):
    pass


def piccolo():
    """(linear_complex(u, t), quadratic terms, psi0, target) of the Piccolo-shaped problem."""
    two_pi = 2 * np.pi
    chi_e, chi_f = two_pi * -1.0e-3, two_pi * -2.0e-3
    eta_e, eta_f = two_pi * 0.15, two_pi * 0.3
    alpha = two_pi * -0.14
    proj = lambda i, j: np.outer(np.eye(NT)[i], np.eye(NT)[j])  # noqa: E731
    a = np.diag(np.sqrt(np.arange(1, NC)), 1).astype(np.complex128)
    ic = np.eye(NC)
    # rotating frame of the drives: anharmonicity and the dispersive shifts remain
    h0 = (np.kron(alpha * proj(2, 2), ic) + np.kron(proj(1, 1), chi_e * a.conj().T @ a)
          + np.kron(proj(2, 2), chi_f * a.conj().T @ a)).astype(np.complex128)
    ge, ef = np.kron(proj(0, 1), ic), np.kron(proj(1, 2), ic)
    sb = np.kron(proj(2, 0), a)  # |f><g| a
    drives = [ge, ef, sb]

    def linear(u, t):
        out = h0
        for k, d in enumerate(drives):
            out = out + u[k] * d + np.conj(u[k]) * d.conj().T
        return out
    stark = np.kron(eta_e * proj(1, 1) + eta_f * proj(2, 2), ic).astype(np.complex128)
    terms = [(4, 4, stark), (5, 5, stark)]  # |eps_sb|^2 = Re^2 + Im^2
    psi0 = np.zeros((1, NT * NC, 1), dtype=np.complex128)
    psi0[0, 0, 0] = 1.0                      # |g, 0>
    target = np.zeros((1, NT * NC, 1), dtype=np.complex128)
    target[0, 1, 0] = 1.0                    # |g, 1>
    return linear, terms, psi0, target


def starts(count, real):
    rng = np.random.default_rng(2024)
    u = 0.02 * rng.standard_normal((count, N_STEPS + 1, 3))
    if not real:
        u = u + 0.02j * rng.standard_normal((count, N_STEPS + 1, 3))
    return u


def time_evaluations(ev, controls, repeats):
    ev.evaluate_batch(controls)  # warm: code objects, buffers
    t0 = time.perf_counter()
    for _ in range(repeats):
        ev.evaluate_batch(controls)
    return (time.perf_counter() - t0) / repeats * 1e3


def main():
    linear, terms, psi0, target = piccolo()
    quad = QuadraticHamiltonian(linear, terms)
    plain = lambda u, t: quad(u, t)  # noqa: E731
    N = N_STEPS + 1

    def evaluator(h):
        return device.SchroedingerEvaluator(T, h, psi0, N, control_count=3, control_eval_count=N,
                                            complex_controls=True,
                                            costs=[TargetStateInfidelity(target)])
    ev_q, ev_o = evaluator(quad), evaluator(plain)
    assert ev_q.opaque_hamiltonian is None and ev_o.opaque_hamiltonian is plain
    u = starts(SEEDS, real=False)
    rows = []
    for key, label, ev, seeds, repeats in (
            ("a", "quadratic route (qocx_set_quadratic_terms)", ev_q, 1, REPEATS),
            ("b", "quadratic route (qocx_set_quadratic_terms)", ev_q, SEEDS, REPEATS),
            ("c", "opaque route (plain lambda, host-sampled generators)", ev_o, 1, 2),
            ("d", "opaque route (plain lambda, host-sampled generators)", ev_o, SEEDS, 1)):
        if key == "d":  # one timed evaluation, no warm-up (tens of seconds of host work)
            t0 = time.perf_counter()
            ev.evaluate_batch(u[:seeds])
            ms = (time.perf_counter() - t0) * 1e3
        else:
            ms = time_evaluations(ev, u[:seeds], repeats)
        rows.append(dict(mode=key, route=label, seeds=seeds, n=NT * NC, steps=N_STEPS,
                         real_controls=6, quadratic_terms=len(terms), timed_evaluations=repeats,
                         ms_per_evaluation=round(ms, 3),
                         ms_per_seed_evaluation=round(ms / seeds, 4)))
        print(json.dumps(rows[-1]), flush=True)
    # consistency of the two routes on the first seed (reported, not asserted)
    eq, gq, _, _ = ev_q.evaluate_batch(u[:1])
    eo, go, _, _ = ev_o.evaluate_batch(u[:1])
    print(json.dumps(dict(check="quadratic vs opaque route, seed 0", error_diff=float(abs(eq[0] - eo[0])),
                          grad_rel_diff=float(np.max(np.abs(gq - go)) / np.max(np.abs(go))))),
          flush=True)

    # multi-start GRAPE on real controls (Re / Im as six real controls): resident vs host loop
    def linear_real(r, t):
        return linear(r[0::2] + 1j * r[1::2], t)
    quad_real = QuadraticHamiltonian(linear_real, terms)
    u_real = np.empty((SEEDS, N, 6))
    u_real[..., 0::2], u_real[..., 1::2] = u.real, u.imag

    def grape(optimizer_class):
        def run(count):
            return qoc_amd.grape_schroedinger_discrete_batch(
                6, N, [TargetStateInfidelity(target)], T, quad_real, psi0, N, u_real.copy(),
                iteration_count=count, log_iteration_step=0, max_control_norms=np.full(6, 0.5),
                optimizer=optimizer_class(learning_rate=1e-3))
        return run
    for key, label, run in (("e", "grape_schroedinger_discrete_batch, device resident", grape(Adam)),
                            ("f", "grape_schroedinger_discrete_batch, host loop (Adam subclass)",
                             grape(PluginAdam))):
        run(1)  # warm
        t0 = time.perf_counter()
        run(GRAPE_ITERATIONS)
        t1 = time.perf_counter()
        run(2 * GRAPE_ITERATIONS)
        t2 = time.perf_counter()
        ms = ((t2 - t1) - (t1 - t0)) / GRAPE_ITERATIONS * 1e3
        print(json.dumps(dict(mode=key, route=label, seeds=SEEDS, n=NT * NC, steps=N_STEPS,
                              real_controls=6, iterations=GRAPE_ITERATIONS,
                              ms_per_iteration=round(ms, 3),
                              setup_ms=round((2 * (t1 - t0) - (t2 - t1)) * 1e3, 1))), flush=True)


if __name__ == "__main__":
    main()
