"""
fuzz_parity.py - TEST TOOLING (parity checker; lives under tests/ because it drives the oracle): random problem shapes, engine (through the C ABI) against the
oracle. Complements the fixed fixtures: sizes 1..32 (any range by argument, up to 256), random step counts / control grids / state
counts / time steps (so that 0..4 squarings occur), all three Magnus policies, Hermitian and
non-Hermitian generators, all state-cost kinds at once. With shapes=True (fuzz_parity.one) each
seed of a draw gets a pulse family of tests/mixed_pulses.py (quiet, bell, spike, square, ramp,
loud) and an amplitude of its own instead of one shared Gaussian scale, so that the steps of one
upload differ in Pade order, squaring count and pivoting regime. With drive=True the drive operators
depend on time as well, G_k(t) = cos(w_k t + k) G_k + sin(w_k t) G'_k with w_k dt in 0.5 .. 1.0 (the
rotating drives of tests/time_dependent_drive.py), and every draw is time dependent; what that adds is
drawn from a generator of its own, seeded by `index`, so the draws of the shared stream - and with
them every problem of the tests that leave drive at False - stay what they are. With costs=True the fixed
cost triple gives way to 1 to 4 random descriptors (kinds, step or final, ragged forbid counts from 1 to
4; tests/state_costs.py: DescriptorCost on the oracle's side), drawn the same way from a generator of
their own.

    python -m tests.fuzz_parity [count] [seed] [nmin] [nmax] [smin] [smax]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import qoc_numpy as onp  # noqa: E402
from qoc_amd.engine import (Engine, QocxError, COST_FORBID, COST_TARGET_COHERENT,  # noqa: E402
                            COST_TARGET_INCOHERENT)
from tests.cases import gue  # noqa: E402
from tests.mixed_pulses import FAMILIES, families  # noqa: E402

NODES = {"M2": (0.5,), "M4": (0.5 - 3 ** 0.5 / 6, 0.5 + 3 ** 0.5 / 6),
         "M6": (0.5 - 15 ** 0.5 / 10, 0.5, 0.5 + 15 ** 0.5 / 10)}


def random_descriptors(own, n, S):
    """1 to 4 random cost descriptors (tests/state_costs.py: DescriptorCost): kind, step or final,
    scale, vectors of their own and - FORBID - ragged counts from 1 to 4."""
    from tests.state_costs import DescriptorCost
    out = []
    for _ in range(int(own.integers(1, 5))):
        kind = int(own.integers(0, 3))
        counts = [int(c) for c in own.integers(1, 5, S)] if kind == COST_FORBID else None
        vec = own.standard_normal((sum(counts) if counts else S, n, 2)) @ np.array([1.0, 1.0j])
        vec /= np.linalg.norm(vec, axis=1, keepdims=True)
        out.append(DescriptorCost(kind, int(own.integers(0, 2)), float(own.uniform(0.3, 1.5)), vec, counts))
    return out


def one(engine, rng, index, nmin=1, nmax=32, smin=1, smax=4, results=None, shapes=False, drive=False,
        costs=False):
    n = int(rng.integers(nmin, nmax + 1))
    N = int(rng.integers(2, 14))
    K = int(rng.integers(1, 4))
    Nc = int(rng.integers(2, 16))
    S = int(rng.integers(smin, smax + 1))
    ces = int(rng.integers(1, 4))
    policy = ("M2", "M2", "M4", "M6")[int(rng.integers(0, 4))]
    hermitian = rng.random() < 0.7
    time_dep = rng.random() < 0.3
    dt = float(10 ** rng.uniform(-2, 0.3))
    scale = float(10 ** rng.uniform(-0.5, 0.8))
    h0 = gue(rng, n) * scale
    g = [gue(rng, n) for _ in range(K)]
    if not hermitian:
        h0 = h0 + 0.3j * scale * gue(rng, n)
        g[0] = g[0] + 0.2j * gue(rng, n)
    omega = float(rng.uniform(0.5, 4.0))
    T = dt * (N - 1)
    if drive:
        time_dep = True
        own = np.random.default_rng([index, 0x6472697665])
        g_sin = [gue(own, n) for _ in range(K)]
        if not hermitian:
            g_sin[0] = g_sin[0] + 0.2j * gue(own, n)
        g_omega = np.sort(own.uniform(0.5, 1.0, K)) / dt

    def g_at(t):
        if not drive:
            return g
        return [np.cos(g_omega[k] * t + k) * g[k] + np.sin(g_omega[k] * t) * g_sin[k] for k in range(K)]

    def hamiltonian(u, t):
        base = h0 * (1 + 0.3 * np.cos(omega * t)) if time_dep else h0
        gt = g_at(t)
        return base + sum(u[k] * gt[k] for k in range(K))

    init = rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))
    init /= np.linalg.norm(init, axis=1, keepdims=True)
    targ = rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))
    targ /= np.linalg.norm(targ, axis=1, keepdims=True)
    forb = rng.standard_normal((S, 2, n)) + 1j * rng.standard_normal((S, 2, n))
    forb /= np.linalg.norm(forb, axis=2, keepdims=True)
    count = (N - 1) // ces
    descs = [dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=0.7, vectors=targ)]
    ocosts = [onp.TargetStateInfidelity(targ[:, :, None], cost_multiplier=0.7)]
    if count > 0:
        descs += [dict(kind=COST_TARGET_INCOHERENT, step_cost=1, scale=1.3 / count, vectors=targ),
                  dict(kind=COST_FORBID, step_cost=1, scale=0.9 / (count * S),
                       vectors=forb.reshape(-1, n), counts=[2] * S)]
        ocosts += [onp.TargetStateInfidelityTime(N, targ[:, :, None], neglect_relative_pahse=True,
                                                 cost_eval_step=ces, cost_multiplier=1.3),
                   onp.ForbidStates(forb[:, :, :, None], N, cost_eval_step=ces,
                                    cost_multiplier=0.9)]
    if costs:
        ocosts = random_descriptors(np.random.default_rng([index, 0x636F737473]), n, S)
        descs = [c.descriptor() for c in ocosts]
    if time_dep:
        times = [j * dt + c * dt for j in range(N - 1) for c in NODES[policy]]
        h0s = np.stack([h0 * (1 + 0.3 * np.cos(omega * t)) for t in times])
        gs = np.stack([np.stack(g_at(t)).reshape(K, n, n) for t in times])
    else:
        h0s, gs = h0[None], np.stack(g)[None]
    engine.set_schroedinger_problem(n, S, K, Nc, N, T, h0s, gs, init, costs=descs,
                                    cost_eval_step=ces, magnus_policy=policy)
    tag = "n={} N={} Nc={} K={} S={} ces={} {} herm={} tdep={} dt={:.3g} |H|={:.3g}".format(
        n, N, Nc, K, S, ces, policy, hermitian, time_dep, dt, scale)
    if drive:
        tag += " drive w dt=" + ",".join("{:.2f}".format(w * dt) for w in g_omega)
    if costs:
        tag += " costs " + ",".join("{}{}{}".format("CIF"[c.kind], "s" if c.step_cost else "f", c.counts or "")
                                    for c in ocosts)
    if shapes:
        # (peak amplitude three times the Gaussian scale of the default draw: its 3 sigma)
        picks = [(FAMILIES[int(rng.integers(0, len(FAMILIES)))], 3 * float(10 ** rng.uniform(-1, 0.5)))
                 for _ in range(2)]
        controls = np.stack([families(Nc, K, amp, rng, quiet_sigma=0.02 * amp)[name]
                             for name, amp in picks])
        tag += " " + " ".join("{}:{:.3g}".format(name, amp) for name, amp in picks)
    else:
        controls = float(10 ** rng.uniform(-1, 0.5)) * rng.standard_normal((2, Nc, K))
    try:
        cost, grads, final = engine.evaluate(controls, want_grad=True)
    except QocxError as exc:
        if exc.code == -5:  # more than 2^10 squarings per step: rejected by design
            return None, tag
        raise
    problem = onp.SchroedingerProblem(T, hamiltonian, init[:, :, None], N, control_eval_count=Nc,
                                      costs=ocosts, cost_eval_step=ces, magnus_policy=policy,
                                      control_count=K)
    if results is not None:
        results.append((cost, grads, final))
    worst = 0.0
    for b in range(2):
        err, gr, fin = onp.evaluate_with_grad(problem, controls[b])
        e_cost = abs(err - cost[b]) / max(1.0, abs(err))
        e_fin = np.max(np.abs(fin[:, :, 0] - final[b])) / max(np.max(np.abs(fin)), 1e-300)
        e_grad = np.max(np.abs(gr - grads[b])) / max(np.max(np.abs(gr)), 1e-3)
        worst = max(worst, e_cost / 1e-10, e_fin / 1e-10, e_grad / 1e-8)
    return worst, tag


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    nmin = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    nmax = int(sys.argv[4]) if len(sys.argv) > 4 else 32
    smin = int(sys.argv[5]) if len(sys.argv) > 5 else 1
    smax = int(sys.argv[6]) if len(sys.argv) > 6 else 4
    rng = np.random.default_rng(seed)
    engine = Engine(0)
    bad = skipped = 0
    overall = 0.0
    for index in range(count):
        worst, tag = one(engine, rng, index, nmin, nmax, smin, smax)
        if worst is None:
            skipped += 1
            continue
        overall = max(overall, worst)
        if worst > 1.0:
            bad += 1
            print("FAIL x{:.2f} of tolerance: {}".format(worst, tag), flush=True)
    print("{} cases ({} rejected for capacity), {} failures, worst {:.2e} of tolerance "
          "(cost/states 1e-10, grads 1e-8)".format(count, skipped, bad, overall))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
