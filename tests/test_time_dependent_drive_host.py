"""
CPU tests (-m "not gpu") of tests/time_dependent_drive.py: the references the GPU tests of
time-dependent drive operators G_k(t) compare against are themselves right on such drives, and a
kernel that read G_k at a wrong time could not pass them.

  * the oracle's gradient against central differences of its own forward pass, and the Lindblad
    model's likewise;
  * the oracle's forward pass against 40-digit arithmetic (mpmath);
  * the discrimination condition: for every configuration the GPU tests run, every way of reading
    G_k at a wrong time (time_dependent_drive.mutants) moves the oracle's gradient by >= 1e-3
    relative - 1e5 times the parity gate - and its final states by >= 1e-5;
  * the host's sampling (core/structure.py: probe_hamiltonian) and the CPU backend of the host
    tests (tests/oracle_backend.py) on a g with nt > 1.
"""

import numpy as np
import pytest

from oracle import qoc_numpy as onp
from tests import time_dependent_drive as tdd


def central_differences(f, u, h=1e-5):
    out = np.empty(u.shape)
    for idx in np.ndindex(*u.shape):
        up, dn = u.copy(), u.copy()
        up[idx] += h
        dn[idx] -= h
        out[idx] = (f(up) - f(dn)) / (2 * h)
    return out


@pytest.mark.parametrize("hermitian", [True, False])
@pytest.mark.parametrize("policy", ["M2", "M4", "M6"])
def test_oracle_gradient_against_finite_differences(policy, hermitian):
    """n = 5, N = 6, Nc = 4, K = 2, a quiet and a loud seed. Gate 1e-8 relative: central differences
    at h = 1e-5 scatter by 2.5e-10 .. 2e-9 on these problems (truncation in h^2, round-off 1e-16 |C| /
    h = 1e-11 per evaluation, against gradients of 1e-2 .. 1)."""
    p = tdd.drive_problem(5, 6, 4, 2, 2, policy=policy, hermitian=hermitian)
    for u in tdd.controls(p, 2, quiet=0.12, loud=2.0):
        _, grads, _ = onp.evaluate_with_grad(p["oracle"], u)
        fd = central_differences(lambda v: onp.evaluate(p["oracle"], v)[0], u)
        rel = np.max(np.abs(grads - fd)) / np.max(np.abs(fd))
        print("{} hermitian={}: gradient against differences {:.2e}".format(policy, hermitian, rel))
        assert rel < 1e-8


def test_lindblad_model_gradient_against_finite_differences():
    """tests/lindblad_model.py with g_of_t, n = 4, N = 4, subdivision 4; gate 1e-7 relative (the
    differences scatter by ~1e-9 here: the cost is a sum over more arithmetic)."""
    from qoc_amd.engine import Engine
    from tests import lindblad_model as lm
    q = tdd.lindblad_drive_problem(4, 4, 3, 2, 2, 2, 4, Engine.lindblad_stage_times)
    system = tdd.lindblad_model_system(q)
    u = q["controls"][2]

    def cost(v):
        return lm.evaluate_with_grad(system, v, q["rho0"], q["T"], q["N"], q["mcosts"], 1,
                                     want_grad=False, subdivision=4)[0]

    _, grads, _ = lm.evaluate_with_grad(system, u, q["rho0"], q["T"], q["N"], q["mcosts"], 1,
                                        subdivision=4)
    fd = central_differences(cost, u)
    rel = np.max(np.abs(grads - fd)) / np.max(np.abs(fd))
    print("Lindblad model gradient against differences {:.2e}".format(rel))
    assert rel < 1e-7


def test_oracle_forward_against_extended_precision():
    """M2, n = 3, N = 4: the final states against the product of expm(-i dt H(u(t_j + dt / 2),
    t_j + dt / 2)) in 40-digit arithmetic, to 1e-13."""
    import mpmath
    mpmath.mp.dps = 40
    p = tdd.drive_problem(3, 4, 3, 2, 2, hermitian=False, costs="final")
    prob = p["oracle"]
    for u in tdd.controls(p, 2, loud=2.0):
        _, final = onp.evaluate(prob, u)
        psi = mpmath.matrix(p["init"].T.tolist())
        for step in range(p["N"] - 1):
            t = step * p["dt"] + 0.5 * p["dt"]
            uk = onp.interpolate_linear_set(t, prob.control_eval_times, u)
            h = mpmath.matrix(p["hamiltonian"](uk, t).tolist())
            psi = mpmath.expm(h * (-1j * mpmath.mpf(p["dt"]))) * psi
        ref = np.array([[complex(psi[i, s]) for i in range(3)] for s in range(p["S"])])
        err = np.max(np.abs(final[:, :, 0] - ref))
        print("oracle forward against mpmath {:.2e}".format(err))
        assert err < 1e-13


# ---- the discrimination condition ------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(tdd.CONFIGS))
def test_wrong_time_index_cannot_pass(name):
    """Per configuration, with Hermitian G and the general costs and with non-Hermitian G and the one
    final target, seed by seed: every mutant moves the gradient by >= 1e-3 relative; every mutant of
    the forward pass moves the final states by >= 1e-5; "mirror nodes" is the identity under M2 (to
    the rounding of (2 j + 1) dt - t). n = 1 with a Hermitian H: the evolution is a phase common to
    all states, every cost is constant and the gradient zero - the states alone tell there."""
    for hermitian, costs in ((True, "general"), (False, "final")):
        p = tdd.configured(name, hermitian, costs)
        assert not np.allclose(p["g"][0], p["g"][1])
        muts = tdd.mutants(p)
        for b, u in enumerate(tdd.config_controls(p, 3 if name.startswith("pipe") else 2)):
            ref = onp.evaluate_with_grad(p["oracle"], u)
            for mutant, prob in muts.items():
                grad, states = tdd.relative_moves(ref, onp.evaluate_with_grad(prob, u))
                if mutant == "mirror nodes" and p["policy"] == "M2":
                    assert grad < 1e-12 and states < 1e-12
                    continue
                if p["n"] == 1 and hermitian:
                    assert np.max(np.abs(ref[1])) < 1e-14
                else:
                    assert grad >= 1e-3, (name, hermitian, b, mutant, grad)
                if mutant == "gradient-only shift":
                    assert states == 0.0
                else:
                    assert states >= 1e-5, (name, hermitian, b, mutant, states)


@pytest.mark.parametrize("name", ["two_n20", "four_n40", "envelope_n20", "envelope_n40"])
def test_quiet_and_loud_seeds_straddle_theta_5(name):
    """What the GPU tests then read from pade_orders(): the quiet seed's bound dt (||H0||_1 + sum_k
    |u_k| max_t ||G_k||_1) stays below theta_5 at every knot, the loud seed's step generators
    exceed it in the 1-norm itself."""
    p = tdd.configured(name)
    u = tdd.controls(p, 2)
    h0n = max(onp.one_norm(m) for m in p["h0"])
    bound = p["dt"] * (h0n + np.max(np.sum(np.abs(u[0]) * tdd.g_norms(p), axis=1)))
    assert bound < tdd.THETA5
    loud = tdd.step_norms(p, u[1])
    assert np.max(loud) > tdd.THETA5
    if p["envelope"]:  # the drive grows 20-fold: low orders early, squarings on the late steps only
        late = [onp.pade_scale_count(v) for v in tdd.step_norms(p, tdd.envelope_controls(p)[1])]
        assert late[-1] > 0 and not any(late[:len(late) // 2])


# ---- the host's samples ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("policy", ["M2", "M6"])
def test_probe_hamiltonian_samples_a_rotating_drive(policy):
    """A constant H0 and a rotating drive: nt == len(times) (the time axis is not collapsed because h0
    alone is constant), and g is the builder's table."""
    from qoc_amd.core.structure import probe_hamiltonian
    p = tdd.drive_problem(4, 5, 3, 2, 1, policy=policy)
    d = p["drive"]
    h0, g = probe_hamiltonian(lambda u, t: d.h0 + sum(u[k] * d.g_at(t)[k] for k in range(2)),
                              4, 2, False, p["times"])
    assert h0.shape[0] == g.shape[0] == len(p["times"])
    assert np.all(h0 == d.h0)
    assert np.max(np.abs(g - p["g"])) < 1e-15
    h0, g = probe_hamiltonian(p["hamiltonian"], 4, 2, False, p["times"])
    assert np.array_equal(h0, p["h0"]) and np.max(np.abs(g - p["g"])) < 1e-15


@pytest.mark.parametrize("policy", ["M2", "M4", "M6"])
def test_oracle_backend_reads_g_by_time(policy):
    """tests/oracle_backend.py, the engine of the host tests, on the builder's tables: the oracle's
    own numbers on the callable."""
    from tests.oracle_backend import OracleBackend
    p = tdd.drive_problem(4, 5, 3, 2, 2, policy=policy, hermitian=False)
    u = tdd.controls(p, 2, loud=2.0)
    backend = OracleBackend()
    tdd.set_engine_problem(backend, p)
    backend.upload_controls(u)
    backend.eval_resident(True)
    cost, grads, final = backend.download_results(True)
    for b in range(2):
        err, gr, fin = onp.evaluate_with_grad(p["oracle"], u[b])
        assert abs(err - cost[b]) < 1e-14
        assert np.max(np.abs(gr - grads[b])) < 1e-14 * max(1.0, np.max(np.abs(gr)))
        assert np.max(np.abs(fin[:, :, 0] - final[b])) < 1e-14


# ---- quadratic terms, ensembles, Lindblad, fuzz --------------------------------------------------------------------

def test_member_oracle_gradient_against_finite_differences():
    """The oracle of an ensemble member with quadratic terms (d H / d u_k taken at the controls under
    evaluation) on rotating G_k(t) and D_j(t): gate 1e-8 relative, as above."""
    p = tdd.drive_problem(5, 6, 4, 5, 2)
    scales, offsets, _ = tdd.ensemble_of(p)
    quad = tdd.quadratic_terms(p)
    u = tdd.controls(p, 2, channels=3)[1]
    prob = tdd.member_oracle(p, u, quad, scales[1], offsets[1])
    _, grads, _ = onp.evaluate_with_grad(prob, u)
    fd = central_differences(lambda v: onp.evaluate(prob, v)[0], u)
    assert np.max(np.abs(grads - fd)) / np.max(np.abs(fd)) < 1e-8
    linear = tdd.member_oracle(p, u, None, scales[1], offsets[1])
    assert abs(onp.evaluate(linear, u)[0] - onp.evaluate(prob, u)[0]) > 1e-4  # the terms matter


@pytest.mark.parametrize("spec", [dict(n=4, N=3, Nc=2, K=2, S=1, L=2, subdivision=4, complex_ops=False),
                                  dict(n=16, N=3, Nc=2, K=2, S=2, L=2, subdivision=1),
                                  dict(n=21, N=4, Nc=3, K=2, S=2, L=3, subdivision=1)],
                         ids=lambda s: "n{n}_sub{subdivision}".format(**s))
def test_lindblad_wrong_stage_cannot_pass(spec):
    """The Lindblad twin: g_stages frozen at t = 0 or read one stage late moves the model's densities
    by >= 1e-6 and its gradient by >= 1e-10 - 1e6 and 1e3 times what the GPU tests allow (1e-12; 1e-10
    of max(|g|, 1e-3)) -, for the two louder seeds of three problems that
    tests/test_gpu_lindblad_time_dependent_drive.py runs (and hands to the engine frozen, too).
    (At n = 1 nothing can: a scalar density commutes with every G_k.)"""
    from qoc_amd.engine import Engine
    from tests import lindblad_model as lm
    q = tdd.lindblad_drive_problem(stage_times=Engine.lindblad_stage_times, **spec)
    times, g_of_t = np.asarray(q["times"]), q["g_of_t"]

    def late(t):  # the sample of the next stage time in the device's table
        return g_of_t(times[min(int(np.argmin(np.abs(times - t))) + 1, len(times) - 1)])

    def run(g, b):
        system = tdd.lindblad_model_system(q, g)
        return lm.evaluate_with_grad(system, q["controls"][b], q["rho0"], q["T"], q["N"], q["mcosts"],
                                     1, subdivision=q["subdivision"])

    for b in (1, 2):
        ref = run(g_of_t, b)
        for name, g in (("frozen", lambda t: g_of_t(0.0)), ("late", late)):
            _, grads, final = run(g, b)
            assert np.max(np.abs(final - ref[2])) >= 1e-6, (name, b)
            assert np.max(np.abs(grads - ref[1])) >= 1e-10, (name, b)


class _Rejecting(object):
    """An engine that turns every draw of fuzz_parity.one away: the draw's tag is all that is wanted."""

    def set_schroedinger_problem(self, *args, **kw):
        self.g = np.asarray(args[7])

    def evaluate(self, *args, **kw):
        from qoc_amd.engine import QocxError
        raise QocxError(-5, "not evaluated")


@pytest.mark.parametrize("seed, kw, tag, then", [
    (2024, {}, "n=4 N=8 Nc=11 K=2 S=4 ces=3 M2 herm=False tdep=False dt=1.44 |H|=3.91",
     0.5631835177416028),
    (6464, dict(nmin=33, nmax=64),
     "n=37 N=4 Nc=6 K=3 S=4 ces=2 M2 herm=True tdep=False dt=0.0581 |H|=2.46", 0.8898187776734643),
    (4040, dict(shapes=True),
     "n=9 N=7 Nc=8 K=3 S=3 ces=1 M2 herm=True tdep=True dt=0.0627 |H|=5.28 quiet:0.309 bell:3.65",
     0.08442326789002585),
    (65256, dict(nmin=65, nmax=256, smax=3),
     "n=92 N=13 Nc=14 K=2 S=3 ces=2 M2 herm=True tdep=False dt=0.0209 |H|=0.772", 0.5491702171748951)])
def test_fuzz_draws_without_drive_are_what_they_were(seed, kw, tag, then):
    """fuzz_parity.one(drive=False): the third draw of the seeds the existing fuzz tests use, and the
    state of the shared stream behind it, as recorded before `drive` existed; with drive=True the
    same stream state follows (its parameters come from a generator of its own) and g varies."""
    from tests import fuzz_parity
    engine = _Rejecting()
    for drive in (False, True):
        rng = np.random.default_rng(seed)
        tags = [fuzz_parity.one(engine, rng, index, drive=drive, **kw)[1] for index in range(3)]
        assert rng.random() == then
        if not drive:
            assert tags[2] == tag
        else:
            assert " drive" in tags[2] and engine.g.shape[0] > 1
            assert not np.allclose(engine.g[0], engine.g[1])
