"""
action_grad_cases.py - TEST INFRASTRUCTURE: the seeded problems whose results on the matrix-free route
(qoc_amd/csrc/qocx_action.hip) are recorded bit for bit under tests/golden/action_grad/ by
tools/record_action_grad_bits.py and compared by tests/test_gpu_action_grad_bits.py. They are built for the
gradient kernel: its loop over the terms rho_i, whose trip counts are the degree m of a step, and its LDS,
whose size is the largest degree the buffers hold.

n = 17, 25 (padded lanes) and 32 (a full wave); K = 1 .. 4; three seeds, 13 steps. ||G_k||_1 = 1 and
||H0||_1 = 2e-8, so that the controls alone decide a step's bound and a pulse can begin at degree 1. Three
pulse shapes:

  ramp  the knots climb from 4e-9 to 0.29 (spectral bound of a step, knob "action_degree" at its default) and
        fall in the last step: the first seed runs m = 1, 2, .. 12, 11 - no two neighbouring steps at one degree;
  flat  every step of every seed at degree 8;
  top   knob "action_degree" = 0, the 1-norm alone: the knots climb to 1.0, the last steps run at m = 18 - the
        most a step can have, and what sizes the gradient kernel's LDS.

tests/test_action_grad_cases_host.py shows on the CPU, by tests/action_degree_model.py, that the step tables
hold these degrees.

Nothing here is imported by the product.
"""

import os

import numpy as np

from oracle import qoc_numpy as onp

N, DT, B = 14, 0.05, 3  # 13 steps
T = DT * (N - 1)
H0_NORM = 2e-8
SEED_SCALES = (1.0, 0.9, 0.75)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "action_grad")
NAMES = ("cost", "grad", "final")

# the bound of a step AT THE KNOTS, without H0's share: the spectral bound (rule 1) or the 1-norm (rule 0)
RAMP = (4e-9, 8e-9, 2e-6, 1e-4, 1.1e-3, 5.9e-3, 1.61e-2, 3.59e-2, 6.41e-2, 1.159e-1, 1.641e-1, 2.459e-1, 2.941e-1, 1.26e-1)
FLAT = (5.6e-2,) * N
TOP = (1e-8, 2e-8, 5e-6, 2e-4, 1.5e-3, 6e-3, 1.7e-2, 4e-2, 1e-1, 2.5e-1, 5e-1, 8e-1, 1.0, 1.0)
SHAPES = dict(ramp=(RAMP, 1), flat=(FLAT, 1), top=(TOP, 0))  # (knot levels, knob "action_degree")

CASES = ([(n, K, "ramp") for n in (17, 25, 32) for K in (1, 2, 3, 4)]
         + [(25, 2, "flat"), (32, 3, "flat")]
         + [(17, 1, "top"), (25, 4, "top"), (32, 2, "top")])

_cache = {}


def hermitian(rng, n):
    m = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    m = (m + m.conj().T) / 2
    return m / onp.one_norm(m)


def case(n, K, shape):
    key = (n, K, shape)
    if key in _cache:
        return _cache[key]
    levels, rule = SHAPES[shape]
    rng = np.random.default_rng([n, K, sorted(SHAPES).index(shape), 0x67726164])
    h0 = hermitian(rng, n) * H0_NORM
    g = [hermitian(rng, n) for _ in range(K)]
    psi0 = np.eye(n, dtype=np.complex128)[:1]
    target = rng.standard_normal((1, n)) + 1j * rng.standard_normal((1, n))
    target /= np.linalg.norm(target)
    # what a unit of |u_k| adds to the bound the rule reads
    weight = np.array([float(np.abs(np.linalg.eigvalsh(m)).max()) if rule else onp.one_norm(m) for m in g])
    share = rng.uniform(0.5, 1.0, (B, K))
    share /= share.sum(axis=1, keepdims=True)  # a seed's channels split its level; signs constant in time
    sign = rng.choice([-1.0, 1.0], (B, K))
    controls = (np.array(SEED_SCALES)[:, None, None] * np.array(levels)[None, :, None]
                * (sign * share / (DT * weight))[:, None, :])
    p = dict(n=n, K=K, shape=shape, rule=rule, h0=h0, g=g, psi0=psi0, target=target, T=T, controls=controls)
    _cache[key] = p
    return p


def set_problem(engine, p):
    from qoc_amd.engine import COST_TARGET_COHERENT
    engine.set_knob("action_degree", p["rule"])
    engine.set_schroedinger_problem(
        p["n"], 1, p["K"], N, N, p["T"], p["h0"][None], np.stack(p["g"])[None], p["psi0"],
        costs=[dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=p["target"])])


def golden_path(n, K, shape, directory=GOLDEN):
    return os.path.join(directory, "n%d_k%d_%s.npz" % (n, K, shape))
