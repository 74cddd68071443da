"""
action_costs_cases.py - TEST INFRASTRUCTURE (NumPy only): the problems of the matrix-free route under
step costs and several costs (qoc_amd/csrc/qocx_action_costs.hip, knob "action_costs"), imported by
tests/test_action_costs_cases_host.py (CPU: the conditions below), tests/test_action_costs_model.py
(CPU: the model) and tests/test_gpu_action_costs.py (GPU).

The fixture is that of tests/test_gpu_action.py::problem - Hermitian operators of 1-norm 1, DT = 0.05,
K = 2, psi0 = e_0, three seeds at amplitudes 1e-3, 1 and 5, so the Taylor degrees span about 8 to 15 - at
n = 17, 20, 32 with cost_eval_step 3 at N = 13 (12 steps: the final step IS a cost step) and N = 14 (13
steps: it is not). Each carries the nine named descriptor sets of tests/state_costs.py at S = 1, built by
its _nominal_set recipe (forbid counts 1, 3 and 2) and balanced as its descriptor_set balances them.

Conditions (tests/test_action_costs_cases_host.py, the oracle alone - those of
tests/test_state_costs_host.py): every descriptor of a set of several holds >= 10 % of the gradient at
every seed, and every misreading of the cost table (state_costs.mutants) moves the oracle gradient by
>= 1e-3 relative on every (set, n, N). Where a draw of the random inputs misses one, the shape takes the
next (DRAWS): inputs are chosen, no condition is loosened.

Nothing here is imported by the product.
"""

import numpy as np

from oracle import qoc_numpy as onp
from tests import state_costs as sc

K, DT, CES = 2, 0.05, 3
SIZES = (17, 20, 32)
STEP_COUNTS = (13, 14)  # N: (N - 1) % CES == 0 - the final step is a cost step - and != 0
AMPLITUDES = (1e-3, 1.0, 5.0)
SETS = sc.SETS
MULTI_SETS = sc.MULTI_SETS
# at S = 1 one final target of either kind is the unit adjoint's: it keeps the two-sided kernels
UNIT_SETS = tuple(s for s in SETS if sc.unit_adjoint_applies(s, 1))
NEW_SETS = tuple(s for s in SETS if s not in UNIT_SETS)
assert UNIT_SETS == ("final_incoherent", "final_coherent") and len(NEW_SETS) == 7

# (n, N): which draw of the random inputs the shape uses (default 0), as state_costs.DRAWS
DRAWS = {}

_problems = {}


def hermitian(rng, n):
    m = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    m = (m + m.conj().T) / 2
    return m / onp.one_norm(m)


def build(n, N, draw=None):
    """The problem at Hilbert size n and N system steps, in the dict shape of state_costs.build (so that
    its descriptor_set, evaluate and mutants take it). "controls" :: (3, N, K)."""
    draw = DRAWS.get((n, N), 0) if draw is None else draw
    key = (n, N, draw)
    if key in _problems:
        return _problems[key]
    rng = np.random.default_rng([n, N, draw, 0x61637473])
    h0 = hermitian(rng, n)
    g = np.stack([hermitian(rng, n) for _ in range(K)])
    init = np.eye(n, dtype=np.complex128)[:1]
    vec = dict(A=sc._unit_vectors(rng, 1, n), B=sc._unit_vectors(rng, 1, n))
    for i, start in enumerate((0, 1, 2)):
        vec["F%d" % i] = sc._unit_vectors(rng, sum(sc.ragged_counts(1, start)), n)
    controls = rng.uniform(-1, 1, (3, N, K)) * np.array(AMPLITUDES)[:, None, None]
    p = dict(n=n, S=1, N=N, Nc=N, K=K, T=DT * (N - 1), dt=DT, ces=CES, kind="plain", policy="M2",
             h0=h0, g=g, init=init, vec=vec, controls=controls, count=(N - 1) // CES, quadratic=None,
             draw=draw)
    _problems[key] = p
    return p


def costs_of(name, p):
    """The named set as balanced DescriptorCosts (state_costs.descriptor_set on this problem)."""
    return sc.descriptor_set(name, p)


def references(name, p):
    """[(error, grads (N, K), final (1, n, 1))] of the three seeds by the oracle: computed once."""
    key = ("refs", name)
    if key not in p:
        costs = costs_of(name, p)
        p[key] = [sc.evaluate(p, costs, b) for b in range(len(AMPLITUDES))]
    return p[key]


def descriptors(name, p):
    """What Engine.set_schroedinger_problem takes as costs."""
    return [c.descriptor() for c in costs_of(name, p)]


def set_problem(engine, p, descs, **kw):
    engine.set_schroedinger_problem(p["n"], 1, K, p["N"], p["N"], p["T"], p["h0"][None], p["g"][None],
                                    p["init"], costs=descs, cost_eval_step=kw.pop("cost_eval_step", CES), **kw)
