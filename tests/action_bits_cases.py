"""
action_bits_cases.py - TEST INFRASTRUCTURE: the seeded problems whose results on the matrix-free route
(qoc_amd/csrc/qocx_action.hip) are recorded bit for bit under tests/golden/action_bits/ by
tools/record_action_bits.py and compared by tests/test_gpu_action_bits.py.

n = 17 (padded rows) and 32; K = 1 (the second register image zero-filled), 2 (the exact build) and 3 (one
control read per step); three seeds; 24 steps. ||H0||_1 = ||G_k||_1 = 1 and the control amplitudes ramp
along the pulse, so that the degree of a step climbs within every pulse while the 1-norm bound of the
loudest step stays below theta_18 (tests/test_action_bits_cases_host.py).

Nothing here is imported by the product.
"""

import os

import numpy as np

from oracle import qoc_numpy as onp

N, DT, B = 25, 0.05, 3  # 24 steps
SIZES = (17, 32)
CONTROL_COUNTS = (1, 2, 3)
PEAKS = (6.0, 10.0, 16.0)  # sum_k |u_k| at the end of the ramp, per seed
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "action_bits")
NAMES = ("cost", "grad", "final")

_cache = {}


def hermitian(rng, n):
    m = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    m = (m + m.conj().T) / 2
    return m / onp.one_norm(m)


def case(n, K):
    key = (n, K)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(7000 + 10 * n + K)
    h0, g = hermitian(rng, n), [hermitian(rng, n) for _ in range(K)]
    psi0 = np.eye(n, dtype=np.complex128)[:1]
    target = rng.standard_normal((1, n)) + 1j * rng.standard_normal((1, n))
    target /= np.linalg.norm(target)
    ramp = np.linspace(0.03, 1.0, N)
    shape = rng.uniform(0.7, 1.0, (B, N, K)) * rng.choice([-1.0, 1.0], (B, N, K))
    controls = shape * ramp[None, :, None] * (np.array(PEAKS) / K)[:, None, None]
    p = dict(n=n, K=K, h0=h0, g=g, psi0=psi0, target=target, T=DT * (N - 1), controls=controls)
    _cache[key] = p
    return p


def set_problem(engine, p):
    from qoc_amd.engine import COST_TARGET_COHERENT
    engine.set_schroedinger_problem(
        p["n"], 1, p["K"], N, N, p["T"], p["h0"][None], np.stack(p["g"])[None], p["psi0"],
        costs=[dict(kind=COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=p["target"])])


def golden_path(n, K, name, directory=GOLDEN):
    return os.path.join(directory, "n%d_k%d_%s.npy" % (n, K, name))
