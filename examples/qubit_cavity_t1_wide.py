"""
qubit_cavity_t1_wide.py - a gate on a qubit coupled to a 20-level cavity (n = 40) under T1 of both:
move the qubit's excitation into the cavity, |e, 0> -> |g, 1>, with one drive on the qubit and one on
the cavity. n = 40 is above the 32 of the Lindblad engine's default kernels: wide=True takes the
sixteen-wave kernel of 33 <= n <= 64 (time-independent systems, the classic launch; README).

    python examples/qubit_cavity_t1_wide.py        # needs an MI355X and qoc_amd/libqocx.so
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from qoc_amd import grape_lindblad_discrete  # noqa: E402
from qoc_amd.standard import Adam, TargetDensityInfidelity  # noqa: E402

LEVELS = 20                     # of the cavity; n = 2 * LEVELS
EVOLUTION_TIME = 60.0           # nanoseconds
SYSTEM_EVAL_COUNT = 61
CONTROL_EVAL_COUNT = 31
COUPLING = 2 * np.pi * 0.02     # GHz: a swap takes pi / (2 g) = 12.5 ns on resonance
DETUNING = 2 * np.pi * 0.05
T1_QUBIT, T1_CAVITY = 30e3, 100e3  # nanoseconds

A = np.kron(np.eye(2), np.diag(np.sqrt(np.arange(1, LEVELS)), k=1)).astype(np.complex128)
SM = np.kron(np.array([[0, 1], [0, 0]]), np.eye(LEVELS)).astype(np.complex128)
H0 = DETUNING * (SM.conj().T @ SM) + COUPLING * (SM.conj().T @ A + A.conj().T @ SM)
DRIVES = [SM + SM.conj().T, A + A.conj().T]
OPERATORS = np.stack([SM, A])
RATES = np.array([1 / T1_QUBIT, 1 / T1_CAVITY])


def basis_density(qubit, photons):
    rho = np.zeros((1, 2 * LEVELS, 2 * LEVELS), dtype=np.complex128)
    rho[0, qubit * LEVELS + photons, qubit * LEVELS + photons] = 1
    return rho


def hamiltonian(controls, time):
    return H0 + controls[0] * DRIVES[0] + controls[1] * DRIVES[1]


def lindblad_data(time):
    return RATES, OPERATORS


def main(iteration_count=200):
    # (|e> is the second qubit level: index 1)
    initial, target = basis_density(1, 0), basis_density(0, 1)
    rng = np.random.default_rng(0)
    start = 0.01 * rng.standard_normal((CONTROL_EVAL_COUNT, 2))
    result = grape_lindblad_discrete(
        2, CONTROL_EVAL_COUNT, [TargetDensityInfidelity(target)], EVOLUTION_TIME, initial,
        SYSTEM_EVAL_COUNT, hamiltonian=hamiltonian, lindblad_data=lindblad_data,
        initial_controls=start, iteration_count=iteration_count, log_iteration_step=20,
        max_control_norms=np.full(2, 0.1), optimizer=Adam(learning_rate=2e-3), wide=True)
    final = result.best_final_densities[0]
    print("best error {:.6e} at iteration {}; population of |g, 1> {:.6f}, trace {:.12f}".format(
        result.best_error, result.best_iteration, final[1, 1].real, np.trace(final).real))
    return result


if __name__ == "__main__":
    main()
