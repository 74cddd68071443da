"""
gate_time_sweep_t1.py - "which gate time is best under T1?": GRAPE for the |0> -> |1> transfer of a
4-level transmon that decays with T1 and dephases with T_phi, at 24 durations in ONE multi-start run
(qoc_amd.standard.LindbladSweep.durations): seed b is the open system run for T_b - Hamiltonian AND
dissipation rates scaled by T_b / reference_time - with a pulse and an optimizer state of its own.
A short gate leaks and cannot finish the rotation within the amplitude bound, a long one decays:
the error has a minimum in T. Prints the error against the duration and d error / d T at the
pulses found (the sign change is the minimum), and d error / d rate factor for the two channels -
which decay channel costs how much.

    python examples/gate_time_sweep_t1.py        # needs an MI355X and qoc_amd/libqocx.so
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from qoc_amd import grape_lindblad_discrete_batch  # noqa: E402
from qoc_amd.standard import (Adam, LindbladSweep, TargetDensityInfidelity,  # noqa: E402
                              get_annihilation_operator, get_creation_operator)

HILBERT_SIZE = 4
A = get_annihilation_operator(HILBERT_SIZE)
A_DAGGER = get_creation_operator(HILBERT_SIZE)
ALPHA = 2 * np.pi * (-0.2)  # GHz; the rotating frame of the qubit
H_SYSTEM = 0.5 * ALPHA * A_DAGGER @ A_DAGGER @ A @ A
DRIVES = (A + A_DAGGER, 1j * (A - A_DAGGER))
T1, T_PHI = 2000.0, 4000.0  # nanoseconds (short, so that the minimum shows within 24 seeds)
DISSIPATORS = np.array([1.0 / T1, 2.0 / T_PHI])
OPERATORS = np.stack([A, A_DAGGER @ A])


def hamiltonian(controls, time):
    return H_SYSTEM + controls[0] * DRIVES[0] + controls[1] * DRIVES[1]


def lindblad_data(time):
    return DISSIPATORS, OPERATORS


INITIAL = np.zeros((1, HILBERT_SIZE, HILBERT_SIZE), dtype=np.complex128)
INITIAL[0, 0, 0] = 1
TARGET = np.zeros((1, HILBERT_SIZE, HILBERT_SIZE), dtype=np.complex128)
TARGET[0, 1, 1] = 1
SYSTEM_EVAL_COUNT, CONTROL_EVAL_COUNT = 101, 21
REFERENCE_TIME = 20.0  # nanoseconds; seed b runs for DURATIONS[b]
DURATIONS = np.linspace(6.0, 98.0, 24)


def main(iteration_count=150):
    sweep = LindbladSweep.durations(hamiltonian, DURATIONS, REFERENCE_TIME)
    rng = np.random.default_rng(0)
    start = np.clip(0.02 * rng.standard_normal((len(DURATIONS), CONTROL_EVAL_COUNT, 2)), -0.06, 0.06)
    result = grape_lindblad_discrete_batch(
        2, CONTROL_EVAL_COUNT, [TargetDensityInfidelity(TARGET)], REFERENCE_TIME, INITIAL,
        SYSTEM_EVAL_COUNT, start, hamiltonian=sweep, lindblad_data=lindblad_data,
        iteration_count=iteration_count, log_iteration_step=50,
        max_control_norms=np.full(2, 0.06), optimizer=Adam(learning_rate=2e-3))
    sens = result.sweep_sensitivities
    slopes, rates = sens["evolution_time_gradients"], sens["rate_scales"]
    print("duration (ns) |   best error   | d error / d T | d error / d c (T1) | d error / d c (T_phi)")
    for b, duration in enumerate(DURATIONS):
        print("{:^13.2f} | {:^14.6e} | {:^+13.3e} | {:^+18.3e} | {:^+21.3e}".format(
            duration, result.best_error[b], slopes[b], rates[b, 0], rates[b, 1]))
    best = int(np.argmin(result.best_error))
    print("the smallest error, {:.3e}, is at T = {:.1f} ns".format(result.best_error[best],
                                                                   DURATIONS[best]))
    return result


if __name__ == "__main__":
    main()
