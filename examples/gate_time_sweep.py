"""
gate_time_sweep.py - "what is the shortest duration at which this gate works?": GRAPE for the
|0> -> |1> transfer of an 8-level transmon at 32 durations in ONE multi-start run
(qoc_amd.standard.HamiltonianSweep.durations): seed b is the system run for T_b, with a pulse and an
optimizer state of its own. Prints the error against the duration, and d error / d T at the pulses
found - what a minimum-time search would follow.

    python examples/gate_time_sweep.py        # needs an MI355X and qoc_amd/libqocx.so
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from qoc_amd import grape_schroedinger_discrete_batch  # noqa: E402
from qoc_amd.standard import (Adam, HamiltonianSweep, TargetStateInfidelity,  # noqa: E402
                              get_annihilation_operator, get_creation_operator)

HILBERT_SIZE = 8
A = get_annihilation_operator(HILBERT_SIZE)
A_DAGGER = get_creation_operator(HILBERT_SIZE)
OMEGA, ALPHA = 2 * np.pi * 0.05, 2 * np.pi * (-0.2)
H_SYSTEM = OMEGA * A_DAGGER @ A + 0.5 * ALPHA * A_DAGGER @ A_DAGGER @ A @ A
DRIVES = (A + A_DAGGER, 1j * (A - A_DAGGER))


def hamiltonian(controls, time):
    return H_SYSTEM + controls[0] * DRIVES[0] + controls[1] * DRIVES[1]


INITIAL_STATES = np.eye(HILBERT_SIZE, dtype=np.complex128)[:, :1][None]
TARGET_STATES = np.eye(HILBERT_SIZE, dtype=np.complex128)[:, 1:2][None]
EVAL_COUNT = 501
REFERENCE_TIME = 25.0  # nanoseconds; seed b runs for DURATIONS[b]
DURATIONS = np.linspace(4.0, 35.0, 32)


def main(iteration_count=200):
    sweep = HamiltonianSweep.durations(hamiltonian, DURATIONS, REFERENCE_TIME)
    rng = np.random.default_rng(0)
    start = 0.05 * rng.standard_normal((len(DURATIONS), EVAL_COUNT, 2))
    result = grape_schroedinger_discrete_batch(
        2, EVAL_COUNT, [TargetStateInfidelity(TARGET_STATES)], REFERENCE_TIME, sweep,
        INITIAL_STATES, EVAL_COUNT, start, iteration_count=iteration_count, log_iteration_step=50,
        max_control_norms=np.full(2, 0.5), optimizer=Adam(learning_rate=1e-2))
    slopes = result.sweep_sensitivities["evolution_time_gradients"]
    print("duration (ns) |   best error   | d error / d T")
    for duration, error, slope in zip(DURATIONS, result.best_error, slopes):
        print("{:^13.2f} | {:^14.6e} | {:^+13.3e}".format(duration, error, slope))
    return result


if __name__ == "__main__":
    main()
