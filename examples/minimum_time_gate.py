"""
minimum_time_gate.py - minimum-time GRAPE: the transmon of examples/gate_time_sweep.py, but the
duration of every start is optimised together with its pulse
(qoc_amd.standard.HamiltonianSweep.durations with time_bounds). 32 starts between 4 and 35 ns, each
with a pulse, a duration and an optimizer state of its own; a small price on time (time_weight) pulls
every start towards the shortest duration at which the |0> -> |1> transfer still works. Prints T_b
before and after.

    python examples/minimum_time_gate.py        # needs an MI355X and qoc_amd/libqocx.so
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from examples.gate_time_sweep import (DURATIONS, EVAL_COUNT, INITIAL_STATES,  # noqa: E402
                                      REFERENCE_TIME, TARGET_STATES, hamiltonian)
from qoc_amd import grape_schroedinger_discrete_batch  # noqa: E402
from qoc_amd.standard import Adam, HamiltonianSweep, TargetStateInfidelity  # noqa: E402

TIME_BOUNDS = (2.0, 40.0)   # nanoseconds
TIME_WEIGHT = 0.02          # error per reference time: 0.02 * T_b / 25 ns is added to seed b's error


def main(iteration_count=200):
    sweep = HamiltonianSweep.durations(hamiltonian, DURATIONS, REFERENCE_TIME,
                                       time_bounds=TIME_BOUNDS, time_weight=TIME_WEIGHT)
    rng = np.random.default_rng(0)
    start = 0.05 * rng.standard_normal((len(DURATIONS), EVAL_COUNT, 2))
    result = grape_schroedinger_discrete_batch(
        2, EVAL_COUNT, [TargetStateInfidelity(TARGET_STATES)], REFERENCE_TIME, sweep,
        INITIAL_STATES, EVAL_COUNT, start, iteration_count=iteration_count, log_iteration_step=50,
        max_control_norms=np.full(2, 0.5), optimizer=Adam(learning_rate=1e-2))
    price = TIME_WEIGHT * result.best_evolution_times / REFERENCE_TIME
    print("start T (ns) | found T (ns) |  infidelity   | price of time")
    for begin, found, error, cost in zip(DURATIONS, result.best_evolution_times, result.best_error,
                                         price):
        print("{:^12.2f} | {:^12.2f} | {:^13.6e} | {:^13.3e}".format(begin, found, error - cost,
                                                                     cost))
    return result


if __name__ == "__main__":
    main()
