"""
minimum_time_gate_t1.py - "how long should the gate be under T1?", answered by a search instead of a
scan: the 4-level transmon of examples/gate_time_sweep_t1.py (|0> -> |1>, T1 decay and T_phi
dephasing), with the DURATION of every seed optimised together with its pulse
(qoc_amd.standard.LindbladSweep.duration_search). Seed b is tau_b times the whole Lindbladian, and
tau_b = T_b / reference_time is one more parameter of the seed on the device, stepped by Adam with
the controls. No price is put on time (time_weight = 0): a closed system would then drift to ever
longer gates, but here dissipation makes long gates worse, so the error has a minimum of its own and
the search finds it from several starting durations. Prints where each start ended, next to the
minimum of the fixed-duration scan of gate_time_sweep_t1.py.

    python examples/minimum_time_gate_t1.py        # needs an MI355X and qoc_amd/libqocx.so
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a checkout
from examples import gate_time_sweep_t1 as scan  # noqa: E402
from qoc_amd import grape_lindblad_discrete_batch  # noqa: E402
from qoc_amd.standard import Adam, LindbladSweep, TargetDensityInfidelity  # noqa: E402

STARTS = np.array([10.0, 20.0, 35.0, 50.0, 70.0, 90.0])  # nanoseconds
TIME_BOUNDS = (6.0, 98.0)                                  # the range the scan covers
# tau_b = T_b / reference_time is stepped with the controls' learning rate, so the reference time - a
# unit, nothing more: seed b is tau_b times the Lindbladian on [0, reference_time] - sets the length
# of Adam's step in time: 2e-3 * 400 ns = 0.8 ns per iteration
REFERENCE_TIME = 400.0


def main(iteration_count=1000, scan_iterations=150):
    sweep = LindbladSweep.duration_search(scan.hamiltonian, STARTS, REFERENCE_TIME, TIME_BOUNDS,
                                          time_weight=0.0)
    rng = np.random.default_rng(0)
    start = np.clip(0.02 * rng.standard_normal((len(STARTS), scan.CONTROL_EVAL_COUNT, 2)), -0.06, 0.06)
    result = grape_lindblad_discrete_batch(
        2, scan.CONTROL_EVAL_COUNT, [TargetDensityInfidelity(scan.TARGET)], REFERENCE_TIME,
        scan.INITIAL, scan.SYSTEM_EVAL_COUNT, start, hamiltonian=sweep,
        lindblad_data=scan.lindblad_data, iteration_count=iteration_count, log_iteration_step=200,
        max_control_norms=np.full(2, 0.06), optimizer=Adam(learning_rate=2e-3))
    slopes = result.sweep_sensitivities["evolution_time_gradients"]
    print("start (ns) | found (ns) |   best error   | d error / d T there")
    for b, begin in enumerate(STARTS):
        print("{:^10.1f} | {:^10.2f} | {:^14.6e} | {:^+19.3e}".format(
            begin, result.best_evolution_times[b], result.best_error[b], slopes[b]))
    fixed = scan.main(scan_iterations)
    best = int(np.argmin(fixed.best_error))
    print("the fixed-duration scan has its smallest error, {:.3e}, at T = {:.1f} ns; the searches "
          "ended at {} ns".format(fixed.best_error[best], scan.DURATIONS[best],
                                  np.round(result.best_evolution_times, 1)))
    return result, fixed


if __name__ == "__main__":
    main()
