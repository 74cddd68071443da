"""
bench_control_costs.py - GPU-BOX TOOLING: multi-start GRAPE with pulse-shaping penalties
(ControlVariation + ControlBandwidthMax) on the device-resident route (qocx_set_control_costs,
qoc_amd/csrc/qocx_ctrlcost.hip) against the host loop of the same problem, and what the
control-cost kernels add to a resident evaluation.

Cases:
    headline          bench.py's shape with four real controls: n = 32, 1000 steps, 256 seeds
    lindblad_c4       BASELINE.json configs[3]: Lindblad, n = 16, 500 steps, 64 seeds, 2 operators
    headline_complex  the headline with 2 complex controls (the same 4 real channels)

Per case, one iteration of the multi-start loop (Adam) on both routes in ONE process, alternating
(resident, host loop) ALTERNATIONS times; each figure is the difference of a run of 2 I and a run of
I iterations over I, so the one-time setup drops out, and the median over the alternations is
reported with the minimum and maximum. The control-cost kernels alone are the difference of
resident evaluations (forward + gradient) with the costs set and cleared, alternating as well.
One JSON line per case.

    python tools/bench_control_costs.py > profiles/control_costs.jsonl
"""
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from qoc_amd import engine as engine_mod  # noqa: E402
from qoc_amd.core import batch as batch_mod  # noqa: E402
from qoc_amd.core import device, lindbladdiscrete, schroedingerdiscrete, structure  # noqa: E402
from qoc_amd.standard import (Adam, ControlBandwidthMax, ControlVariation,  # noqa: E402
                              TargetDensityInfidelity, TargetStateInfidelity)

ALTERNATIONS = 5
ITERATIONS = 4
EVALUATIONS = 30


class PluginAdam(Adam):  # not type(...) is Adam: takes the host loop
    pass


def shaping_costs(K, Nc, T):
    """Second differences and the upper four fifths of the positive spectrum of every control."""
    freqs = np.fft.fftfreq(Nc, d=T / (Nc - 1))
    return [ControlVariation(K, Nc, cost_multiplier=0.1, order=2),
            ControlBandwidthMax(K, Nc, T, np.full(K, freqs[Nc // 10]), cost_multiplier=0.1)]


def starts(seeds, Nc, K, cplx):
    rng = np.random.default_rng(1000)
    u = 0.1 * rng.standard_normal((seeds, Nc, K))
    return u + 0.1j * rng.standard_normal((seeds, Nc, K)) if cplx else u


def schroedinger_case(cplx):
    rng = np.random.default_rng(2003)
    n, Nc, kr = bench.DIM, bench.N_EVAL, 4
    h0 = bench.gue(rng, n)
    g = [bench.gue(rng, n) for _ in range(kr)]
    K = kr // 2 if cplx else kr

    def hamiltonian(u, t):
        out = h0
        for k in range(K):
            out = out + (u[k].real * g[2 * k] + u[k].imag * g[2 * k + 1] if cplx else u[k] * g[k])
        return out
    T = bench.DT * (Nc - 1)
    psi0 = np.eye(n, dtype=np.complex128)[:1].reshape(1, n, 1)
    target = np.eye(n, dtype=np.complex128)[1:2].reshape(1, n, 1)
    costs = [TargetStateInfidelity(target)] + shaping_costs(K, Nc, T)
    ev = device.SchroedingerEvaluator(T, hamiltonian, psi0, Nc, control_count=K,
                                      control_eval_count=Nc, complex_controls=cplx, costs=costs)
    return dict(evaluator=ev, K=K, Nc=Nc, T=T, cplx=cplx, seeds=bench.SEEDS_PER_GPU, n=n,
                ops=schroedingerdiscrete._ResidentOps, path=engine_mod.PATH_SCHROEDINGER,
                result=schroedingerdiscrete.GrapeSchroedingerBatchResult)


def lindblad_case():
    h0, g, gam, ops, rho0, target = bench.lindblad_problem()
    K, Nc = len(g), bench.LB_EVAL
    T = bench.DT * (Nc - 1)

    def hamiltonian(u, t):
        return h0 + sum(u[k] * g[k] for k in range(K))
    costs = [TargetDensityInfidelity(target)] + shaping_costs(K, Nc, T)
    ev = device.LindbladEvaluator(T, rho0, Nc, hamiltonian=hamiltonian,
                                  lindblad_data=lambda t: (gam, ops), control_count=K,
                                  control_eval_count=Nc, costs=costs, control_bounds=np.ones(K))
    return dict(evaluator=ev, K=K, Nc=Nc, T=T, cplx=False, seeds=bench.LB_SEEDS, n=bench.LB_DIM,
                ops=lindbladdiscrete._ResidentOps, path=engine_mod.PATH_LINDBLAD,
                result=lindbladdiscrete.GrapeLindbladBatchResult)


def per_iteration(run):
    """ms per iteration of run(count): (run(2 I) - run(I)) / I."""
    def timed(count):
        gc.collect()
        t0 = time.perf_counter()
        run(count)
        return time.perf_counter() - t0
    return (timed(2 * ITERATIONS) - timed(ITERATIONS)) / ITERATIONS * 1e3


def summary(samples):
    return dict(median=round(float(np.median(samples)), 3), min=round(float(np.min(samples)), 3),
                max=round(float(np.max(samples)), 3))


def measure(name, case):
    ev, K, Nc, cplx, seeds = case["evaluator"], case["K"], case["Nc"], case["cplx"], case["seeds"]
    assert ev.resident_capable()
    descriptors = ev.control_cost_descriptors
    comm, pstate, params = batch_mod.prepare_seeds(starts(seeds, Nc, K, cplx), cplx, K, Nc,
                                                   case["T"], np.ones(K), None, None)

    def resident(count):
        batch_mod.run_batch_resident(case["ops"](ev.backend, descriptors, cplx),
                                     Adam(learning_rate=1e-3), params.copy(), pstate, count, 0, 0,
                                     comm, case["result"](seeds))

    def host(count):
        batch_mod.run_batch_host(ev, None, PluginAdam(learning_rate=1e-3), params.copy(), pstate,
                                 count, 0, 0, comm, case["result"](seeds))
    resident(1)  # warm: code objects, buffers
    host(1)
    res_ms, host_ms = [], []
    for _ in range(ALTERNATIONS):
        res_ms.append(per_iteration(resident))
        host_ms.append(per_iteration(host))

    # the control-cost kernels alone: resident evaluations with the costs set / cleared
    backend = ev.backend
    lindblad = case["path"] == engine_mod.PATH_LINDBLAD
    upload = backend.lindblad_upload_controls if lindblad else backend.upload_controls
    evaluate = backend.eval_lindblad_resident if lindblad else backend.eval_resident
    real = structure.to_real_controls(starts(seeds, Nc, K, cplx), cplx)

    def evaluations(with_costs):
        backend.set_control_costs(case["path"], cplx, descriptors if with_costs else [])
        upload(real)
        evaluate(True)
        backend.synchronize()
        t0 = time.perf_counter()
        for _ in range(EVALUATIONS):
            evaluate(True)
        backend.synchronize()
        return (time.perf_counter() - t0) / EVALUATIONS * 1e3
    with_ms, without_ms = [], []
    for _ in range(ALTERNATIONS):
        with_ms.append(evaluations(True))
        without_ms.append(evaluations(False))
    backend.set_control_costs(case["path"], cplx, descriptors)
    t0 = time.perf_counter()
    for _ in range(EVALUATIONS):
        backend.eval_control_costs(case["path"], real)
    host_buffers_ms = (time.perf_counter() - t0) / EVALUATIONS * 1e3
    backend.set_control_costs(case["path"], cplx, [])
    bins = [len(b) for d in descriptors if d.get("bins") is not None for b in d["bins"]]
    print(json.dumps(dict(
        case=name, n=case["n"], steps=Nc - 1, seeds=seeds, controls=K, complex_controls=cplx,
        costs=["ControlVariation(order=2)", "ControlBandwidthMax"], penalised_bins=bins,
        alternations=ALTERNATIONS, iterations_per_sample=ITERATIONS,
        resident_ms_per_iteration=summary(res_ms), host_loop_ms_per_iteration=summary(host_ms),
        resident_evaluation_ms=summary(without_ms),
        resident_evaluation_with_control_costs_ms=summary(with_ms),
        control_cost_kernels_ms=round(float(np.median(with_ms) - np.median(without_ms)), 3),
        eval_control_costs_host_buffers_ms=round(host_buffers_ms, 3))), flush=True)
    backend.close()


def main():
    measure("headline", schroedinger_case(False))
    measure("lindblad_c4", lindblad_case())
    measure("headline_complex", schroedinger_case(True))


if __name__ == "__main__":
    main()
