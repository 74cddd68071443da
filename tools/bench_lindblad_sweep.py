"""
bench_lindblad_sweep.py - GPU-BOX TOOLING: a 64-duration LindbladSweep (qocx_lindblad_set_sweep)
against the plain problem it expands to and against what a duration sweep under T1 / T2 cost
without the feature, the rate-sensitivity kernel's time, and the gate that runs without a sweep
cost what they cost on the parent commit.

The shape of BASELINE.json configs[3] as bench.py builds it (bench.lindblad_problem): n = 16, 501
system evaluation points, two real controls, two Lindblad operators, 64 seeds. The sweep runs seed b
for T_b = tau_b T, tau_b from 0.5 to 1.5: the drift H0 is the fixed channel D_0 (3 channels) and
seed b's rates are tau_b * gamma. Three runs per line (each the mean over REPS timed repetitions
after a warm one; (e) one repetition), ranges reported; (s) and (x) run in turns in one process.

    (s)  one resident Adam iteration of the sweep: qocx_lindblad_opt_clip, qocx_eval_lindblad_resident
         (expand, the evaluation of 64 items behind the member table, reduce), 64 costs to the
         host, qocx_lindblad_opt_step
    (x)  the same iteration of the plain 3-channel problem on the host-expanded controls with ONE
         rate set (tau = 1 for every seed: the plain kernels, no member table)
    (d)  the evaluation with rate sensitivities that follows an optimisation, and the download
    (e)  64 single-seed evaluations with a problem set-up each: the sweep without the feature
    (p)  a plain 64-seed Lindblad evaluation, no sweep              } fresh process per library: this
    (q)  a rate-ensemble evaluation (M = 3 members), no sweep       } build and - with
                                                                    } --parent-library PATH - the
                                                                    } parent commit's, alternating,
                                                                    } order swapped per visit

A run without a sweep launches what it launched before, so this build's median of (p) and (q) must
not lie above the parent's slowest run: the check lines, the rule of tools/bench_sweep.py.

    python tools/bench_lindblad_sweep.py [--parent-library PATH] > profiles/lindblad_sweep.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o lsweep -- python tools/bench_lindblad_sweep.py --trace-child
    python tools/bench_lindblad_sweep.py --trace-summary DIR/lsweep_results.db >> profiles/lindblad_sweep.jsonl
        (a run of its own: the per-launch times of the rate-sensitivity kernels, read from the
        trace's rocpd database)
"""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from qoc_amd import engine as engine_mod  # noqa: E402

DIM, N_EVAL, SEEDS, K_CTRL, DT = bench.LB_DIM, bench.LB_EVAL, bench.LB_SEEDS, bench.K_CTRL, bench.DT
T = DT * (N_EVAL - 1)
RUNS, REPS = 3, 10
NEW_SYMBOLS = ("qocx_lindblad_set_sweep", "qocx_lindblad_sweep_want_rate_sensitivities",
               "qocx_lindblad_sweep_download_sensitivities")
ADAM = dict(learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-8)


def controls(count=SEEDS):
    return np.stack([0.1 * np.random.default_rng(1000 + b).standard_normal((N_EVAL, K_CTRL))
                     for b in range(count)])


def taus():
    return np.linspace(0.5, 1.5, SEEDS)


def set_problem(engine, h0, g, gam, evolution_time=T):
    _, _, _, ops, rho0, target = bench.lindblad_problem()
    engine.set_lindblad_problem(
        DIM, 1, len(g), N_EVAL, N_EVAL, evolution_time, h0, list(g), gam, ops, rho0,
        costs=[dict(kind=engine_mod.COST_TARGET_DENSITY, step_cost=0, scale=1.0, vectors=target)])


def runs_of(call, reps=REPS):
    out = []
    for _ in range(RUNS):
        call()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        out.append((time.perf_counter() - t0) / reps * 1e3)
    return out


def alternating(first, second):
    a, b = [], []
    for _ in range(RUNS):
        for call, out in ((first, a), (second, b)):
            call()
            t0 = time.perf_counter()
            for _ in range(REPS):
                call()
            out.append((time.perf_counter() - t0) / REPS * 1e3)
    return a, b


def line(mode, what, runs, **more):
    rec = dict(mode=mode, what=what, n=DIM, steps=N_EVAL - 1, seeds=SEEDS, controls=K_CTRL,
               runs_ms=[round(r, 3) for r in runs], ms_min=round(min(runs), 3),
               ms_max=round(max(runs), 3), ms_median=round(float(np.median(runs)), 3), **more)
    print(json.dumps(rec), flush=True)
    return rec


def resident_iteration(engine, channels):
    step = [0]
    on = np.ones(SEEDS, dtype=bool)

    def call():
        step[0] += 1
        engine.lindblad_opt_clip(np.full(channels, 10.0))
        engine.eval_lindblad_resident(True)
        engine.lindblad_download_costs()
        engine.lindblad_opt_step(1, on, on, ADAM["learning_rate"], ADAM["beta_1"], ADAM["beta_2"],
                                 ADAM["epsilon"], 1 - ADAM["beta_1"] ** step[0],
                                 1 - ADAM["beta_2"] ** step[0])
    return call


def sweep_engine():
    h0, g, gam, _, _, _ = bench.lindblad_problem()
    tau = taus()
    engine = engine_mod.Engine(0)
    set_problem(engine, np.zeros_like(h0), list(g) + [h0], gam)
    engine.set_lindblad_sweep(np.repeat(tau[:, None], K_CTRL, axis=1), tau[:, None],
                              np.repeat(tau[:, None], len(gam), axis=1))
    return engine


def gate_child(library):
    """Modes (p) and (q) in this process, on the library at `library`: nothing here sets a sweep."""
    try:
        engine_mod.load_library(library)
    except AttributeError:  # the parent commit's library: no sweep symbols to bind
        for name in NEW_SYMBOLS:
            engine_mod.SIGNATURES.pop(name, None)
        engine_mod.load_library(library)
    h0, g, gam, _, _, _ = bench.lindblad_problem()
    u = controls()
    engine = engine_mod.Engine(0)
    set_problem(engine, h0, g, gam)
    plain = runs_of(lambda: engine.evaluate_lindblad(u), reps=5)
    members = 3
    engine.set_lindblad_ensemble(np.array([[1.0, 1.0], [0.98, 1.02], [1.03, 0.97]]), None,
                                 np.full(members, 1.0 / members))
    engine.set_lindblad_ensemble_rates(np.array([[1.0, 1.0], [0.5, 2.0], [2.0, 0.5]]))
    third = u[:SEEDS // members + 1]
    rates = runs_of(lambda: engine.evaluate_lindblad(third), reps=5)
    engine.close()
    print(json.dumps(dict(plain=plain, rates=rates)), flush=True)


def gate(parent_library):
    """This build and the parent's library in fresh processes, alternating, two visits each; the
    second visit in the opposite order, so that neither library is always the one that runs second."""
    results = {}
    libraries = [("this build", engine_mod.LIBRARY_PATH)]
    if parent_library:
        libraries.insert(0, ("parent commit", os.path.abspath(parent_library)))
    for visit in range(2):
        for label, path in (libraries if visit == 0 else libraries[::-1]):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--gate-library", path],
                                 check=True, capture_output=True, text=True, timeout=300).stdout
            got = json.loads(out.strip().splitlines()[-1])
            for key in ("plain", "rates"):
                results.setdefault((key, label), []).extend(got[key])
    names = dict(plain=("p", "plain 64-seed Lindblad evaluation, no sweep"),
                 rates=("q", "rate-ensemble evaluation (22 seeds x 3 members), no sweep"))
    for (key, label), runs in results.items():
        line(names[key][0], "{}, {} (fresh processes)".format(names[key][1], label), runs)
    if parent_library:
        for key in ("plain", "rates"):
            parent, this = results[(key, "parent commit")], results[(key, "this build")]
            print(json.dumps(dict(
                check="{}: this build's median against the parent's slowest run".format(names[key][1]),
                this_median_ms=round(float(np.median(this)), 3), parent_max_ms=round(max(parent), 3),
                parent_median_ms=round(float(np.median(parent)), 3),
                passed=bool(np.median(this) <= max(parent)))), flush=True)
    return results


def trace_child():
    """Five evaluations with rate sensitivities, for a kernel trace."""
    engine = sweep_engine()
    u = controls()
    engine.lindblad_sweep_want_rate_sensitivities(True)
    for _ in range(5):
        engine.evaluate_lindblad(u)
        engine.lindblad_sweep_sensitivities()
    engine.close()


def trace_summary(database):
    """One line with the per-launch times (us) of the rate-sensitivity kernels, and of the combine
    kernel beside which they run, in a rocprofv3 kernel trace of trace_child(), read from its rocpd
    (SQLite) database."""
    import sqlite3
    rows = sqlite3.connect(database).execute('select name, "end" - start from kernels').fetchall()
    out = {}
    for kernel in ("lindblad_ratesens_kernel", "lindblad_ratesens_reduce_kernel",
                   "lindblad_combine_kernel"):
        times = [duration / 1e3 for name, duration in rows
                 if kernel in name and (kernel != "lindblad_ratesens_kernel" or "reduce" not in name)]
        out[kernel] = dict(launches=len(times), us_min=round(min(times), 2),
                           us_median=round(float(np.median(times)), 2), us_max=round(max(times), 2))
    print(json.dumps(dict(mode="t", what="per-launch times of the rate-sensitivity kernels "
                                         "(rocprofv3 --kernel-trace, a run of its own)", n=DIM,
                          steps=N_EVAL - 1, seeds=SEEDS, controls=K_CTRL, dispatches=len(rows),
                          **out)), flush=True)


def main(parent_library):
    gate(parent_library)  # (before this process opens the device)
    h0, g, gam, _, _, _ = bench.lindblad_problem()
    tau, u = taus(), controls()
    # (s) and (x) in turns, each on an engine of its own
    sweep = sweep_engine()
    sweep.lindblad_upload_controls(u)
    sweep.lindblad_opt_begin()
    engine = engine_mod.Engine(0)
    set_problem(engine, np.zeros_like(h0), list(g) + [h0], gam)
    wide = np.concatenate([tau[:, None, None] * u,
                           np.broadcast_to(tau[:, None, None], (SEEDS, N_EVAL, 1))], axis=2)
    engine.lindblad_upload_controls(wide)
    engine.lindblad_opt_begin()
    s_runs, x_runs = alternating(resident_iteration(sweep, K_CTRL),
                                 resident_iteration(engine, K_CTRL + 1))
    s = line("s", "resident Adam iteration of the 64-duration Lindblad sweep (3 channels, rates per "
                  "seed), in turns with (x)", s_runs)
    x = line("x", "resident Adam iteration of the plain 3-channel problem, host-expanded controls, one "
                  "rate set, in turns with (s)", x_runs)
    print(json.dumps(dict(check="sweep iteration against the plain 3-channel iteration (reported, "
                                "not asserted)", plain_ms=[x["ms_min"], x["ms_max"]],
                          sweep_ms=[s["ms_min"], s["ms_max"]],
                          ratio_of_medians=round(s["ms_median"] / x["ms_median"], 4))), flush=True)
    engine.close()

    def with_sensitivities():
        sweep.lindblad_sweep_want_rate_sensitivities(True)
        sweep.evaluate_lindblad(u)
        out = sweep.lindblad_sweep_sensitivities()
        sweep.lindblad_sweep_want_rate_sensitivities(False)
        assert out[2] is not None
    d = line("d", "evaluation with rate sensitivities and the download of the three tables",
             runs_of(with_sensitivities, reps=5))
    line("g", "the same evaluation without rate sensitivities ((d) minus this: the kernel's share)",
         runs_of(lambda: sweep.evaluate_lindblad(u), reps=5), with_rates_ms_median=d["ms_median"])
    sweep.close()
    gc.collect()

    single = engine_mod.Engine(0)

    def one_by_one():
        for b in range(SEEDS):
            set_problem(single, h0, g, gam, evolution_time=tau[b] * T)
            single.evaluate_lindblad(u[b:b + 1])
    line("e", "64 single-seed evaluations with a problem set-up each (the duration sweep without the "
              "feature)", runs_of(one_by_one, reps=1))
    single.close()


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--parent-library")
    parser.add_argument("--gate-library")
    parser.add_argument("--trace-child", action="store_true")
    parser.add_argument("--trace-summary")
    args = parser.parse_args()
    if args.gate_library:
        gate_child(args.gate_library)
    elif args.trace_child:
        trace_child()
    elif args.trace_summary:
        trace_summary(args.trace_summary)
    else:
        main(args.parent_library)
