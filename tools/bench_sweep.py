"""
bench_sweep.py - GPU-BOX TOOLING: a 256-duration HamiltonianSweep (qocx_set_sweep) against the plain
problem it expands to and against what a duration sweep costs without the feature, and the gate
that runs without a sweep cost what they cost on the parent commit.

The headline shape with four real controls: n = 32, 1001 system evaluations (1000 steps), 256 seeds,
control knots at the system times. The sweep runs seed b for T_b = tau_b T, tau_b from 0.5 to 1.5:
the drift H0 is the fixed channel D_0, so the expanded problem has 5 channels. Three runs per line
(each the mean over 20 timed repetitions after a warm one; (e) one repetition), ranges reported;
(s) and (x) run in turns in one process.

    (s)  one resident Adam iteration of the sweep: qocx_opt_clip, qocx_eval_resident (expand, the
         evaluation of 256 items, reduce), 256 costs to the host, qocx_opt_step
    (x)  the same iteration of the plain 5-channel problem on the host-expanded controls: (s) should
         cost this plus its expand and reduce launches
    (d)  qocx_sweep_download_sensitivities after an evaluation (the third kernel and two copies)
    (e)  256 single-seed evaluations with a problem set-up each: a duration sweep without the feature
    (p)  a plain 256-seed evaluation of the 4-channel problem       } fresh process per library: this
    (r)  one resident Adam iteration of it, no sweep                } build and - with --parent-library
                                                                    } PATH - the parent commit's,
                                                                    } alternating, order swapped per visit

A run without a sweep launches what it launched before (the sweep's kernels are a code object of
their own behind a setter of their own), so this build's median of (p) and (r) must not lie above the
parent's slowest run: the check lines, the rule of tools/bench_lindblad_rate_ensemble.py.

    python tools/bench_sweep.py [--parent-library PATH] > profiles/sweep.jsonl
    python tools/bench_sweep.py --parent-library PATH --gate-only 5 > profiles/sweep_gate.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o sweep -- python tools/bench_sweep.py --trace-child
    python tools/bench_sweep.py --trace-summary DIR/sweep_results.db >> profiles/sweep.jsonl
        (a run of its own: the per-launch times of sweep_expand / _reduce / _sensitivity_kernel,
        read from the trace's rocpd database)
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
from qoc_amd import engine as engine_mod  # noqa: E402

DIM, N_EVAL, SEEDS, K_CTRL, DT = 32, 1001, 256, 4, 0.05
RUNS, REPS = 3, 20
NEW_SYMBOLS = ("qocx_set_sweep", "qocx_sweep_download_sensitivities")
ADAM = dict(learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-8)


def gue(rng, n):
    g = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    h = (g + g.conj().T) / 2
    return h / np.linalg.norm(h, 2)


def problem():
    rng = np.random.default_rng(2003)
    h0 = gue(rng, DIM)
    g = np.stack([gue(rng, DIM) for _ in range(K_CTRL)])
    psi0 = np.eye(DIM, dtype=np.complex128)[:1]
    target = np.eye(DIM, dtype=np.complex128)[1:2]
    return h0, g, psi0, target


def controls(count=SEEDS):
    return np.stack([0.1 * np.random.default_rng(1000 + b).standard_normal((N_EVAL, K_CTRL))
                     for b in range(count)])


def taus():
    return np.linspace(0.5, 1.5, SEEDS)


def set_problem(engine, h0, g, evolution_time=DT * (N_EVAL - 1)):
    _, _, psi0, target = problem()
    g = np.asarray(g)
    engine.set_schroedinger_problem(
        DIM, 1, g.shape[0], N_EVAL, N_EVAL, evolution_time, h0[None], g[None], psi0,
        costs=[dict(kind=engine_mod.COST_TARGET_COHERENT, step_cost=0, scale=1.0, vectors=target)])


def runs_of(call, reps=REPS):
    """ms per call, RUNS times, each the mean over `reps` calls after one warm call."""
    call()
    out = []
    for _ in range(RUNS):
        gc.collect()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        out.append(round((time.perf_counter() - t0) / reps * 1e3, 3))
    return out


def alternating(first, second, reps=REPS):
    """runs_of for two calls in turns (first, second, first, ...): neither is always the one that
    runs later in the session."""
    first()
    second()
    out = ([], [])
    for _ in range(RUNS):
        for runs, call in zip(out, (first, second)):
            gc.collect()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            runs.append(round((time.perf_counter() - t0) / reps * 1e3, 3))
    return out


def line(mode, what, runs, **more):
    row = dict(mode=mode, what=what, n=DIM, steps=N_EVAL - 1, seeds=SEEDS, controls=K_CTRL,
               runs_ms=runs, ms_min=min(runs), ms_max=max(runs), **more)
    print(json.dumps(row), flush=True)
    return row


def resident_iteration(engine, channels):
    """One iteration of the resident Adam loop on the uploaded seeds (core/batch.py's calls)."""
    flags = np.ones(SEEDS, dtype=np.uint8)
    norms = np.full(channels, 1.0)
    step = [0]

    def iteration():
        engine.opt_clip(norms)
        engine.eval_resident(True)
        engine.download_costs()
        step[0] += 1
        engine.opt_step(1, flags, flags, ADAM["learning_rate"], ADAM["beta_1"], ADAM["beta_2"],
                        ADAM["epsilon"], 1 - ADAM["beta_1"] ** step[0], 1 - ADAM["beta_2"] ** step[0])
    return iteration


def gate_child(library):
    """Modes (p) and (r) in this process, on the library at `library`: nothing here sets a sweep."""
    try:
        engine_mod.load_library(library)
    except AttributeError:  # the parent commit's library: no sweep symbols to bind
        for name in NEW_SYMBOLS:
            engine_mod.SIGNATURES.pop(name, None)
        engine_mod.load_library(library)
    h0, g, _, _ = problem()
    u = controls()
    engine = engine_mod.Engine(0)
    set_problem(engine, h0, g)
    plain = runs_of(lambda: engine.evaluate(u))
    engine.upload_controls(u)
    engine.opt_begin()
    iteration = runs_of(resident_iteration(engine, K_CTRL))
    engine.close()
    print(json.dumps(dict(library=library, plain=plain, iteration=iteration)), flush=True)


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
            for key in ("plain", "iteration"):
                results.setdefault((key, label), []).extend(got[key])
    names = dict(plain=("p", "plain 256-seed evaluation, no sweep"),
                 iteration=("r", "resident Adam iteration, no sweep"))
    for (key, label), runs in results.items():
        line(names[key][0], "{}, {} (fresh processes)".format(names[key][1], label), runs)
    if parent_library:
        for key in ("plain", "iteration"):
            parent, this = results[(key, "parent commit")], results[(key, "this build")]
            print(json.dumps(dict(
                check="{}: this build against the parent commit's library".format(names[key][1]),
                parent_ms=[min(parent), max(parent)], this_ms=[min(this), max(this)],
                parent_median_ms=float(np.median(parent)), this_median_ms=float(np.median(this)),
                visit_order=["parent, this", "this, parent"],
                within_parent_scatter=bool(np.median(this) <= max(parent)))), flush=True)
    return results


def gates(parent_library, count):
    """The gate alone, `count` times over, and the runs of all of them pooled per library: a single
    gate has six runs per library."""
    pooled = {}
    for _ in range(count):
        for key, runs in gate(parent_library).items():
            pooled.setdefault(key, []).extend(runs)
    for (what, label), runs in sorted(pooled.items()):
        print(json.dumps(dict(pooled=what, library=label, runs=len(runs),
                              median_ms=float(np.median(runs)), ms_min=min(runs), ms_max=max(runs))),
              flush=True)


def sweep_engine():
    """(engine with the 256-duration sweep set, its seed controls)."""
    h0, g, _, _ = problem()
    engine = engine_mod.Engine(0)
    set_problem(engine, np.zeros_like(h0), np.concatenate([g, h0[None]]))
    tau = taus()
    engine.set_sweep(np.repeat(tau[:, None], K_CTRL, axis=1), tau[:, None])
    return engine, controls()


def trace_child():
    """A few sweep iterations and a sensitivity download, for a kernel trace."""
    engine, u = sweep_engine()
    engine.upload_controls(u)
    engine.opt_begin()
    iteration = resident_iteration(engine, K_CTRL)
    for _ in range(5):
        iteration()
    engine.opt_clip(np.full(K_CTRL, 1.0))
    engine.eval_resident(True)
    engine.sweep_sensitivities()
    engine.close()


def trace_summary(database):
    """One line with the per-launch times (us) of the three sweep kernels in a rocprofv3 kernel
    trace of trace_child(), read from its rocpd (SQLite) database."""
    import sqlite3
    rows = sqlite3.connect(database).execute('select name, "end" - start from kernels').fetchall()
    out = {}
    for kernel in ("sweep_expand_kernel", "sweep_reduce_kernel", "sweep_sensitivity_kernel"):
        times = [duration / 1e3 for name, duration in rows if kernel in name]
        out[kernel] = dict(launches=len(times), us_min=round(min(times), 2),
                           us_median=round(float(np.median(times)), 2), us_max=round(max(times), 2))
    print(json.dumps(dict(mode="t", what="per-launch times of the sweep's kernels (rocprofv3 "
                                         "--kernel-trace, a run of its own)", n=DIM,
                          steps=N_EVAL - 1, seeds=SEEDS, controls=K_CTRL, dispatches=len(rows),
                          **out)), flush=True)


def main(parent_library):
    gate(parent_library)  # (before this process opens the device)
    h0, g, _, _ = problem()
    tau, u = taus(), controls()
    # (s) and (x) in turns, each on an engine of its own: the sweep, and the plain 5-channel problem
    # on the host-expanded controls
    sweep, _ = sweep_engine()
    sweep.upload_controls(u)
    sweep.opt_begin()
    engine = engine_mod.Engine(0)
    set_problem(engine, np.zeros_like(h0), np.concatenate([g, h0[None]]))
    wide = np.concatenate([tau[:, None, None] * u,
                           np.broadcast_to(tau[:, None, None], (SEEDS, N_EVAL, 1))], axis=2)
    engine.upload_controls(wide)
    engine.opt_begin()
    s_runs, x_runs = alternating(resident_iteration(sweep, K_CTRL),
                                 resident_iteration(engine, K_CTRL + 1))
    s = line("s", "resident Adam iteration of the 256-duration sweep (5 channels), in turns with (x)",
             s_runs)
    x = line("x", "resident Adam iteration of the plain 5-channel problem, host-expanded controls "
                  "(its optimizer moves 5 channels, the sweep's 4), in turns with (s)", x_runs)
    print(json.dumps(dict(check="sweep iteration against the plain 5-channel iteration (reported, "
                                "not asserted)", plain_ms=[x["ms_min"], x["ms_max"]],
                          sweep_ms=[s["ms_min"], s["ms_max"]],
                          plain_median_ms=float(np.median(x_runs)),
                          sweep_median_ms=float(np.median(s_runs)))), flush=True)
    # (d): the sensitivities of an evaluation of the start controls
    sweep.upload_controls(u)
    sweep.eval_resident(True)
    sweep_cost = sweep.download_costs()
    line("d", "qocx_sweep_download_sensitivities after an evaluation",
         runs_of(sweep.sweep_sensitivities))
    sweep.close()
    # (e): one problem set-up and one single-seed evaluation per duration
    T = DT * (N_EVAL - 1)
    costs = np.empty(SEEDS)

    def one_by_one():
        for b in range(SEEDS):
            set_problem(engine, h0, g, evolution_time=tau[b] * T)
            costs[b] = engine.evaluate(u[b:b + 1])[0][0]
    line("e", "256 single-seed evaluations with a problem set-up each", runs_of(one_by_one, reps=1))
    print(json.dumps(dict(check="sweep costs against the 256 separate problems at evolution_time T_b",
                          max_abs_diff=float(np.max(np.abs(costs - sweep_cost))))), flush=True)
    engine.close()


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--parent-library", default=None,
                        help="libqocx.so built from the parent commit: the gate times it too")
    parser.add_argument("--gate-only", type=int, default=0, metavar="COUNT",
                        help="the gate alone, COUNT times, with the runs pooled per library")
    parser.add_argument("--gate-library", default=None, help=argparse.SUPPRESS)
    parser.add_argument("--trace-child", action="store_true",
                        help="a few sweep iterations and a sensitivity download, for a kernel trace")
    parser.add_argument("--trace-summary", default=None, metavar="DATABASE",
                        help="the sweep kernels' per-launch times from a kernel trace of --trace-child")
    args = parser.parse_args()
    if args.trace_summary:
        trace_summary(args.trace_summary)
    elif args.gate_library:
        gate_child(args.gate_library)
    elif args.gate_only:
        gates(args.parent_library, args.gate_only)
    elif args.trace_child:
        trace_child()
    else:
        main(args.parent_library)
