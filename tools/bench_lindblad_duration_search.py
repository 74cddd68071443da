"""
bench_lindblad_duration_search.py - GPU-BOX TOOLING: what the duration search of a Lindblad sweep costs
per resident iteration (qocx_lindblad_sweep_set_durations, qocx_lindblad_duration.hip), what the same
search costs as a user's loop over the fixed-duration sweep, and the gate that runs without a search
cost what they cost on the parent commit.

The shape of BASELINE.json configs[3] as bench.py builds it (tools/bench_lindblad_sweep.py): n = 16, 501
system evaluation points, two real controls, two Lindblad operators, 64 seeds, tau_b from 0.5 to 1.5.
Three runs per line (each the mean over REPS timed repetitions after a warm one), lines of one group
timed in turns in one process.

    (s)  one resident Adam iteration of the search: qocx_lindblad_opt_clip (tau clipped, the tables and
         the seeds' generators rewritten, tau to the host with the control maxima),
         qocx_eval_lindblad_resident with rate sensitivities and the chain rule, 64 costs to the host,
         qocx_lindblad_opt_step
    (r)  the same iteration of the fixed-duration sweep with rate sensitivities asked for
    (f)  the same iteration of the fixed-duration sweep without them
    (u)  one iteration of the search as a user's loop over the fixed sweep: the problem set-up,
         qocx_lindblad_set_sweep at the current tau, an upload, an evaluation with rate sensitivities,
         gradients and the three tables to the host
    (p)  a plain 64-seed Lindblad evaluation, no sweep                  } fresh process per library:
    (w)  a resident iteration of the fixed-duration LindbladSweep        } this build and - with
    (h)  a resident iteration of the Schroedinger duration search        } --parent-library PATH - the
         (tools/bench_duration_search.py's)                              } parent commit's, alternating,
                                                                         } order swapped per visit

A run without a Lindblad search launches what it launched before, so this build's median of (p), (w)
and (h) must not lie above the parent's slowest run: the check lines.

    python tools/bench_lindblad_duration_search.py [--parent-library PATH] \\
        > profiles/lindblad_duration_search.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o lsearch -- \\
        python tools/bench_lindblad_duration_search.py --trace-child
    python tools/bench_lindblad_duration_search.py --trace-summary DIR/lsearch_results.db \\
        >> profiles/lindblad_duration_search.jsonl
        (a run of its own: the per-launch times of the two new kernels and of the kernels they run
        beside, read from the trace's rocpd database)
    python tools/bench_lindblad_duration_search.py --gate-only --parent-library PATH \
        >> profiles/lindblad_duration_search_gate.jsonl
        (the gate alone, for more visits than the two of a full run)
"""
import argparse
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
from tools import bench_duration_search as schroedinger  # noqa: E402
from tools.bench_lindblad_sweep import (K_CTRL, N_EVAL, RUNS, REPS, SEEDS, controls, line,  # noqa: E402
                                        resident_iteration, runs_of, set_problem, sweep_engine, taus)

NEW_SYMBOLS = ("qocx_lindblad_sweep_set_durations", "qocx_lindblad_sweep_download_durations",
               "qocx_lindblad_opt_download_best_durations")
TAU_BOX = (0.4, 1.6)


def search_engine(time_weight=0.0):
    """The 64-duration sweep of tools/bench_lindblad_sweep.py as a search."""
    engine = sweep_engine()
    engine.lindblad_sweep_set_durations(taus(), None, np.ones((SEEDS, 1)), None, *TAU_BOX, time_weight)
    return engine


def in_turns(calls):
    out = [[] for _ in calls]
    for _ in range(RUNS):
        for call, runs in zip(calls, out):
            call()
            t0 = time.perf_counter()
            for _ in range(REPS):
                call()
            runs.append((time.perf_counter() - t0) / REPS * 1e3)
    return out


def gate_child(library):
    """Modes (p), (w) and (h) in this process, on the library at `library`: nothing here sets the
    durations of a Lindblad sweep."""
    try:
        engine_mod.load_library(library)
    except AttributeError:  # the parent commit's library: no symbols of the Lindblad search to bind
        for name in NEW_SYMBOLS:
            engine_mod.SIGNATURES.pop(name, None)
        engine_mod.load_library(library)
    h0, g, gam, _, _, _ = bench.lindblad_problem()
    u = controls()
    engine = engine_mod.Engine(0)
    set_problem(engine, h0, g, gam)
    plain = runs_of(lambda: engine.evaluate_lindblad(u), reps=5)
    engine.close()
    sweep = sweep_engine()
    sweep.lindblad_upload_controls(u)
    sweep.lindblad_opt_begin()
    fixed = runs_of(resident_iteration(sweep, K_CTRL), reps=5)
    sweep.close()
    search, us = schroedinger.search_engine(0.01)
    search.upload_controls(us)
    search.opt_begin()
    closed = runs_of(schroedinger.resident_iteration(search, schroedinger.K_CTRL), reps=5)
    search.close()
    print(json.dumps(dict(plain=plain, fixed=fixed, closed=closed)), flush=True)


NAMES = dict(plain=("p", "plain 64-seed Lindblad evaluation, no sweep"),
             fixed=("w", "resident Adam iteration of the fixed-duration LindbladSweep, no search"),
             closed=("h", "resident Adam iteration of the Schroedinger duration search"))


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
            for key in NAMES:
                results.setdefault((key, label), []).extend(got[key])
    for (key, label), runs in results.items():
        line(NAMES[key][0], "{}, {} (fresh processes)".format(NAMES[key][1], label), runs)
    if parent_library:
        for key in NAMES:
            parent, this = results[(key, "parent commit")], results[(key, "this build")]
            print(json.dumps(dict(
                check="{}: this build's median against the parent's slowest run".format(NAMES[key][1]),
                this_median_ms=round(float(np.median(this)), 3), parent_max_ms=round(max(parent), 3),
                parent_median_ms=round(float(np.median(parent)), 3),
                visit_order=["parent, this", "this, parent"],
                passed=bool(np.median(this) <= max(parent)))), flush=True)


def trace_child():
    """A few iterations of the search, for a kernel trace."""
    engine = search_engine(0.01)
    engine.lindblad_upload_controls(controls())
    engine.lindblad_opt_begin()
    iteration = resident_iteration(engine, K_CTRL)
    for _ in range(6):
        iteration()
    engine.close()


def trace_summary(database):
    """One line with the per-launch times (us) of the search's kernels in a rocprofv3 kernel trace
    of trace_child(), read from its rocpd (SQLite) database."""
    import sqlite3
    rows = sqlite3.connect(database).execute('select name, "end" - start from kernels').fetchall()
    out = {}
    for kernel in ("lindblad_duration_generators_kernel", "lindblad_duration_gradient_kernel",
                   "duration_tables_kernel", "duration_step_kernel", "sweep_sensitivity_kernel"):
        times = [duration / 1e3 for name, duration in rows if kernel in name]
        out[kernel] = dict(launches=len(times), us_min=round(min(times), 2),
                           us_median=round(float(np.median(times)), 2), us_max=round(max(times), 2))
    print(json.dumps(dict(mode="t", what="per-launch times of the Lindblad duration search's kernels "
                                         "(rocprofv3 --kernel-trace, a run of its own)",
                          n=bench.LB_DIM, steps=N_EVAL - 1, seeds=SEEDS, controls=K_CTRL,
                          dispatches=len(rows), **out)), flush=True)


def main(parent_library):
    gate(parent_library)  # (before this process opens the device)
    h0, g, gam, _, _, _ = bench.lindblad_problem()
    u = controls()
    search = search_engine(0.0)
    with_rates, without = sweep_engine(), sweep_engine()
    with_rates.lindblad_sweep_want_rate_sensitivities(True)
    for engine in (search, with_rates, without):
        engine.lindblad_upload_controls(u)
        engine.lindblad_opt_begin()
    s_runs, r_runs, f_runs = in_turns([resident_iteration(e, K_CTRL)
                                       for e in (search, with_rates, without)])
    s = line("s", "resident Adam iteration of the 64-duration Lindblad search, in turns with (r), (f)",
             s_runs)
    r = line("r", "resident Adam iteration of the same sweep with fixed durations and rate "
                  "sensitivities, in turns with (s), (f)", r_runs)
    f = line("f", "resident Adam iteration of the same sweep with fixed durations, without rate "
                  "sensitivities, in turns with (s), (r)", f_runs)
    print(json.dumps(dict(check="search iteration against the fixed-duration iterations (reported, "
                                "not asserted)", search_median_ms=s["ms_median"],
                          fixed_with_rates_median_ms=r["ms_median"],
                          fixed_median_ms=f["ms_median"],
                          search_minus_fixed_with_rates_us=round(
                              (s["ms_median"] - r["ms_median"]) * 1e3, 1))), flush=True)
    moved = search.lindblad_sweep_download_durations(want_grad=False)[0]
    print(json.dumps(dict(check="the search moved the durations", seeds_moved=int(np.sum(
        moved != np.minimum(np.maximum(taus(), TAU_BOX[0]), TAU_BOX[1]))), seeds=SEEDS)), flush=True)
    for engine in (search, with_rates, without):
        engine.close()
    # (u): the same search without the feature - the tables change every iteration, so every
    # iteration sets the problem and the sweep again, and brings the sensitivities to the host
    user = engine_mod.Engine(0)
    tau = taus()

    def users_iteration():
        set_problem(user, np.zeros_like(h0), list(g) + [h0], gam)
        user.set_lindblad_sweep(np.repeat(tau[:, None], K_CTRL, axis=1), tau[:, None],
                                np.repeat(tau[:, None], len(gam), axis=1))
        user.lindblad_sweep_want_rate_sensitivities(True)
        user.evaluate_lindblad(u)
        assert user.lindblad_sweep_sensitivities()[2] is not None
    line("u", "one iteration of the search as a user's loop: problem set-up, qocx_lindblad_set_sweep, "
              "upload, evaluation with rate sensitivities, gradients and the three tables to the host",
         runs_of(users_iteration, reps=5))
    user.close()


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--parent-library")
    parser.add_argument("--gate-library")
    parser.add_argument("--gate-only", action="store_true")
    parser.add_argument("--trace-child", action="store_true")
    parser.add_argument("--trace-summary")
    args = parser.parse_args()
    if args.gate_library:
        gate_child(args.gate_library)
    elif args.trace_child:
        trace_child()
    elif args.trace_summary:
        trace_summary(args.trace_summary)
    elif args.gate_only:
        gate(args.parent_library)
    else:
        main(args.parent_library)
