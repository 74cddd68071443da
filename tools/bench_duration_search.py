"""
bench_duration_search.py - GPU-BOX TOOLING: what optimising the durations of a 256-duration sweep
costs per resident iteration (qocx_sweep_set_durations, qocx_duration.hip), what the same search
costs as a user's loop without the feature, and the gate that runs which do not ask for a search
cost what they cost on the parent commit.

The shape of tools/bench_sweep.py, whose helpers this tool uses: n = 32, 1001 system evaluations
(1000 steps), 256 seeds, four real controls, tau_b from 0.5 to 1.5, the drift as the fixed channel
D_0; resident Adam. Three runs per line, each the mean over 20 timed repetitions after a warm one;
(s) and (f) run in turns in one process.

    (s)  one resident Adam iteration of the search: qocx_opt_clip (clips tau, rewrites the tables),
         qocx_eval_resident (expand, 256 items, reduce, the sensitivity kernel, the tau gradient),
         256 costs to the host, qocx_opt_step (steps the controls and tau)
    (f)  the same iteration of the sweep with fixed durations: (s) minus (f) is the cost of the feature
    (u)  the search as a user's loop over the plain sweep: per iteration a problem set-up, qocx_set_sweep
         with the new tables, an upload, an evaluation and the sensitivities to the host
    (p)  a plain 256-seed evaluation of the 4-channel problem   } fresh process per library: this build
    (w)  one resident Adam iteration of the fixed-duration      } and - with --parent-library PATH - the
         sweep, no search                                       } parent commit's, alternating, order
                                                                } swapped between the two visits

This build's median of (p) and (w) must not lie above the parent's slowest run: the check lines, the
rule of tools/bench_sweep.py.

    python tools/bench_duration_search.py [--parent-library PATH] > profiles/duration_search.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o search -- python tools/bench_duration_search.py --trace-child
    python tools/bench_duration_search.py --trace-summary DIR/search_results.db >> profiles/duration_search.jsonl
        (a run of its own: the per-launch times of the three kernels of qocx_duration.hip and of
        sweep_sensitivity_kernel, read from the trace's rocpd database)
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qoc_amd import engine as engine_mod  # noqa: E402
from tools import bench_sweep as base  # noqa: E402
from tools.bench_sweep import (K_CTRL, N_EVAL, SEEDS, alternating, controls, line, problem,  # noqa: E402
                               resident_iteration, runs_of, set_problem, sweep_engine, taus)

NEW_SYMBOLS = ("qocx_sweep_set_durations", "qocx_sweep_download_durations",
               "qocx_opt_download_best_durations")
TAU_BOX = (0.4, 1.6)


def search_engine(time_weight=0.0):
    """(engine with the 256-duration sweep as a search, its seed controls)."""
    engine, u = sweep_engine()
    engine.sweep_set_durations(taus(), None, np.ones((SEEDS, 1)), *TAU_BOX, time_weight)
    return engine, u


def gate_child(library):
    """Modes (p) and (w) in this process, on the library at `library`: nothing here sets durations."""
    try:
        engine_mod.load_library(library)
    except AttributeError:  # the parent commit's library: no durations symbols to bind
        for name in NEW_SYMBOLS:
            engine_mod.SIGNATURES.pop(name, None)
        engine_mod.load_library(library)
    h0, g, _, _ = problem()
    u = controls()
    engine = engine_mod.Engine(0)
    set_problem(engine, h0, g)
    plain = runs_of(lambda: engine.evaluate(u))
    engine.close()
    sweep, u = sweep_engine()
    sweep.upload_controls(u)
    sweep.opt_begin()
    iteration = runs_of(resident_iteration(sweep, K_CTRL))
    sweep.close()
    print(json.dumps(dict(library=library, plain=plain, iteration=iteration)), flush=True)


def gate(parent_library):
    """This build and the parent's library in fresh processes, alternating, two visits each, the
    second in the opposite order."""
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
                 iteration=("w", "resident Adam iteration of the fixed-duration sweep, no search"))
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


def trace_child():
    """A few iterations of the search, for a kernel trace."""
    engine, u = search_engine(0.01)
    engine.upload_controls(u)
    engine.opt_begin()
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
    for kernel in ("duration_tables_kernel", "duration_gradient_kernel", "duration_step_kernel",
                   "sweep_sensitivity_kernel"):
        times = [duration / 1e3 for name, duration in rows if kernel in name]
        out[kernel] = dict(launches=len(times), us_min=round(min(times), 2),
                           us_median=round(float(np.median(times)), 2), us_max=round(max(times), 2))
    print(json.dumps(dict(mode="t", what="per-launch times of the duration search's kernels "
                                         "(rocprofv3 --kernel-trace, a run of its own)", n=base.DIM,
                          steps=N_EVAL - 1, seeds=SEEDS, controls=K_CTRL, dispatches=len(rows),
                          **out)), flush=True)


def main(parent_library):
    gate(parent_library)  # (before this process opens the device)
    h0, g, _, _ = problem()
    search, u = search_engine(0.01)
    search.upload_controls(u)
    search.opt_begin()
    fixed, _ = sweep_engine()
    fixed.upload_controls(u)
    fixed.opt_begin()
    s_runs, f_runs = alternating(resident_iteration(search, K_CTRL),
                                 resident_iteration(fixed, K_CTRL))
    s = line("s", "resident Adam iteration of the 256-duration search, in turns with (f)", s_runs)
    f = line("f", "resident Adam iteration of the same sweep with fixed durations, in turns with (s)",
             f_runs)
    print(json.dumps(dict(check="search iteration against the fixed-duration iteration (reported, "
                                "not asserted)", fixed_ms=[f["ms_min"], f["ms_max"]],
                          search_ms=[s["ms_min"], s["ms_max"]],
                          fixed_median_ms=float(np.median(f_runs)),
                          search_median_ms=float(np.median(s_runs)),
                          difference_of_medians_us=round(
                              (float(np.median(s_runs)) - float(np.median(f_runs))) * 1e3, 1))),
          flush=True)
    moved = search.sweep_download_durations(want_grad=False)[0]
    print(json.dumps(dict(check="the search moved the durations", seeds_moved=int(np.sum(
        moved != np.minimum(np.maximum(taus(), TAU_BOX[0]), TAU_BOX[1]))), seeds=SEEDS)), flush=True)
    search.close()
    # (u): the same search without the feature - the tables change every iteration, so every
    # iteration sets the problem and the sweep again
    tau = taus()
    wide_g = np.concatenate([g, h0[None]])

    def user_iteration():
        set_problem(fixed, np.zeros_like(h0), wide_g)
        fixed.set_sweep(np.repeat(tau[:, None], K_CTRL, axis=1), tau[:, None])
        fixed.upload_controls(u)
        fixed.eval_resident(True)
        fixed.download_results()
        fixed.sweep_sensitivities()
    line("u", "one iteration of the search as a user's loop: problem set-up, qocx_set_sweep, upload, "
              "evaluation, gradients and sensitivities to the host", runs_of(user_iteration, reps=5))
    fixed.close()


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--parent-library", default=None,
                        help="libqocx.so built from the parent commit: the gate times it too")
    parser.add_argument("--gate-library", default=None, help=argparse.SUPPRESS)
    parser.add_argument("--trace-child", action="store_true",
                        help="a few iterations of the search, for a kernel trace")
    parser.add_argument("--trace-summary", default=None, metavar="DATABASE",
                        help="the search kernels' per-launch times from a kernel trace of --trace-child")
    args = parser.parse_args()
    if args.trace_summary:
        trace_summary(args.trace_summary)
    elif args.gate_library:
        gate_child(args.gate_library)
    elif args.trace_child:
        trace_child()
    else:
        main(args.parent_library)
