"""
bench_piecewise_constant.py - GPU-BOX TOOLING: what an evaluation costs under each
InterpolationPolicy at the headline shape (bench.py's problem - dim 32, 1000 propagator steps, 256
seeds - with four real controls), on one MI355X. Wall time per forward + gradient evaluation of
controls resident in HBM (qocx_eval_resident and the wait for it), three runs per line with their
range:

  linear              LINEAR with Nc = 1001 knots - what bench.py times, with four controls
  piecewise_constant  PIECEWISE_CONSTANT with Nc = 1000 slices, one step per slice

--library PATH loads that build of libqocx.so in the place of the product's. An older build - the
parent commit's, for the comparison that matters: runs under LINEAR launch what they launched
before, so their time must stay within the parent's own run-to-run scatter measured in the same
session - lacks qocx_set_interpolation_policy: the call is left out of the binding and only
`linear` can be run on it.

    python tools/bench_piecewise_constant.py [--library PATH] [--lines linear,piecewise_constant]
                                             [--label TEXT] [--append]
                                             [--out profiles/piecewise_constant.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from qoc_amd import engine as engine_mod  # noqa: E402

K = 4
POLICY_CALL = "qocx_set_interpolation_policy"


def load(path):
    """The library at `path` under the product's binding; False if it knows one policy only."""
    import ctypes
    has_policy = hasattr(ctypes.CDLL(path), POLICY_CALL)
    if not has_policy:
        engine_mod.SIGNATURES.pop(POLICY_CALL, None)
    engine_mod.load_library(path)
    return has_policy


def problem():
    h0, g, psi0, target = bench.make_problem()
    rng = np.random.default_rng(2004)
    g = list(g) + [bench.gue(rng, bench.DIM) for _ in range(K - len(g))]
    return h0, np.stack(g), psi0, target


def starts(rows):
    return np.stack([0.1 * np.random.default_rng(1000 + b).standard_normal((rows, K))
                     for b in range(bench.SEEDS_PER_GPU)])


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "piecewise_constant.jsonl"))
    parser.add_argument("--append", action="store_true")
    parser.add_argument("--library", default=None)
    parser.add_argument("--label", default="this build")
    parser.add_argument("--lines", default="linear,piecewise_constant")
    parser.add_argument("--evaluations", type=int, default=10)
    parser.add_argument("--runs", type=int, default=3)
    opts = parser.parse_args()
    has_policy = load(opts.library) if opts.library else True
    h0, g, psi0, target = problem()
    steps = bench.N_EVAL - 1
    cases = {"linear": steps + 1, "piecewise_constant": steps}
    lines = []
    for line in opts.lines.split(","):
        if line != "linear" and not has_policy:
            raise SystemExit("{} has no {}: only --lines linear".format(opts.library, POLICY_CALL))
        nc = cases[line]
        engine = engine_mod.Engine(0)
        # (a linear problem never makes the policy call: Engine makes it when the policy changes)
        engine.set_schroedinger_problem(
            bench.DIM, 1, K, nc, bench.N_EVAL, bench.DT * steps, h0[None], g[None], psi0,
            costs=[dict(kind=engine_mod.COST_TARGET_COHERENT, step_cost=0, scale=1.0,
                        vectors=target)], interpolation=line)
        engine.upload_controls(starts(nc))

        def evaluate():
            engine.eval_resident(True)
            engine.synchronize()
        for _ in range(5):  # first touch of the buffers, event and signal pools, clocks
            evaluate()
        samples = []
        for _ in range(opts.runs):
            t0 = time.perf_counter()
            for _ in range(opts.evaluations):
                evaluate()
            samples.append((time.perf_counter() - t0) / opts.evaluations * 1e3)
        cost = engine.download_results(want_grad=False, want_final=False)[0]
        record = dict(
            measurement="ms_per_evaluation", line=line, library=opts.label,
            control_eval_count=nc, evaluations=opts.evaluations,
            ms_per_evaluation=dict(median=round(float(np.median(samples)), 3),
                                   min=round(min(samples), 3), max=round(max(samples), 3)),
            runs=[round(s, 3) for s in samples], pade_orders=engine.pade_orders(),
            cost_sum=float(np.sum(cost)), dim=bench.DIM, steps=steps, seeds=bench.SEEDS_PER_GPU,
            controls=K)
        engine.close()
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "a" if opts.append else "w") as handle:
        handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
