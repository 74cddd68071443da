"""
bench_control_basis.py - GPU-BOX TOOLING: what a ControlBasis costs in
grape_schroedinger_discrete_batch at the headline shape (bench.py's problem - dim 32, 1000 propagator
steps, 256 seeds - with four real controls, Adam), on one MI355X. Wall time per iteration - between
the moments at which consecutive iterations have their costs on the host, so that a run's set-up (the
start pulses of a P = Nc basis take seconds to expand on the host) stays out of it -, three runs per
line with their range:

  plain      the device-resident iteration without a basis (4004 parameters per seed)
  sine       resident with ControlBasis.sine(1001, 16): 64 coefficients per seed
  sine_host  the same on the host loop (a subclass of Adam counts as "another plugin")
  gaussian   resident with ControlBasis.gaussian_filter(1001, 8): P = Nc, the one shape in which the
             two basis kernels are a billion multiply-adds each

--library PATH loads that build of libqocx.so in the place of the product's. An older build - the
parent commit's, for the comparison of the `plain` line before and after the multi-start driver
learned about a basis - lacks the basis calls: they are left out of the binding and only `plain` can
be run on it.

    python tools/bench_control_basis.py [--library PATH] [--lines plain,sine,sine_host,gaussian]
                                        [--label TEXT] [--out profiles/control_basis.jsonl] [--append]

Per-kernel times: one run of its own under `rocprofv3 --kernel-trace --stats` with
--lines sine,gaussian --runs 1 (profiles/control_basis_kernel_stats.csv).
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
ADAM_LEARNING_RATE = 1e-2  # (tools/bench_multistart.py's)
BASIS_CALLS = ("qocx_opt_begin_basis", "qocx_opt_download_best_params",
               "qocx_lindblad_opt_begin_basis", "qocx_lindblad_opt_download_best_params",
               "qocx_control_basis_apply")


def load(path):
    """The library at `path` under the product's binding; False if it has no basis calls."""
    import ctypes
    probe = ctypes.CDLL(path)
    has_basis = all(hasattr(probe, name) for name in BASIS_CALLS)
    if not has_basis:
        for name in BASIS_CALLS:
            engine_mod.SIGNATURES.pop(name, None)
        for name in ("opt_begin_basis", "opt_download_best_params", "lindblad_opt_begin_basis",
                     "lindblad_opt_download_best_params", "control_basis_apply"):
            delattr(engine_mod.Engine, name)  # (resident_route then sees a backend without them)
    engine_mod.load_library(path)
    return has_basis


def problem():
    from qoc_amd.standard import TargetStateInfidelity
    h0, g, psi0, target = bench.make_problem()
    rng = np.random.default_rng(2004)
    g = list(g) + [bench.gue(rng, bench.DIM) for _ in range(K - len(g))]

    def hamiltonian(u, t):
        out = h0
        for k in range(K):
            out = out + u[k] * g[k]
        return out
    return (K, bench.N_EVAL, [TargetStateInfidelity(target[:, :, None])],
            bench.DT * (bench.N_EVAL - 1), hamiltonian, psi0[:, :, None], bench.N_EVAL)


def starts(rows, sigma):
    return np.stack([sigma * np.random.default_rng(1000 + b).standard_normal((rows, K))
                     for b in range(bench.SEEDS_PER_GPU)])


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "control_basis.jsonl"))
    parser.add_argument("--append", action="store_true")
    parser.add_argument("--library", default=None)
    parser.add_argument("--label", default="this build")
    parser.add_argument("--lines", default="plain,sine,sine_host,gaussian")
    parser.add_argument("--iterations", type=int, default=12)
    parser.add_argument("--runs", type=int, default=3)
    opts = parser.parse_args()
    has_basis = load(opts.library) if opts.library else True
    import qoc_amd
    from qoc_amd.core import batch as batch_mod
    from qoc_amd.standard import Adam, ControlBasis

    class HostAdam(Adam):  # not type(...) is Adam: the host loop
        pass

    taken, stamps = [], []
    for name in ("run_batch_resident", "run_batch_host"):
        def counted(*a, _inner=getattr(batch_mod, name), _name=name, **k):
            taken.append(_name)
            return _inner(*a, **k)
        setattr(batch_mod, name, counted)
    # every iteration brings its costs to the host once: download_costs on the resident route,
    # download_results on the host loop (both wait for the device)
    for name in ("download_costs", "download_results"):
        def stamped(self, *a, _inner=getattr(engine_mod.Engine, name), **k):
            out = _inner(self, *a, **k)
            stamps.append(time.perf_counter())
            return out
        setattr(engine_mod.Engine, name, stamped)

    args = problem()
    nc = bench.N_EVAL
    cases = {
        "plain": (None, starts(nc, 0.1), Adam, "run_batch_resident", opts.iterations),
        "sine": (lambda: ControlBasis.sine(nc, 16), starts(16, 0.02), Adam, "run_batch_resident",
                 opts.iterations),
        "sine_host": (lambda: ControlBasis.sine(nc, 16), starts(16, 0.02), HostAdam,
                      "run_batch_host", max(2, opts.iterations // 3)),
        "gaussian": (lambda: ControlBasis.gaussian_filter(nc, 8.0), starts(nc, 0.1), Adam,
                     "run_batch_resident", opts.iterations),
    }

    def run(basis, u0, make, count):
        """ms per iteration over the last count - 1 of count iterations, and the result"""
        kw = {} if basis is None else dict(control_basis=basis)
        del stamps[:]
        result = qoc_amd.grape_schroedinger_discrete_batch(
            *args, u0.copy(), iteration_count=count, log_iteration_step=0,
            optimizer=make(learning_rate=ADAM_LEARNING_RATE), max_control_norms=np.ones(K), **kw)
        assert len(stamps) == count, (len(stamps), count)
        return (stamps[-1] - stamps[0]) / (count - 1) * 1e3, result

    lines = []
    for line in opts.lines.split(","):
        make_basis, u0, make, route, iterations = cases[line]
        if make_basis is not None and not has_basis:
            raise SystemExit("{} has no basis calls: only --lines plain".format(opts.library))
        basis = make_basis() if make_basis is not None else None
        run(basis, u0, make, 2)  # warm
        samples = []
        for _ in range(opts.runs):
            del taken[:]
            sample, result = run(basis, u0, make, 2 * iterations + 1)
            assert taken == [route], taken
            samples.append(sample)
        record = dict(
            measurement="ms_per_iteration", line=line, library=opts.label, route=route,
            basis=None if basis is None else repr(basis), optimizer="Adam",
            parameters_per_seed=u0.shape[1] * K, iterations=2 * iterations,
            ms_per_iteration=dict(median=round(float(np.median(samples)), 3),
                                  min=round(min(samples), 3), max=round(max(samples), 3)),
            runs=[round(s, 3) for s in samples], best_error=float(result.best.best_error),
            dim=bench.DIM, steps=bench.N_EVAL - 1, seeds=bench.SEEDS_PER_GPU, controls=K)
        lines.append(json.dumps(record))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(opts.out)), exist_ok=True)
    with open(opts.out, "a" if opts.append else "w") as handle:
        handle.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
