"""
measure_lindblad_exact.py - CPU only: the discretisation error of the device scheme, measured by its
NumPy model (tests/lindblad_model.py, tests/lindblad_sweep_model.py) against the exact references of
tests/lindblad_exact.py over the case table of tests/lindblad_exact_cases.py. One JSON line per case
goes to profiles/lindblad_exact.jsonl, and a last line holds the worst number of every quantity: the
gate constants of tests/lindblad_exact.py quote that line.

    python tools/measure_lindblad_exact.py [--out profiles/lindblad_exact.jsonl] [case ...]

The engine is never run here: a gate comes from the scheme's own error and from the precision of the
references, not from what the code under test gives.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import lindblad_exact_cases as xc  # noqa: E402

# quantity of compare() -> the gate of tests/lindblad_exact.py it feeds
GROUPS = {"cost": "cost", "member_cost": "cost", "densities": "densities", "gradient": "gradient",
          "scale_sens": "sensitivities", "offset_sens": "sensitivities",
          "rate_sens": "sensitivities", "tau_grad": "sensitivities"}


def measure(name):
    case = xc.build(name)
    start = time.time()
    exact = xc.exact_results(name)
    middle = time.time()
    errors = xc.compare(xc.model_results(name), exact)
    line = dict(case=name, kind=case.kind, n=case.n, L=case.L, S=case.S, N=case.N, Nc=case.Nc,
                model_vs_exact=errors, exact_seconds=round(middle - start, 3),
                model_seconds=round(time.time() - middle, 3))
    if "disagreement" in exact:
        line["two_method_disagreement"] = exact["disagreement"]
    if case.kind == "search":
        line["shares"] = case.base
    return line


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "lindblad_exact.jsonl"))
    parser.add_argument("cases", nargs="*")
    args = parser.parse_args()
    names = args.cases or xc.NAMES
    worst = {}
    lines = []
    for name in names:
        line = measure(name)
        lines.append(line)
        print(json.dumps(line), flush=True)
        linear = line["kind"] == "linear"
        for key, value in line["model_vs_exact"].items():
            group = ("linear_" + ("derivative" if key == "derivative" else key) if linear
                     else GROUPS[key])
            if value > worst.get(group, (0.0, None))[0] or group not in worst:
                worst[group] = (value, name)
        for key, value in line.get("two_method_disagreement", {}).items():
            group = "linear_two_method_" + key
            if value > worst.get(group, (0.0, None))[0] or group not in worst:
                worst[group] = (value, name)
    summary = dict(worst={k: dict(value=v[0], case=v[1]) for k, v in sorted(worst.items())})
    print(json.dumps(summary), flush=True)
    if not args.cases:
        with open(args.out, "w") as f:
            for line in lines + [summary]:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
