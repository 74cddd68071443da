"""
measure_schroedinger_exact.py - CPU only: how far the NumPy models of the Schroedinger routes
(tests/device_model.py under both Pade policies, its explicit-inverse twin with the blocked
Gauss-Jordan elimination of tests/test_general_model.py, tests/action_model.py at the degrees of
tests/action_degree_model.py, all through tests/schroedinger_exact_cases.py: step_model) are from the
exact step propagators of tests/schroedinger_exact.py, over the case table of
tests/schroedinger_exact_cases.py. One JSON line per case goes to profiles/schroedinger_exact.jsonl;
then one line per mpmath self-check of the reference ("mpmath": the smallest case of each kind at 40
digits), and a last line holds the worst number of every quantity per gate family ("worst") and of the
self-checks ("mpmath_worst"): the gate constants of tests/schroedinger_exact.py quote that line.

    python tools/measure_schroedinger_exact.py [--out profiles/schroedinger_exact.jsonl] [case ...]

The engine is never run here: a gate comes from the rounding of the scheme's own arithmetic and from
the precision of the reference, not from what the code under test gives. Numbers are rounded up to three
significant digits and no timings are kept, so that a rerun reproduces the file (the products of the
cases above n = 64 may move in their last digit with the number of BLAS threads).
"""

import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import schroedinger_exact as ex  # noqa: E402
from tests import schroedinger_exact_cases as xc  # noqa: E402


def rounded(value):
    """Up to three significant digits: a gate of ten times the number is never below the number."""
    if not value > 0:
        return 0.0
    scale = 10.0 ** (math.floor(math.log10(value)) - 2)
    return float("%.3g" % (math.ceil(value / scale) * scale))


def measure(name):
    case = xc.build(name)
    exact = xc.exact_results(name)
    errors = {k: rounded(v) for k, v in xc.compare(xc.model_results(name), exact).items()}
    dec = xc.decisions(case)
    line = dict(case=name, family=case.family, kind=case.kind, ops=case.ops, model=case.model, n=case.n,
                S=case.S, K=case.K, N=case.N, Nc=case.Nc, magnus=case.magnus, level=rounded(case.level),
                model_vs_exact=errors)
    if case.model == "action":
        line["degrees"] = sorted(set(int(m) for m in dec["degree"].ravel()))
    else:
        line["orders"] = sorted(set(int(m) for m in dec["order_table"].ravel()))
        line["squarings"] = sorted(set(int(s) for s in dec["squarings"].ravel()))
    if case.kind == "search":
        line["shares"] = case.base
    return line


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "schroedinger_exact.jsonl"))
    parser.add_argument("cases", nargs="*")
    args = parser.parse_args()
    names = args.cases or xc.NAMES
    worst = {family: {} for family in ex.FAMILIES}
    lines = []
    for name in names:
        line = measure(name)
        lines.append(line)
        print(json.dumps(line), flush=True)
        for key, value in line["model_vs_exact"].items():
            group = ex.QUANTITY_GATE[key]
            seen = worst[line["family"]]
            if group not in seen or value > seen[group]["value"]:
                seen[group] = dict(value=value, case=name)
    mp_worst = {}
    if not args.cases:
        for name in xc.MPMATH_CASES:
            check = {k: rounded(v) for k, v in xc.mpmath_disagreement(name).items()}
            line = dict(mpmath=name, disagreement=check)
            lines.append(line)
            print(json.dumps(line), flush=True)
            for key, value in check.items():
                if key not in mp_worst or value > mp_worst[key]["value"]:
                    mp_worst[key] = dict(value=value, case=name)
    summary = dict(worst=worst, mpmath_worst=mp_worst)
    print(json.dumps(summary), flush=True)
    if not args.cases:
        with open(args.out, "w") as f:
            for line in lines + [summary]:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
