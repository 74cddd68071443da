"""
measure_lindblad_wide_exact.py - CPU only: the discretisation error of the device scheme at
33 <= n <= 64, measured by its NumPy model (tests/lindblad_model.py with the norm bound of
tests/lindblad_wide_cases.py) against the exact superoperator reference of tests/lindblad_exact.py over
EXACT_NAMES of tests/lindblad_wide_cases.py. One JSON line per case goes to
profiles/lindblad_wide_exact.jsonl, and a last line holds the worst number of every quantity: the gates
of tests/test_gpu_lindblad_wide.py quote that line (tools/measure_lindblad_exact.py does the same for the
table of n <= 32).

    python tools/measure_lindblad_wide_exact.py [--out profiles/lindblad_wide_exact.jsonl]

The engine is never run here: a gate comes from the scheme's own error and from the precision of the
reference, not from what the code under test gives.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import lindblad_wide_cases as wc  # noqa: E402


def measure(name):
    case = wc.build(name)
    start = time.time()
    exact = wc.exact_results(name)
    middle = time.time()
    errors = wc.compare(wc.model_results(name), exact)
    return dict(case=name, n=case.n, L=case.L, S=case.S, K=case.K, N=case.N, Nc=case.Nc,
                model_vs_exact=errors, exact_seconds=round(middle - start, 3),
                model_seconds=round(time.time() - middle, 3))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "lindblad_wide_exact.jsonl"))
    args = parser.parse_args()
    worst, lines = {}, []
    for name in wc.EXACT_NAMES:
        line = measure(name)
        lines.append(line)
        print(json.dumps(line), flush=True)
        for key, value in line["model_vs_exact"].items():
            if key not in worst or value > worst[key][0]:
                worst[key] = (value, name)
    summary = dict(worst={k: dict(value=v[0], case=v[1]) for k, v in sorted(worst.items())})
    print(json.dumps(summary), flush=True)
    with open(args.out, "w") as f:
        for line in lines + [summary]:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
