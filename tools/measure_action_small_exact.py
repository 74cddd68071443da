"""
measure_action_small_exact.py - CPU only: how far the NumPy model of the matrix-free route
(tests/action_model.py at the degrees of tests/action_degree_model.py) is from the exact step propagators
of tests/schroedinger_exact.py on the cases of tests/action_small_exact_cases.py (n = 3, 8, 16), by the
method of tools/measure_schroedinger_exact.py. One JSON line per case and a last line with the worst number
of every quantity ("worst") go to profiles/action_small_exact.jsonl: the gates of
tests/test_gpu_action_small_exact.py quote that line.

    python tools/measure_action_small_exact.py [--out profiles/action_small_exact.jsonl]

The engine is never run here.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tools")):
    if path not in sys.path:
        sys.path.insert(0, path)

import measure_schroedinger_exact as base  # noqa: E402
from tests import action_small_exact_cases as sc  # noqa: E402
from tests import schroedinger_exact as ex  # noqa: E402


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "action_small_exact.jsonl"))
    args = parser.parse_args()
    worst, lines = {}, []
    for name in sc.NAMES:
        sc.build(name)
        line = base.measure(name)
        lines.append(line)
        print(json.dumps(line), flush=True)
        for key, value in line["model_vs_exact"].items():
            group = ex.QUANTITY_GATE[key]
            if group not in worst or value > worst[group]["value"]:
                worst[group] = dict(value=value, case=name)
    summary = dict(worst=worst)
    print(json.dumps(summary), flush=True)
    with open(args.out, "w") as f:
        for line in lines + [summary]:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
