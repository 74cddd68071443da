"""
record_action_grad_bits.py - GPU-BOX TOOLING: record what the matrix-free route computes on the problems of
tests/action_grad_cases.py - cost, gradient and final states of every case, one .npz each - so that a change
of its gradient kernel that must not move a bit (tests/test_gpu_action_grad_bits.py) is held to the library
it started from. Run it once on the PARENT's library:

    python tools/record_action_grad_bits.py --library path/to/parent/libqocx.so [--out tests/golden/action_grad]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import action_grad_cases as cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library", default=None, help="the library to record (default: this build's)")
    ap.add_argument("--out", default=cases.GOLDEN)
    args = ap.parse_args()
    from qoc_amd import engine as engine_mod
    if args.library:
        engine_mod.LIBRARY_PATH = os.path.abspath(args.library)
    os.makedirs(args.out, exist_ok=True)
    engine = engine_mod.Engine(0)
    for n, K, shape in cases.CASES:
        p = cases.case(n, K, shape)
        cases.set_problem(engine, p)
        out = engine.evaluate(p["controls"], True)
        degrees = {m: c for m, c in engine.action_degrees().items() if c}
        assert sum(degrees.values()) == cases.B * (cases.N - 1) and engine.action_reruns() == 0, degrees
        np.savez(cases.golden_path(n, K, shape, args.out), **dict(zip(cases.NAMES, out)))
        print("n={} K={} {} degrees {} cost {}".format(n, K, shape, degrees, out[0]))
    engine.set_knob("action_degree", 1)
    engine.close()


if __name__ == "__main__":
    main()
