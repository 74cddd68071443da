"""
action_small_exact_cases.py - TEST INFRASTRUCTURE: the cases that hold the matrix-free route at n <= 16
(qoc_amd/csrc/qocx_action16.hip, knob "action_small" = 1) to the exact step propagators of
tests/schroedinger_exact.py, built by the case builder of tests/schroedinger_exact_cases.py: ladder and GUE
operators at n = 3, 8 and 16, two seeds, the largest SPECTRAL step bound at 0.97 of a threshold theta'_m of
qoc_amd/csrc/qocx_action.h - a low, a middle and a high degree, each below the host's 1-norm bound theta_18.
Shared by tools/measure_action_small_exact.py (the model against exact, on the CPU:
profiles/action_small_exact.jsonl) and tests/test_gpu_action_small_exact.py (the engine against exact).

Nothing here is imported by the product.
"""

from tests import schroedinger_exact_cases as xc

KNOBS = dict(action_small=1)


def _spec(name, n, degree, ops, **kw):
    return xc._spec(name, "matrix_free", n, xc.NEAR * xc.THN[degree], norm="two", ops=ops, model="action",
                    knobs=KNOBS, degree=degree, **kw)


SPECS = [
    _spec("action_small_n3_ladder_degree6", 3, 6, "ladder", N=6),
    _spec("action_small_n8_ladder_degree11", 8, 11, "ladder"),
    _spec("action_small_n16_ladder_degree14", 16, 14, "ladder"),
    _spec("action_small_n3_gue_degree9", 3, 9, "gue", N=6),
    _spec("action_small_n8_gue_degree7", 8, 7, "gue"),
    _spec("action_small_n16_gue_degree10", 16, 10, "gue"),
]
NAMES = [s["name"] for s in SPECS]


def build(name):
    """The case `name`, through schroedinger_exact_cases.build (which looks a name up in its own tables: the
    spec stands in them for the length of the call; the built case stays in its cache, where exact_results and
    model_results find it)."""
    if name not in xc._BUILT:
        spec = next(s for s in SPECS if s["name"] == name)
        xc.MP_SPECS.append(spec)
        try:
            xc.build(name)
        finally:
            xc.MP_SPECS.remove(spec)
    return xc._BUILT[name]
