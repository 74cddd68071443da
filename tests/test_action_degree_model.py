"""
CPU tests of the degree rule of the matrix-free route (tests/action_degree_model.py, the NumPy twin of
qoc_amd/csrc/qocx_action.h: action_degree_normal / action_degree_rule, knob "action_degree"): the table
theta'_m = ((m+1)! 2^-53)^(1/(m+1)) and its remainder inequality, the rule against the 1-norm rule it may
never exceed, the truncation error of T_m(a) x for normal a at the table's edge, and the headline problem
of bench.py under both rules against the oracle.
"""

import os
import re

import numpy as np
import pytest

import bench
from oracle import qoc_numpy as onp
from tests import action_degree_model as dm
from tests import action_model as am
from tests.helpers import rel_err

EPS = 2.0 ** -53


def test_table_edges():
    assert sorted(dm.THETA_NORMAL) == list(range(1, dm.MAX_DEGREE + 1))
    for m in range(1, dm.MAX_DEGREE + 1):
        assert dm.degree_normal(dm.THETA_NORMAL[m]) == m
        assert dm.degree_normal(1.02 * dm.THETA_NORMAL[m]) == m + 1
    assert dm.degree_normal(0.0) == 1
    assert dm.degree_normal(float("nan")) == dm.MAX_DEGREE + 1
    assert dm.degree_normal(float("inf")) == dm.MAX_DEGREE + 1


def test_remainder_inequality_holds_at_the_threshold_and_fails_at_the_next():
    """Exact rational arithmetic: theta'_m^(m+1) / (m+1)! <= 2^-53 (each entry is rounded DOWN), the next
    double above it fails, and so does theta'_(m+1) for degree m. The closed form agrees to rounding."""
    for m in range(1, dm.MAX_DEGREE + 1):
        th = dm.THETA_NORMAL[m]
        assert dm.remainder_holds(th, m)
        assert not dm.remainder_holds(float(np.nextafter(th, np.inf)), m)
        if m < dm.MAX_DEGREE:
            assert not dm.remainder_holds(dm.THETA_NORMAL[m + 1], m)
        closed = (float(dm.factorial(m + 1)) * EPS) ** (1.0 / (m + 1))
        assert abs(closed - th) <= 1e-14 * th  # (the roundings of the product, the quotient and pow)


def test_device_header_carries_the_same_table():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qoc_amd", "csrc",
                        "qocx_action.h")
    found = {int(m): float(v) for m, v in re.findall(r"case (\d+): t = ([0-9.e-]+); break;", open(path).read())}
    assert found == dm.THETA_NORMAL


def test_rule_never_exceeds_the_one_norm_rule():
    rng = np.random.default_rng(5)
    grid = np.concatenate([10.0 ** rng.uniform(-17, 0.5, 4000), list(am.THETA.values()),
                           list(dm.THETA_NORMAL.values()), [0.0, np.inf, np.nan]])
    for b1 in grid:
        for ratio in (1.0, 0.5, 0.3, 1e-3):  # ||a||_2 <= ||a||_1 for a Hermitian H; the bound may be anything
            b2 = b1 * ratio
            m = dm.degree_rule(b1, b2, 1)
            assert m <= am.degree_for(b1)
            assert m == min(am.degree_for(b1), dm.degree_normal(b2))
            assert dm.degree_rule(b1, b2, 0) == am.degree_for(b1)
    assert dm.degree_rule(np.nan, np.nan) == dm.MAX_DEGREE + 1
    assert dm.degree_rule(0.05, np.nan) == am.degree_for(0.05)  # no spectral bound: the 1-norm's degree


def taylor_error(a, x, exact, m):
    terms = am.taylor_terms(a, x, m)
    return np.linalg.norm(sum(terms) - exact)


@pytest.mark.parametrize("n", [17, 32])
def test_truncation_error_of_normal_generators_at_the_edge_of_the_table(n):
    """||a||_2 = 0.999 theta'_m: ||T_m(a) x - exp(a) x|| <= 4 * 2^-53 ||x|| + the error of the same sum at
    degree m + 4 - whose truncation is far below 2^-53, so it carries the rounding of the sum and of the
    reference (exp(a) x through eigh) and what is left on the other side is truncation."""
    rng = np.random.default_rng(40 + n)
    for m in range(4, 15):
        g = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
        h = (g + g.conj().T) / 2
        lam, vec = np.linalg.eigh(h)
        scale = 0.999 * dm.THETA_NORMAL[m] / np.abs(lam).max()
        a = -1j * scale * h
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        x /= np.linalg.norm(x)
        exact = vec @ (np.exp(-1j * scale * lam) * (vec.conj().T @ x))
        err, floor = taylor_error(a, x, exact, m), taylor_error(a, x, exact, m + 4)
        print("n={} m={}: error {:.2e} (degree m + 4: {:.2e}; degree m - 1: {:.2e})".format(
            n, m, err, floor, taylor_error(a, x, exact, m - 1)))
        assert err <= 4 * EPS + floor


# ---- the headline problem under both rules ----------------------------------------------------------------

_headline = {}


def headline(seed):
    """bench.py's problem (n = 32, N = 1001, two controls), one seed: the oracle and the model under the
    parent's rule (0) and the new one (1). Computed once per seed."""
    if seed not in _headline:
        h0, g, psi0, target = bench.make_problem()
        controls = bench.make_controls(seed, 1)[0]
        T = bench.DT * (bench.N_EVAL - 1)
        oracle = onp.SchroedingerProblem(
            T, lambda u, t: h0 + u[0] * g[0] + u[1] * g[1], psi0[:, :, None], bench.N_EVAL,
            control_eval_count=bench.N_EVAL, costs=[onp.TargetStateInfidelity(target[:, :, None])],
            control_count=bench.K_CTRL)
        ref = onp.evaluate_with_grad(oracle, controls)
        out = {}
        for rule in (0, 1):
            cost, grads, final, degrees = dm.evaluate_with_grad(h0, g, psi0[0], target[0], bench.N_EVAL, T,
                                                                controls, rule)
            out[rule] = dict(cost=abs(cost - ref[0]), final=float(np.abs(final - ref[2][0, :, 0]).max()),
                             grad=float(rel_err(grads, ref[1])), degrees=sorted(set(degrees)))
        _headline[seed] = out
    return _headline[seed]


@pytest.mark.parametrize("seed", [0, 7])
def test_headline_problem_under_both_rules(seed):
    """Errors against the oracle stay within the suite's gates (1e-10 cost and final state, 1e-8 gradient)
    and within twice the parent rule's errors on the same seed plus 1e-15.

    Measured (final state error, relative gradient error; the parent's rule runs degree 11, with a handful
    of steps at 12 among the 256 seeds - the new rule degree 8 on every step of both seeds):
        seed 0: parent 3.40e-15, 2.55e-14; new 3.56e-15, 2.46e-14
        seed 7: parent 3.72e-15, 1.08e-14; new 3.83e-15, 1.13e-14
    """
    got = headline(seed)
    parent, new = got[0], got[1]
    print("seed {}: parent rule {} | new rule {}".format(seed, parent, new))
    assert set(parent["degrees"]) <= {11, 12} and new["degrees"] == [8]
    for rule in (parent, new):
        assert rule["cost"] < 1e-10 and rule["final"] < 1e-10 and rule["grad"] < 1e-8
    for key in ("cost", "final", "grad"):
        assert new[key] <= 2 * parent[key] + 1e-15, (key, new[key], parent[key])
