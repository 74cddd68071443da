"""
CPU tests (-m "not gpu") of tests/action_costs_cases.py, with the oracle alone: the problems that
tests/test_gpu_action_costs.py holds the kernels of qoc_amd/csrc/qocx_action_costs.hip to could not be
passed by a kernel that misread the cost table or left a descriptor out - the conditions of
tests/test_state_costs_host.py on this fixture, for every (set, n, N) and seed by seed:

  * every misreading of the cost table that applies at S = 1 (state_costs.mutants: the second forbid
    reading the counts of the first; step costs left out at, or counted at, the final step) moves the
    oracle's gradient by >= 1e-3 of its largest entry - 1e5 parity gates - and the cost by >= 1e-6;
  * every descriptor of a set of several holds >= 10 % of the max-norm of the set's gradient;
  * every gradient stands above the floor of the gradient gate (1e-3);
  * the Taylor degrees the step table will choose span at least three values per problem.
"""

import numpy as np
import pytest

from tests import action_costs_cases as acc
from tests import action_model as am
from tests import state_costs as sc


@pytest.mark.parametrize("n", acc.SIZES)
def test_a_misread_cost_table_cannot_pass(n):
    applied = set()
    for N in acc.STEP_COUNTS:
        p = acc.build(n, N)
        assert ((N - 1) % acc.CES == 0) == (N == 13)
        for name in acc.SETS:
            costs = acc.costs_of(name, p)
            muts = sc.mutants(costs, 1, N, acc.CES)
            refs = acc.references(name, p)
            for b, ref in enumerate(refs):
                gmax = np.max(np.abs(ref[1]))
                assert gmax > 1e-3, (name, n, N, b, gmax)
                for mutant, (mcosts, forward) in muts.items():
                    assert forward
                    out = sc.evaluate(p, mcosts, b)
                    move = np.max(np.abs(out[1] - ref[1])) / gmax
                    assert move >= 1e-3, (name, n, N, b, mutant, move)
                    moved = abs(out[0] - ref[0]) / max(1.0, abs(ref[0]))
                    assert moved >= 1e-6, (name, n, N, b, mutant, moved)
                    applied.add(mutant)
                if name in acc.MULTI_SETS:
                    for i, c in enumerate(costs):
                        share = np.max(np.abs(sc.evaluate(p, [c], b)[1])) / gmax
                        assert share >= 0.10, (name, n, N, b, i, share)
    assert applied == {"counts of the first forbid", "final step cost"}


@pytest.mark.parametrize("n", acc.SIZES)
@pytest.mark.parametrize("N", acc.STEP_COUNTS)
def test_the_fixture_is_that_of_the_one_target_tests(n, N):
    """1-norms 1, so a step's bound is DT (1 + sum |u_k|): the quiet seed near degree 8, the loud one up
    to 15; every step within the buffers."""
    from oracle import qoc_numpy as onp
    p = acc.build(n, N)
    assert abs(onp.one_norm(p["h0"]) - 1) < 1e-14 and all(abs(onp.one_norm(m) - 1) < 1e-14 for m in p["g"])
    assert p["controls"].shape == (3, N, acc.K) and p["count"] == (N - 1) // acc.CES == 4
    degrees = set()
    for u in p["controls"]:
        mid = 0.5 * (u[:-1] + u[1:])
        degrees |= {am.degree_for(acc.DT * (1 + np.sum(np.abs(row)))) for row in mid}
    assert len(degrees) >= 3 and 8 <= min(degrees) and max(degrees) <= 15, degrees


def test_the_sets_are_what_the_table_says():
    p = acc.build(20, 13)
    C, I, F = sc.COHERENT, sc.INCOHERENT, sc.FORBID
    want = dict(final_incoherent=[(I, 0)], final_coherent=[(C, 0)], step_coherent=[(C, 1)],
                step_incoherent_alone=[(I, 1)], forbid_ragged=[(F, 1)], two_forbids=[(F, 1), (F, 1)],
                target_after_ragged_forbid=[(F, 1), (I, 1), (C, 0)], two_finals=[(C, 0), (I, 0)],
                forbid_final=[(F, 0)])
    for name, kinds in want.items():
        assert [(c.kind, c.step_cost) for c in acc.costs_of(name, p)] == kinds
    two = acc.costs_of("two_forbids", p)
    assert two[0].counts == [1] and two[1].counts == [3]  # ragged between the descriptors
    assert acc.costs_of("target_after_ragged_forbid", p)[0].counts == [2]
    for d in acc.descriptors("two_forbids", p):
        assert len(d["vectors"]) == sum(d["counts"])
