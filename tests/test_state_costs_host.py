"""
CPU tests (-m "not gpu") of tests/state_costs.py: the references that tests/test_gpu_state_costs.py holds
the cost code of every sweep route to are right, and a kernel that misread a cost table could not
pass them.

  * DescriptorCost / DescriptorDensityCost against the oracle's and the product's cost classes wherever
    both can state the cost, to 1e-15;
  * the oracle's gradient with every descriptor set against central differences of its forward pass;
  * the discrimination condition: for every (set, row) the GPU module runs, at both step counts and
    seed by seed, every misreading of the cost table (state_costs.mutants) moves the oracle's gradient
    by >= 1e-3 relative - 1e5 parity gates - and, where it touches the forward value, the cost by >= 1e-6;
  * the share condition: every descriptor of a set of several holds >= 10 % of the max-norm of the
    set's gradient, at every seed;
  * fuzz_parity.one(costs=True) leaves the shared stream of draws what it was.
"""

import numpy as np
import pytest

from oracle import qoc_lindblad_numpy as ol
from oracle import qoc_numpy as onp
from tests import state_costs as sc
from tests.cases import random_density


def _states(rng, S, n):
    return sc._unit_vectors(rng, S, n)[:, :, None]


def _same(a, b, tol=1e-15):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) <= tol


# ---- agreement with the existing classes ----------------------------------------------------------------

@pytest.mark.parametrize("S, n", [(1, 5), (3, 5), (4, 2)])
def test_descriptor_cost_equals_the_oracle_and_product_classes(S, n):
    """Value and cotangent against oracle/qoc_numpy.py, value against qoc_amd.standard through
    device_descriptor() - the dict the product hands the engine - for the three kinds, final and step
    (N = 8, cost_eval_step 3: two evaluations), forbid counts uniform 2 (all an ndarray can state)."""
    from qoc_amd import standard as prod
    rng = np.random.default_rng(100 * S + n)
    psi, targ = _states(rng, S, n), _states(rng, S, n)
    forb = sc._unit_vectors(rng, 2 * S, n).reshape(S, 2, n, 1)
    N, ces = 8, 3
    pairs = []
    for neglect in (False, True):
        kind = sc.INCOHERENT if neglect else sc.COHERENT
        pairs.append((onp.TargetStateInfidelity(targ, neglect, 0.7),
                      prod.TargetStateInfidelity(targ, neglect, 0.7), (kind, 0, 0.7)))
        pairs.append((onp.TargetStateInfidelityTime(N, targ, neglect, ces, 1.3),
                      prod.TargetStateInfidelityTime(N, targ, neglect, ces, 1.3), (kind, 1, 1.3 / 2)))
    pairs.append((onp.ForbidStates(forb, N, ces, 0.9), prod.ForbidStates(forb, N, ces, 0.9),
                  (sc.FORBID, 1, 0.9 / (2 * S))))
    for oracle_cost, product_cost, (kind, step_cost, scale) in pairs:
        desc = product_cost.device_descriptor(S, n)
        assert (desc["kind"], desc["step_cost"]) == (kind, step_cost) and abs(desc["scale"] - scale) < 1e-16
        mine = sc.DescriptorCost(desc["kind"], desc["step_cost"], desc["scale"], desc["vectors"],
                                 desc.get("counts"))
        assert mine.requires_step_evaluation == oracle_cost.requires_step_evaluation == bool(step_cost)
        assert abs(mine.cost(None, psi, 3) - oracle_cost.cost(None, psi, 3)) <= 1e-15
        assert abs(mine.cost(None, psi, 3) - product_cost.cost(None, psi, 3)) <= 1e-15
        assert _same(mine.states_bar(None, psi, 3), oracle_cost.states_bar(None, psi, 3))
        back = mine.descriptor()
        assert back["kind"] == kind and np.array_equal(back["vectors"], desc["vectors"].reshape(-1, n))


@pytest.mark.parametrize("S, n", [(1, 4), (2, 5)])
def test_descriptor_density_cost_equals_the_oracle_and_product_classes(S, n):
    from qoc_amd import standard as prod
    rng = np.random.default_rng(200 * S + n)
    rho = np.stack([random_density(rng, n) for _ in range(S)])
    targ = np.stack([random_density(rng, n) for _ in range(S)])
    forb = np.stack([random_density(rng, n) for _ in range(2 * S)]).reshape(S, 2, n, n)
    N, ces = 7, 2
    pairs = [(ol.TargetDensityInfidelity(targ, 0.8), prod.TargetDensityInfidelity(targ, 0.8)),
             (ol.TargetDensityInfidelityTime(N, targ, ces, 1.2), prod.TargetDensityInfidelityTime(N, targ, ces, 1.2)),
             (ol.ForbidDensities(forb, N, ces, 1.5), prod.ForbidDensities(forb, N, ces, 1.5))]
    for oracle_cost, product_cost in pairs:
        desc = product_cost.device_descriptor(S, n)
        mine = sc.DescriptorDensityCost(desc["kind"], desc["step_cost"], desc["scale"],
                                        np.asarray(desc["vectors"]).reshape(-1, n, n), desc.get("counts"))
        assert mine.requires_step_evaluation == oracle_cost.requires_step_evaluation
        assert abs(mine.cost(None, rho, 2) - oracle_cost.cost(None, rho, 2)) <= 1e-15
        assert abs(mine.cost(None, rho, 2) - product_cost.cost(None, rho, 2)) <= 1e-15
        assert _same(mine.states_bar(None, rho, 2), oracle_cost.states_bar(None, rho, 2))


def test_ragged_forbid_is_the_sum_of_its_states():
    """What no ndarray can state: counts [1, 3, 2]. Each state with its own uniform ForbidStates (S = 1,
    scale folded by hand) adds up to the ragged descriptor, value and cotangent."""
    rng = np.random.default_rng(5)
    n, counts = 6, [1, 3, 2]
    psi, vec = _states(rng, 3, n), sc._unit_vectors(rng, 6, n)
    mine = sc.DescriptorCost(sc.FORBID, 1, 0.4, vec, counts)
    total, bar, base = 0.0, np.zeros((3, n, 1), dtype=np.complex128), 0
    for s, fs in enumerate(counts):
        one = onp.ForbidStates(vec[base:base + fs].reshape(1, fs, n, 1), 2, 1, 0.4)  # N = 2: count 1
        total += one.cost(None, psi[s:s + 1], 1)
        bar[s] = one.states_bar(None, psi[s:s + 1], 1)[0]
        base += fs
    assert abs(total - mine.cost(None, psi, 1)) <= 1e-15 and _same(bar, mine.states_bar(None, psi, 1))


@pytest.mark.parametrize("name", sc.SETS)
def test_table_read_equals_the_descriptors(name):
    """TableCost with no option set - the device's pool, counts array and offsets read rightly - is
    the descriptor itself, for every cost of every set (S = 3: ragged counts, offsets behind them)."""
    p = sc.build(sc._row("host", 5, 3), 7)
    costs = sc.descriptor_set(name, p)
    table = sc.device_table(costs)
    psi = _states(np.random.default_rng(9), 3, 5)
    offset = 0
    for i, c in enumerate(costs):
        assert table[2][i][0] == offset
        offset += len(c.vectors)
        read = sc.TableCost(table, i, c)
        assert abs(read.cost(None, psi, 3) - c.cost(None, psi, 3)) <= 1e-15
        assert _same(read.states_bar(None, psi, 3), c.states_bar(None, psi, 3))
    assert offset == len(table[0])


# ---- finite differences ---------------------------------------------------------------------------------

def central_differences(f, u, h=1e-5):
    out = np.empty(u.shape)
    for idx in np.ndindex(*u.shape):
        up, dn = u.copy(), u.copy()
        up[idx] += h
        dn[idx] -= h
        out[idx] = (f(up) - f(dn)) / (2 * h)
    return out


@pytest.mark.parametrize("N", sc.STEP_COUNTS)
@pytest.mark.parametrize("name", sc.SETS)
def test_oracle_gradient_against_finite_differences(name, N):
    """n = 5, S = 3, the loud seeds: the oracle's gradient with the set's DescriptorCosts against central
    differences (h = 1e-5) of its forward pass, at the project's finite-difference gate of 1e-7 relative
    (measured: <= 1.3e-9)."""
    p = sc.build(sc._row("host", 5, 3), N)
    costs = sc.descriptor_set(name, p)
    prob = sc.oracle_problem(p, costs)
    for b in (1, 2):
        u = p["controls"][b]
        grads = onp.evaluate_with_grad(prob, u)[1]
        fd = central_differences(lambda v: onp.evaluate(prob, v)[0], u)
        rel = np.max(np.abs(grads - fd)) / np.max(np.abs(fd))
        print("{} N={} seed {}: gradient against differences {:.2e}".format(name, N, b, rel))
        assert rel < 1e-7


def test_lindblad_model_gradient_with_density_descriptors():
    """tests/lindblad_model.py with DescriptorDensityCosts (ragged forbid counts, a step target), n = 4:
    gate 1e-7 relative."""
    q = sc.lindblad_problem(4, 1)
    costs = sc.lindblad_set("two_forbids", q, 2) + sc.lindblad_set("target_step", q, 2)
    u = q["controls"][0]

    def run(v, want_grad):
        return sc.lindblad_model_run(dict(q, controls=[v]), costs, 2, 0, want_grad)

    fd = central_differences(lambda v: run(v, False)[0], u)
    rel = np.max(np.abs(run(u, True)[1] - fd)) / np.max(np.abs(fd))
    print("Lindblad model with density descriptors: gradient against differences {:.2e}".format(rel))
    assert rel < 1e-7


# ---- discrimination and share --------------------------------------------------------------------------

def _shapes():
    """The distinct (n, S, kind) of the rows: the conditions do not depend on the route's knobs."""
    out = {}
    for row in sc.ROWS:
        out.setdefault((row["n"], row["S"], row["kind"]), row)
    return list(out.values())


@pytest.mark.parametrize("row", _shapes(), ids=lambda r: "n{n}_S{S}_{kind}".format(**r))
def test_a_misread_cost_table_cannot_pass(row):
    """Every (set, row) of the GPU module, N = 7 and 8, seed by seed: each applicable misreading moves
    the gradient by >= 1e-3 of max(|g|, 1e-3) and - but for the scalar of state 0, which leaves the
    forward pass alone - the cost by >= 1e-6; and every descriptor of a set of several holds >= 10 % of
    the max-norm of the set's gradient."""
    applied = set()
    for N in sc.STEP_COUNTS:
        p = sc.build(row, N)
        assert ((N - 1) % p["ces"] == 0) == (N == 7)
        for name in sc.SETS:
            assert (name, row["name"]) in sc.pairs()
            costs = sc.descriptor_set(name, p)
            muts = sc.mutants(costs, p["S"], N)
            for b in range(len(sc.SIGMAS)):
                ref = sc.evaluate(p, costs, b)
                gmax = np.max(np.abs(ref[1]))
                assert gmax > 1e-3, (name, N, b, gmax)  # (above the floor of the gradient gate)
                for mutant, (mcosts, forward) in muts.items():
                    out = sc.evaluate(p, mcosts, b)
                    move = np.max(np.abs(out[1] - ref[1])) / gmax
                    assert move >= 1e-3, (name, N, b, mutant, move)
                    if forward:
                        moved = abs(out[0] - ref[0]) / max(1.0, abs(ref[0]))
                        assert moved >= 1e-6, (name, N, b, mutant, moved)
                    else:
                        assert abs(out[0] - ref[0]) <= 1e-14 * abs(ref[0]) and np.array_equal(out[2], ref[2])
                    applied.add(mutant)
                if name in sc.MULTI_SETS:
                    for i, c in enumerate(costs):
                        share = np.max(np.abs(sc.evaluate(p, [c], b)[1])) / gmax
                        assert share >= 0.10, (name, N, b, i, share)
    want = {"counts of the first forbid", "final step cost"}
    if row["S"] >= 2:
        want |= {"kinds swapped", "scalar of state 0", "counts uniform", "vec_offset uniform"}
    assert applied == want


def test_the_sets_are_what_the_table_says():
    """Kinds, step flags and counts of the nine sets at S = 5; ragged counts, a count above 2, a second
    forbid with cnt_offset != 0 and other counts, descriptors behind a ragged sum."""
    p = sc.build(sc._row("host", 6, 5), 8)
    C, I, F = sc.COHERENT, sc.INCOHERENT, sc.FORBID
    want = dict(final_incoherent=[(I, 0)], final_coherent=[(C, 0)], step_coherent=[(C, 1)],
                step_incoherent_alone=[(I, 1)], forbid_ragged=[(F, 1)], two_forbids=[(F, 1), (F, 1)],
                target_after_ragged_forbid=[(F, 1), (I, 1), (C, 0)], two_finals=[(C, 0), (I, 0)],
                forbid_final=[(F, 0)])
    assert set(want) == set(sc.SETS)
    for name, kinds in want.items():
        costs = sc.descriptor_set(name, p)
        assert [(c.kind, c.step_cost) for c in costs] == kinds
        for c in costs:
            if c.kind == F:
                assert len(set(c.counts)) > 1 and max(c.counts) > 2 and len(c.vectors) == sum(c.counts)
    assert sc.descriptor_set("forbid_ragged", p)[0].counts == [1, 3, 2, 5, 1]
    two = sc.descriptor_set("two_forbids", p)
    assert two[0].counts != two[1].counts and not np.array_equal(two[0].vectors[0], two[1].vectors[0])
    finals = sc.descriptor_set("two_finals", p)
    assert not np.allclose(finals[0].vectors, finals[1].vectors)
    assert np.max(np.abs(p["vec"]["A"].imag)) > 0.1  # complex targets
    assert sc.unit_adjoint_applies("final_coherent", 5) and not sc.unit_adjoint_applies("final_incoherent", 5)
    assert sc.unit_adjoint_applies("final_incoherent", 1) and not sc.unit_adjoint_applies("two_finals", 1)


@pytest.mark.parametrize("n, L", [(4, 1), (16, 2), (20, 2)])
def test_lindblad_sets_bite(n, L):
    """The Lindblad companion, cost_eval_step 1 and 2, seed by seed: each descriptor of a set of two
    holds >= 10 % of the set's gradient, and every cost stays O(1) (the gates are absolute). At n = 4
    also: ragged counts read as uniform, the second forbid reading the first one's counts, and a step
    target evaluated as a final one move the model's gradient by >= 1e-3 relative."""
    q = sc.lindblad_problem(n, L)

    def grad(costs, ces, b):
        return sc.lindblad_model_run(q, costs, ces, b)[1]

    D = sc.DescriptorDensityCost
    for ces in (1, 2):
        for name in ("two_forbids", "two_target_finals"):
            costs = sc.lindblad_set(name, q, ces)
            for b in range(len(q["controls"])):
                err, ref, _ = sc.lindblad_model_run(q, costs, ces, b)
                assert 1e-2 < abs(err) < 20
                gmax = np.max(np.abs(ref))
                for c in costs:
                    assert np.max(np.abs(grad([c], ces, b))) >= 0.10 * gmax, (name, ces, b)
        if n != 4:
            continue
        first, second = sc.lindblad_set("two_forbids", q, ces)
        step = sc.lindblad_set("target_step", q, ces)[0]
        for b in range(len(q["controls"])):
            ref = grad([first, second], ces, b)
            gmax = np.max(np.abs(ref))
            uniform = D(sc.FORBID_DENSITY, 1, first.scale, first.vectors[[0, 1]], [1, 1])
            borrowed = D(sc.FORBID_DENSITY, 1, second.scale, np.concatenate([second.vectors, second.vectors[:1]]),
                         first.counts)
            assert np.max(np.abs(grad([uniform, second], ces, b) - ref)) >= 1e-3 * gmax
            assert np.max(np.abs(grad([first, borrowed], ces, b) - ref)) >= 1e-3 * gmax
            ref = grad([step], ces, b)
            final = D(sc.TARGET_DENSITY, 0, step.scale, step.vectors)
            assert np.max(np.abs(grad([final], ces, b) - ref)) >= 1e-3 * np.max(np.abs(ref))


# ---- fuzz -------------------------------------------------------------------------------------------------

class _Rejecting(object):
    """An engine that turns every draw of fuzz_parity.one away: the problem it is handed is all that is
    wanted."""

    def set_schroedinger_problem(self, *args, **kw):
        self.S, self.costs = args[1], kw["costs"]

    def evaluate(self, *args, **kw):
        from qoc_amd.engine import QocxError
        raise QocxError(-5, "not evaluated")


@pytest.mark.parametrize("seed, kw, then", [(2024, {}, 0.5631835177416028),
                                            (6464, dict(nmin=33, nmax=64), 0.8898187776734643)])
def test_fuzz_draws_with_costs_leave_the_shared_stream_alone(seed, kw, then):
    """fuzz_parity.one(costs=True): the state of the shared stream behind three draws is the one
    recorded before `costs` existed (tests/test_time_dependent_drive_host.py holds the draws themselves
    to their tags); the descriptors come from a generator of their own: 1 to 4 of them, every kind
    over the draws of a seed, ragged counts from 1 to 4."""
    from tests import fuzz_parity
    engine = _Rejecting()
    rng = np.random.default_rng(seed)
    tags, kinds, counts = [], set(), set()
    for index in range(3):
        tags.append(fuzz_parity.one(engine, rng, index, costs=True, **kw)[1])
        assert 1 <= len(engine.costs) <= 4
        for d in engine.costs:
            kinds.add((d["kind"], d["step_cost"]))
            if d["kind"] == sc.FORBID:
                assert len(d["counts"]) == engine.S and len(d["vectors"]) == sum(d["counts"])
                counts.update(d["counts"])
    assert rng.random() == then
    assert all(" costs " in tag for tag in tags)
    assert len(kinds) >= 3 and counts and min(counts) >= 1 and max(counts) <= 4
    plain = np.random.default_rng(seed)
    assert [fuzz_parity.one(engine, plain, i, **kw)[1] for i in range(3)] == [t.split(" costs ")[0] for t in tags]
