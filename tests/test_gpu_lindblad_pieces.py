"""
GPU tests (-m gpu) of the piece schedule of a Lindblad evaluation, observed through the launch counts.

A piece-wise evaluation is bit for bit the one-piece evaluation by design, so no result can tell whether the
launches follow the schedule: a seed group whose stage values fit goes as one piece, one that does not in
pieces that fit, and below `min_piece` seeds per piece as one piece whose adjoint recomputes the stages; a
piece runs two-sided (forward and adjoint launch, then the combine kernel) where it keeps its stage values on
the several-wave launches. The kernel timing counts the launches per family ("lindblad": every forward,
adjoint or classic launch; "lindblad_combine"; "scatter": one per piece with gradients), and
`lindblad_last_subintervals()` the sub-intervals of the evaluation's seeds.
"""

import numpy as np
import pytest

from tests import cases as cases_mod

pytestmark = pytest.mark.gpu

N_HILBERT, S, K, L, N, NC = 4, 1, 2, 2, 6, 4


@pytest.fixture(scope="module")
def engine():
    from qoc_amd.engine import COST_TARGET_DENSITY, Engine
    rng = np.random.default_rng(4711)
    gue, n = cases_mod.gue, N_HILBERT
    h0 = gue(rng, n) * 1.5
    g = [gue(rng, n) for _ in range(K)]
    ops = np.stack([gue(rng, n) + 0.5j * gue(rng, n) for _ in range(L)])
    gam = np.array([0.21, 0.13])
    rho0 = np.stack([cases_mod.random_density(rng, n) for _ in range(S)])
    targ = np.stack([cases_mod.random_density(rng, n) for _ in range(S)])
    e = Engine(0)
    # one final target-density cost: the shape that is eligible for the two-sided evaluation
    e.set_lindblad_problem(n, S, K, NC, N, 0.3 * (N - 1), h0, g, gam, ops, rho0,
                           costs=[dict(kind=COST_TARGET_DENSITY, step_cost=0, scale=0.8, vectors=targ)])
    yield e
    e.close()


def seeds_of_one_group(amplitude, count=8, seed=99):
    """`count` seeds that are sign-flipped copies of two control arrays, the second the first one reversed
    in time: every seed has the same control maxima, so all take the same sub-division count."""
    rng = np.random.default_rng(seed)
    base = amplitude * rng.standard_normal((NC, K))
    pair = (base, base[::-1])
    signs = ((1, 1), (1, -1), (-1, 1), (-1, -1))
    return np.stack([pair[b % 2] * np.array(signs[(b // 2) % 4]) for b in range(count)])


def counted(engine, controls, knobs, want_grad=True):
    """One evaluation under qocx_debug_lindblad_knobs: its results, its (lindblad, combine, scatter) launch
    counts and its sub-interval count."""
    try:
        engine.debug_lindblad_knobs(*knobs)
        engine.set_timing(True)
        engine.reset_timing()
        out = engine.evaluate_lindblad(controls, want_grad=want_grad)
        timing = engine.timing()
        subs = engine.lindblad_last_subintervals()
    finally:
        engine.set_timing(False)
        engine.debug_lindblad_knobs(0, 256, 0)
    counts = tuple(timing[name][0] for name in ("lindblad", "lindblad_combine", "scatter"))
    print("knobs", knobs, "gradients", want_grad, "launches (lindblad, combine, scatter)", counts,
          "sub-intervals", subs)
    return out, counts, subs


# (stage_seeds, min_piece, wave_mode), gradients -> (lindblad, combine, scatter), from the rule:
# fit = stage_seeds or what the budget holds; fit >= 8: one kept piece; fit >= min_piece: kept pieces of fit;
# else one recomputing piece; wave mode 1: one wave per seed (classic launch), 2: several (two-sided where the
# stages are kept); without gradients one piece and no scatter
SCHEDULE = [
    ((0, 256, 1), True, (1, 0, 1)),   # 8, classic
    ((3, 2, 1), True, (3, 0, 3)),     # 3, 3, 2, classic
    ((1, 256, 1), True, (1, 0, 1)),   # 8, recompute
    ((0, 256, 2), True, (2, 1, 1)),   # 8, two-sided
    ((3, 2, 2), True, (6, 3, 3)),     # 3, 3, 2, two-sided
    ((1, 256, 2), True, (1, 0, 1)),   # 8, recompute, so not two-sided
    ((3, 2, 1), False, (1, 0, 0)),    # 8
]


@pytest.mark.parametrize("knobs,want_grad,expected", SCHEDULE)
def test_lindblad_launches_follow_the_piece_schedule(engine, knobs, want_grad, expected):
    controls = seeds_of_one_group(0.7)
    _, counts, subs = counted(engine, controls, knobs, want_grad)
    assert counts == expected
    assert subs % 8 == 0 and subs >= 8 * (N - 1)   # one group: eight seeds of one sub-division count


def test_lindblad_two_groups_launch_apart_and_keep_seed_order(engine):
    """Four seeds at a small amplitude and four at one that needs a finer sub-division, interleaved: two
    groups, a launch and a scatter each, and every seed's results those of its half evaluated alone, bit
    for bit and in seed order."""
    small, large = seeds_of_one_group(0.05, 4, seed=5), seeds_of_one_group(8.0, 4, seed=6)
    mixed = np.empty((8, NC, K))
    mixed[0::2], mixed[1::2] = small, large
    knobs = (0, 256, 1)
    out_small, counts_small, subs_small = counted(engine, small, knobs)
    out_large, counts_large, subs_large = counted(engine, large, knobs)
    out_mixed, counts_mixed, subs_mixed = counted(engine, mixed, knobs)
    assert counts_small == counts_large == (1, 0, 1)
    assert subs_small % 4 == 0 and subs_large % 4 == 0 and subs_small != subs_large
    assert subs_mixed == subs_small + subs_large
    assert counts_mixed == (2, 0, 2)
    for mine, a, b in zip(out_mixed, out_small, out_large):
        assert np.array_equal(mine[0::2], a)
        assert np.array_equal(mine[1::2], b)
        assert np.all(np.isfinite(mine))
