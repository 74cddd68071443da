"""
CPU test of the piece schedule of a Lindblad evaluation (qoc_amd/csrc/qocx_lindblad_route.h:
lindblad_group_pieces), through the library's context-free debug entry qocx_debug_lindblad_pieces (no GPU
call): the rows of tests/test_gpu_lindblad_pieces.py as integers, which that test can see through launch
counts only, then the round cap and the stage budget.

The rule: fit = the debug knob's seeds, or what the stage budget holds; fit >= the group: one kept piece;
fit >= min_piece: kept pieces of `fit` seeds; else one piece whose adjoint recomputes the stages - as without
gradients. Several waves per seed (unless wave mode 1) go in rounds of one seed per CU (unless wave mode 2).
"""

import ctypes

import pytest

from qoc_amd import engine

PER_SEED = 5 * 12 * 256   # stage elements of a seed: sub-intervals x stages x a 16 x 16 dump


def pieces(want_grad, multi_wave, knobs, seeds, cu_count=256, stage_budget=0, per_seed=PER_SEED):
    """([(count, keep_stages, multi_wave)], sized_for) of one group under (stage_seeds, min_piece, wave_mode)."""
    stage_seeds, min_piece, wave_mode = knobs
    capacity = seeds
    counts, keep, multi = ((ctypes.c_int32 * capacity)() for _ in range(3))
    found, sized_for = ctypes.c_int32(-1), ctypes.c_int64(-1)
    rc = engine.load_library().qocx_debug_lindblad_pieces(
        int(want_grad), int(multi_wave), stage_budget, stage_seeds, min_piece, wave_mode, cu_count, seeds,
        per_seed, capacity, counts, keep, multi, ctypes.byref(found), ctypes.byref(sized_for))
    assert rc == 0
    assert 1 <= found.value <= capacity
    return [(counts[i], keep[i], multi[i]) for i in range(found.value)], sized_for.value


def listed(counts, keep, multi):
    return [(count, int(keep), int(multi)) for count in counts]


# tests/test_gpu_lindblad_pieces.py: SCHEDULE on its problem (several waves per seed are built for it), Bg = 8
SCHEDULE = [
    ((0, 256, 1), True, [8], True, False),        # 8, classic (the budget below holds the group)
    ((3, 2, 1), True, [3, 3, 2], True, False),    # 3, 3, 2, classic
    ((1, 256, 1), True, [8], False, False),       # 8, recompute
    ((0, 256, 2), True, [8], True, True),         # 8, two-sided
    ((3, 2, 2), True, [3, 3, 2], True, True),     # 3, 3, 2, two-sided
    ((1, 256, 2), True, [8], False, True),        # 8, recompute, so not two-sided
    ((3, 2, 1), False, [8], False, False),        # 8
]


@pytest.mark.parametrize("knobs,want_grad,counts,keep,multi", SCHEDULE)
def test_the_schedule_rows_of_the_gpu_test(knobs, want_grad, counts, keep, multi):
    got, sized_for = pieces(want_grad, True, knobs, 8, stage_budget=1000 * PER_SEED)
    print(knobs, want_grad, "->", got, sized_for)
    assert got == listed(counts, keep, multi)
    assert sized_for == (counts[0] if keep else 0)


def test_rounds_of_one_seed_per_cu_and_buffers_sized_before_the_cap():
    got, sized_for = pieces(True, True, (0, 256, 0), 10, cu_count=4, stage_budget=1000 * PER_SEED)
    assert got == listed([4, 4, 2], True, True)
    assert sized_for == 10
    # the cap is for several waves per seed in wave mode 0 alone
    roomy = dict(cu_count=4, stage_budget=1000 * PER_SEED)
    assert pieces(True, True, (0, 256, 2), 10, **roomy) == (listed([10], True, True), 10)
    assert pieces(True, True, (0, 256, 1), 10, **roomy) == (listed([10], True, False), 10)
    assert pieces(True, False, (0, 256, 0), 10, **roomy) == (listed([10], True, False), 10)
    # ... of kept pieces: the smaller of both, and of a recomputing piece as well
    assert pieces(True, True, (6, 2, 0), 10, cu_count=4) == (listed([4, 4, 2], True, True), 6)
    assert pieces(True, True, (3, 2, 0), 10, cu_count=4) == (listed([3, 3, 3, 1], True, True), 3)
    assert pieces(True, True, (1, 256, 0), 10, cu_count=4) == (listed([4, 4, 2], False, True), 0)
    assert pieces(False, True, (0, 256, 0), 10, cu_count=4) == (listed([4, 4, 2], False, True), 0)


@pytest.mark.parametrize("fit,min_piece,counts,keep", [
    (9, 4, [8], True),            # the budget holds more than the group
    (8, 4, [8], True),            # ... exactly the group
    (7, 4, [7, 1], True),         # ... less: pieces that fit
    (4, 4, [4, 4], True),         # ... exactly min_piece
    (3, 4, [8], False),           # ... less than min_piece: one piece, stages recomputed
    (0, 1, [1] * 8, True),        # (a budget below one seed counts as one)
    (0, 2, [8], False),
])
def test_the_stage_budget_decides_where_no_debug_knob_does(fit, min_piece, counts, keep):
    # `fit` whole seeds and most of another: the quotient is rounded down
    budget = fit * PER_SEED + PER_SEED - 1 if fit else PER_SEED // 2
    got, sized_for = pieces(True, False, (0, min_piece, 0), 8, stage_budget=budget)
    print(fit, min_piece, "->", got, sized_for)
    assert got == listed(counts, keep, False)
    assert sized_for == (counts[0] if keep else 0)


def test_bad_arguments_are_refused():
    lib = engine.load_library()
    buf, found, sized_for = (ctypes.c_int32 * 8)(), ctypes.c_int32(0), ctypes.c_int64(0)
    null, null64 = ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_int64)()
    good = [1, 1, 0, 0, 256, 0, 4, 8, PER_SEED, 8, buf, buf, buf, ctypes.byref(found), ctypes.byref(sized_for)]
    assert lib.qocx_debug_lindblad_pieces(*good) == 0
    for at, bad in ((3, -1), (4, 0), (5, 3), (6, 0), (7, 0), (8, 0), (10, null), (13, null), (14, null64)):
        args = list(good)
        args[at] = bad
        assert lib.qocx_debug_lindblad_pieces(*args) != 0, at
