"""
CPU test of the route decision of the matrix-free route (qoc_amd/csrc/qocx_action_route.h: action_plan),
through the library's context-free debug entry qocx_debug_action_route (no GPU call): a table of literal
rows - the base facts with one or two fields changed, and the kernel family and step table the knob
documentation of include/qocx.h says they take. No Python copy of the predicate: a row that disagrees
with the library is a finding about one of the two.

(The plan's channel count - Ke on effective controls, else K - is not among the entry's outputs; the GPU
tests of the effective-control route, tests/test_gpu_action_effective.py, depend on it.)
"""

import ctypes
import math

import pytest

from qoc_amd import engine

NONE, N32, N32_EFF_EXACT, STATES, COSTS, N16, N64 = range(7)  # *kernel of qocx_debug_action_route
PLAIN, EFF = 0, 1                                             # *table
THETA_18 = 1.09                                               # qocx_action.h: action_theta(18)

# 17 <= n <= 32, one state, two controls, structured M2 on a time-independent Hermitian system, one final
# TargetStateInfidelity, everything on the device, every knob at its default: the headline's route
BASE = dict(
    n=32, S=1, K=2, nt=1, nodes=1, eff_kind=0, Ke=0, hermitian=1, unit_ok=1, has_step_costs=0, cost_count=1,
    inj_count=0, keep_step_states=0, explicit_gen=0, dense=0, one_wave_k1a=0, latency=0,
    have_norms=1, have_eff_norms=1, have_e_img=1,
    bound1=0.3, bound1_mid=0.3, bound2=0.2, bound2_mid=0.2,
    action=1, action_states=0, action_costs=0, action_small=0, action_eff=0, action_eff_exact=1,
    action_degree=1, action_plan=1, pade_order=0, unit_adjoint=1, allow=1)
M4 = dict(eff_kind=1, Ke=5)      # M4-linear with two controls: v_k, w_k and one z_kl
QUAD = dict(eff_kind=2, Ke=3)    # two controls and one quadratic term


def route(**changes):
    """(kernel, table, m_max) of BASE with `changes`; a changed bound moves its midpoint twin along."""
    values = dict(BASE)
    for name in ("bound1", "bound2"):
        if name in changes and name + "_mid" not in changes:
            values[name + "_mid"] = changes[name]
    values.update(changes)
    assert set(values) == set(BASE)
    facts = engine.ActionFacts(**values)
    kernel, table, m_max = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = engine.load_library().qocx_debug_action_route(
        ctypes.byref(facts), ctypes.byref(kernel), ctypes.byref(table), ctypes.byref(m_max))
    assert rc == 0
    return kernel.value, table.value, m_max.value


def rows():
    out = []

    def row(name, kernel, table=PLAIN, **changes):
        out.append(pytest.param(changes, kernel, table, id=name))

    row("base", N32)
    # sizes
    row("n16", NONE, n=16)
    row("n17", N32, n=17)
    row("n33", NONE, n=33)
    row("n64", NONE, n=64)
    row("n1 small", N16, n=1, action_small=1)
    row("n3 small", N16, n=3, action_small=1)
    row("n16 small", N16, n=16, action_small=1)
    row("n8 small without action", N16, n=8, action=0, action_small=1)
    row("n20 small", N32, n=20, action_small=1)  # (no effect above n = 16)
    row("n33 wide", N64, n=33, action=2)
    row("n48 wide", N64, n=48, action=2)
    row("n64 wide", N64, n=64, action=2)
    row("n65 wide", NONE, n=65, action=2)
    row("n32 wide", N32, action=2)
    row("n16 wide", NONE, n=16, action=2)
    row("n33 action 1", NONE, n=33, action=1)
    row("n32 action 0", NONE, action=0)
    # states
    row("S2", NONE, S=2)
    row("S2 states 4", STATES, S=2, action_states=4)
    row("S4 states 4", STATES, S=4, action_states=4)
    row("S2 states 2", STATES, S=2, action_states=2)
    row("S3 states 2", NONE, S=3, action_states=2)
    row("S1 states 4", N32, action_states=4)
    row("S2 n16 small", NONE, S=2, n=16, action_small=1, action_states=4)
    row("S2 n48 wide", NONE, S=2, n=48, action=2, action_states=4)
    # costs
    row("not unit_ok", NONE, unit_ok=0)
    row("not unit_ok costs", COSTS, unit_ok=0, action_costs=1)
    row("step costs costs", COSTS, unit_ok=0, has_step_costs=1, cost_count=2, action_costs=1)
    row("no cost costs", NONE, unit_ok=0, cost_count=0, action_costs=1)
    row("n16 costs", NONE, unit_ok=0, action_costs=1, n=16, action_small=1)
    row("n48 costs", NONE, unit_ok=0, action_costs=1, n=48, action=2)
    row("S2 costs", NONE, unit_ok=0, action_costs=1, S=2, action_states=4)
    row("unit_ok costs", N32, action_costs=1)
    row("unit_ok step costs costs", NONE, has_step_costs=1, action_costs=1)
    row("unit_ok step costs", NONE, has_step_costs=1)
    row("no unit adjoint", NONE, unit_adjoint=0)
    # every single yield
    row("time-dependent system", NONE, nt=2)
    row("non-Hermitian", NONE, hermitian=0)
    row("state cotangents", NONE, inj_count=1)
    row("latency", NONE, latency=1)
    row("kept step states", NONE, keep_step_states=1)
    row("pade_order 13", NONE, pade_order=13)
    row("explicit generators", NONE, explicit_gen=1)
    row("two nodes", NONE, nodes=2)
    row("no controls", NONE, K=0)
    row("no operand norms", NONE, have_norms=0)
    row("dense sweep", NONE, dense=1)
    row("rerun", NONE, allow=0)
    row("no E image, plain", N32, have_e_img=0)  # (not a yield: the evaluation fails where it wants a gradient)
    # the 1-norm bound alone admits, equality included; the lesser of knots and midpoints counts
    row("bound at theta_18", N32, bound1=THETA_18)
    row("bound above theta_18", NONE, bound1=math.nextafter(THETA_18, 2.0))
    row("bound NaN", NONE, bound1=math.nan)
    row("bound infinite", NONE, bound1=math.inf)
    row("midpoint bound admits", N32, bound1=2.0, bound1_mid=0.3)
    row("knot bound admits", N32, bound1=0.3, bound1_mid=2.0)
    row("spectral bound does not decide", N32, bound2=5.0)
    row("spectral bound NaN does not decide", N32, bound2=math.nan)
    # effective controls
    row("M4", NONE, **M4)
    row("M4 eff", N32_EFF_EXACT, EFF, action_eff=1, **M4)
    row("M4 eff streamed", N32, EFF, action_eff=1, action_eff_exact=0, **M4)
    row("M4 Ke 2 eff", N32, EFF, action_eff=1, eff_kind=1, Ke=2, K=1)
    row("quadratic", NONE, **QUAD)
    row("quadratic eff", N32, EFF, action_eff=1, **QUAD)
    row("quadratic Ke 5 eff", N32_EFF_EXACT, EFF, action_eff=1, eff_kind=2, Ke=5)  # (the register build asks for Ke alone)
    row("M4 eff action 0", NONE, action_eff=1, action=0, **M4)
    row("M4 eff n8", NONE, action_eff=1, n=8, **M4)
    row("M4 eff n8 small", N16, EFF, action_eff=1, n=8, action_small=1, **M4)
    row("M4 eff n48", NONE, action_eff=1, n=48, **M4)
    row("M4 eff n48 wide", N64, EFF, action_eff=1, n=48, action=2, **M4)
    row("M4 eff S2", NONE, action_eff=1, S=2, action_states=4, **M4)
    row("M4 eff costs", NONE, action_eff=1, unit_ok=0, action_costs=1, **M4)
    row("M4 eff no norms", NONE, action_eff=1, have_eff_norms=0, **M4)
    row("M4 eff no operand norms", N32_EFF_EXACT, EFF, action_eff=1, have_norms=0, **M4)  # (its table reads its own)
    row("M4 eff no E image", NONE, action_eff=1, have_e_img=0, **M4)
    row("M4 eff n8 no E image", NONE, action_eff=1, have_e_img=0, n=8, action_small=1, **M4)
    row("M4 eff n48 no E image", N64, EFF, action_eff=1, have_e_img=0, n=48, action=2, **M4)
    row("M4 eff latency", NONE, action_eff=1, latency=1, **M4)
    return out


@pytest.mark.parametrize("changes,kernel,table", rows())
def test_route_table(changes, kernel, table):
    got_kernel, got_table, m_max = route(**changes)
    print(changes, "->", got_kernel, got_table, m_max)
    assert (got_kernel, got_table) == (kernel, table)
    assert (m_max == 0) == (kernel == NONE)


def native_degree(bound1, bound2, rule):
    out = ctypes.c_int32(-1)
    assert engine.load_library().qocx_debug_action_degree(float(bound1), float(bound2), rule,
                                                          ctypes.byref(out)) == 0
    return out.value


@pytest.mark.parametrize("rule", (0, 1))
def test_buffers_follow_the_degree_rule_on_the_bounds_with_their_margin(rule):
    """m_max: action_degree_rule on the host's two bounds times (1 + 1e-9), at most 18 - for every table."""
    taken = (dict(), dict(n=8, action_small=1), dict(n=48, action=2), dict(S=2, action_states=2),
             dict(unit_ok=0, action_costs=1), dict(action_eff=1, **M4), dict(action_eff=1, **QUAD))
    bounds = ((0.3, 0.2), (0.3, 0.3), (0.3, 0.01), (0.05, 0.05), (2.4e-3, 2.4e-3), (1.0, 0.9),
              (THETA_18, 0.2), (THETA_18, THETA_18), (0.5, math.nan))
    for changes in taken:
        for b1, b2 in bounds:
            kernel, _, m_max = route(bound1=b1, bound2=b2, action_degree=rule, **changes)
            want = min(18, native_degree(b1 * (1 + 1e-9), b2 * (1 + 1e-9), rule))
            assert kernel != NONE and m_max == want, (changes, b1, b2, rule, m_max, want)
    # (the lesser of the bounds over the knots and at the midpoints, for each norm)
    _, _, m_max = route(bound1=0.9, bound1_mid=0.3, bound2=0.2, bound2_mid=0.8, action_degree=rule)
    assert m_max == native_degree(0.3 * (1 + 1e-9), 0.2 * (1 + 1e-9), rule)


def test_the_facts_are_the_struct_of_the_header_and_null_arguments_are_refused():
    # 20 flags and counts, four doubles, ten knob values and `allow`, padded to 8 (include/qocx.h: qocx_action_facts)
    assert ctypes.sizeof(engine.ActionFacts) == 20 * 4 + 4 * 8 + 11 * 4 + 4
    assert [name for name, _ in engine.ActionFacts._fields_] == list(BASE)
    lib = engine.load_library()
    facts, out = engine.ActionFacts(**BASE), ctypes.c_int32(0)
    null = ctypes.POINTER(ctypes.c_int32)()
    assert lib.qocx_debug_action_route(None, ctypes.byref(out), ctypes.byref(out), ctypes.byref(out)) != 0
    assert lib.qocx_debug_action_route(ctypes.byref(facts), null, ctypes.byref(out), ctypes.byref(out)) != 0
