"""
CPU test of the kernel choice of the Lindblad path (qoc_amd/csrc/qocx_lindblad_route.h: lindblad_form,
lindblad_route), through the library's context-free debug entry qocx_debug_lindblad_route (no GPU call): a
table of literal rows - the base facts with one or two fields changed, and the kernels of the classic, the
forward and the adjoint launch they take. No Python copy of the predicate: a row that disagrees with the
library is a finding about one of the two.

(The route's flag values for LindbladArgs - hermitian, q2, chain, ops_real, side_limit - are not among the
entry's outputs; tests/test_gpu_lindblad.py holds the kernels they select against each other.)
"""

import ctypes

import pytest

from qoc_amd import engine

# kernels[] of qocx_debug_lindblad_route
(NONE, ONE_WAVE_LDS, ONE_WAVE_SCRATCH, ONE_WAVE_32, WAVES_NOPS2, FOUR_WAVES, FOUR_WAVES_Q2, FOUR_WAVES_CHAIN,
 TILE4, TILE4_HERM, TILE16) = range(11)

# n = 4, one density, two controls, two operators, static, one final target-density cost, gradients, no host
# cotangents, one side stream, every knob at its default (lindblad_side_limit: half of 256 CUs)
BASE = dict(
    n=4, S=1, K=2, nops=2, stage_tables=0, g_tables=0, op_tables=0, hermitian=1, ops_real=1, unit_ok=1,
    inj_count=0, want_grad=1, rates=0, sweep=0, want_rate_sens=0, side_streams=1, cu_count=256,
    dbg_wave_mode=0, lindblad_4t=1, lindblad_two_sided=1, lindblad_hermitian=1, lindblad_q2=1,
    lindblad_chain=1, lindblad_real_ops=1, lindblad_pad_operator=1, lindblad_side_limit=128,
    lindblad_stamps=0, single_wave=0)
STAGE_TABLES = dict(stage_tables=1, hermitian=0)   # (the problem setter calls no problem with tables Hermitian)
SENS = dict(sweep=1, want_rate_sens=1)             # a sweep that asked for its rate sensitivities


def route(**changes):
    values = dict(BASE)
    values.update(changes)
    assert set(values) == set(BASE)
    facts = engine.LindbladFacts(**values)
    kernels, form = (ctypes.c_int32 * 3)(-1, -1, -1), (ctypes.c_int32 * 4)(-1, -1, -1, -1)
    multi_wave, two_sided, rate_sens = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = engine.load_library().qocx_debug_lindblad_route(
        ctypes.byref(facts), kernels, ctypes.byref(multi_wave), ctypes.byref(two_sided), ctypes.byref(rate_sens),
        form)
    assert rc == 0
    return dict(kernels=tuple(kernels), multi_wave=multi_wave.value, two_sided=two_sided.value,
                rate_sens=rate_sens.value, scratch=form[0], pad_op=form[1], form_multi_wave=form[2],
                cache_gen=form[3])


def rows():
    out = []

    def row(name, classic, sided=None, changes=None, **outputs):
        """`sided`: the kernel of the forward and of the adjoint launch; None: the route is not two-sided.
        `outputs`: further outputs of the entry the row pins."""
        out.append(pytest.param(changes or {}, classic, sided, outputs, id=name))

    # ---- one tile, several waves ----
    # (cache_gen: the generator dumps of K = 2 controls do not fit beside four waves' slots; those of one do)
    row("base", FOUR_WAVES, FOUR_WAVES_CHAIN, multi_wave=1, scratch=0, pad_op=0, form_multi_wave=1, cache_gen=0)
    row("K1", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(K=1), cache_gen=1)
    row("K0", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(K=0), cache_gen=1)
    row("K4", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(K=4))
    row("K5", FOUR_WAVES, FOUR_WAVES, dict(K=5))          # q2 needs K <= 4
    row("K8", FOUR_WAVES, FOUR_WAVES, dict(K=8))
    row("chain 0", FOUR_WAVES, FOUR_WAVES_Q2, dict(lindblad_chain=0))
    row("chain 0 L3", WAVES_NOPS2, WAVES_NOPS2, dict(lindblad_chain=0, nops=3))
    row("q2 0", FOUR_WAVES, FOUR_WAVES, dict(lindblad_q2=0))
    row("q2 0 L3", WAVES_NOPS2, WAVES_NOPS2, dict(lindblad_q2=0, nops=3))
    row("L1", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(nops=1), pad_op=1, multi_wave=1)
    row("L1 K1", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(nops=1, K=1), pad_op=1, cache_gen=1)
    row("L1 chain 0", FOUR_WAVES, FOUR_WAVES_Q2, dict(nops=1, lindblad_chain=0), pad_op=1)
    row("L1 no pad", WAVES_NOPS2, WAVES_NOPS2, dict(nops=1, lindblad_pad_operator=0), pad_op=0, multi_wave=1)
    row("L1 operator tables", WAVES_NOPS2, None, dict(nops=1, op_tables=1, **STAGE_TABLES), pad_op=0)
    row("L3", WAVES_NOPS2, FOUR_WAVES_CHAIN, dict(nops=3), multi_wave=1)
    row("L4", WAVES_NOPS2, FOUR_WAVES_CHAIN, dict(nops=4), multi_wave=1)
    row("n1", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(n=1))
    row("n16", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(n=16), scratch=0)
    row("not Hermitian", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(hermitian=0))   # (a flag of the launch, no kernel)
    row("stamps", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(lindblad_stamps=1))    # (the product library has no stamped build)
    row("wave mode 2", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(dbg_wave_mode=2), multi_wave=1)
    # ---- one tile, one wave ----
    row("L0", ONE_WAVE_LDS, None, dict(nops=0), multi_wave=0, form_multi_wave=0, scratch=0)
    row("L5", ONE_WAVE_LDS, None, dict(nops=5), multi_wave=0, form_multi_wave=0, scratch=0)
    row("L8", ONE_WAVE_LDS, None, dict(nops=8), multi_wave=0)
    row("S8", ONE_WAVE_LDS, None, dict(S=8), form_multi_wave=0, scratch=0)   # one wave fits LDS, four do not
    row("S16", ONE_WAVE_SCRATCH, None, dict(S=16), scratch=1, form_multi_wave=0)  # 44 dumps of 4 KiB > 160 KiB
    row("S64", ONE_WAVE_SCRATCH, None, dict(S=64), scratch=1)
    row("wave mode 1", ONE_WAVE_LDS, None, dict(dbg_wave_mode=1), multi_wave=0, form_multi_wave=1)
    row("wave mode 1 L1", ONE_WAVE_LDS, None, dict(dbg_wave_mode=1, nops=1), multi_wave=0, pad_op=1)
    row("single wave", ONE_WAVE_LDS, None, dict(single_wave=1), multi_wave=0, form_multi_wave=0, cache_gen=0)
    # ---- two-sided switched off: the classic kernel stays ----
    row("not unit_ok", FOUR_WAVES, None, dict(unit_ok=0))
    row("density cotangents", FOUR_WAVES, None, dict(inj_count=1))
    row("no gradients", FOUR_WAVES, None, dict(want_grad=0))
    row("two_sided 0", FOUR_WAVES, None, dict(lindblad_two_sided=0))
    row("stage tables", FOUR_WAVES, None, STAGE_TABLES, cache_gen=0)
    row("stage tables K1", FOUR_WAVES, None, dict(K=1, **STAGE_TABLES), cache_gen=0)
    row("no side stream", FOUR_WAVES, None, dict(side_streams=0))
    # ---- 17 <= n <= 32 ----
    for n in (17, 20, 32):
        tag = "n%d " % n
        row(tag + "Hermitian", TILE4_HERM, TILE4_HERM, dict(n=n), multi_wave=0, scratch=1, pad_op=0)
        row(tag + "L0", TILE4_HERM, TILE4_HERM, dict(n=n, nops=0))
        row(tag + "L1", TILE4_HERM, TILE4_HERM, dict(n=n, nops=1), pad_op=0)
        row(tag + "L4", TILE4_HERM, TILE4_HERM, dict(n=n, nops=4))
        row(tag + "not Hermitian", TILE4, TILE4, dict(n=n, hermitian=0))
        row(tag + "density cotangents", TILE4, None, dict(n=n, inj_count=2))
        row(tag + "hermitian 0", TILE4, TILE4, dict(n=n, lindblad_hermitian=0))
        row(tag + "L5", ONE_WAVE_32, None, dict(n=n, nops=5))
        row(tag + "4t 0", ONE_WAVE_32, None, dict(n=n, lindblad_4t=0))
        row(tag + "stage tables", TILE4, None, dict(n=n, **STAGE_TABLES))
        row(tag + "no gradients", TILE4_HERM, None, dict(n=n, want_grad=0))
        row(tag + "two_sided 0", TILE4_HERM, None, dict(n=n, lindblad_two_sided=0))
        row(tag + "not unit_ok", TILE4_HERM, None, dict(n=n, unit_ok=0))
        row(tag + "wave mode 1", TILE4_HERM, TILE4_HERM, dict(n=n, dbg_wave_mode=1))  # (one tile's switch)
        row(tag + "K5", TILE4_HERM, TILE4_HERM, dict(n=n, K=5))
    # ---- 33 <= n <= 64: the classic launch of static problems ----
    for n in (33, 64):
        for L in range(9):
            row("n%d L%d" % (n, L), TILE16, None, dict(n=n, nops=L), multi_wave=0, scratch=1, rate_sens=0)
        row("n%d sweep" % n, TILE16, None, dict(n=n, **SENS), rate_sens=0)
        row("n%d stage tables" % n, NONE, None, dict(n=n, **STAGE_TABLES))
        row("n%d L9" % n, NONE, None, dict(n=n, nops=9))
        row("n%d no gradients" % n, TILE16, None, dict(n=n, want_grad=0))
    row("n65", NONE, None, dict(n=65))
    # ---- rates change no kernel ----
    row("rates", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(rates=1))
    row("rates L1", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(rates=1, nops=1))
    row("rates wave mode 1", ONE_WAVE_LDS, None, dict(rates=1, dbg_wave_mode=1))
    row("rates n20", TILE4_HERM, TILE4_HERM, dict(rates=1, n=20))
    row("rates n20 L5", ONE_WAVE_32, None, dict(rates=1, n=20, nops=5))
    # ---- rate sensitivities: a sweep that wants them, gradients, 1 .. 4 operators, two-sided ----
    row("sens", FOUR_WAVES, FOUR_WAVES_CHAIN, SENS, rate_sens=1)
    row("sens L1", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(nops=1, **SENS), rate_sens=1)
    row("sens L4", WAVES_NOPS2, FOUR_WAVES_CHAIN, dict(nops=4, **SENS), rate_sens=1)
    row("sens n20", TILE4_HERM, TILE4_HERM, dict(n=20, **SENS), rate_sens=1)
    row("sens no sweep", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(sweep=0, want_rate_sens=1), rate_sens=0)
    row("sens not wanted", FOUR_WAVES, FOUR_WAVES_CHAIN, dict(sweep=1, want_rate_sens=0), rate_sens=0)
    row("sens no gradients", FOUR_WAVES, None, dict(want_grad=0, **SENS), rate_sens=0)
    row("sens L0", ONE_WAVE_LDS, None, dict(nops=0, **SENS), rate_sens=0)
    row("sens n20 L0", TILE4_HERM, TILE4_HERM, dict(n=20, nops=0, **SENS), rate_sens=0)
    row("sens L5", ONE_WAVE_LDS, None, dict(nops=5, **SENS), rate_sens=0)
    row("sens not two-sided", FOUR_WAVES, None, dict(lindblad_two_sided=0, **SENS), rate_sens=0)
    row("sens not unit_ok", FOUR_WAVES, None, dict(unit_ok=0, **SENS), rate_sens=0)
    return out


@pytest.mark.parametrize("changes,classic,sided,outputs", rows())
def test_route_table(changes, classic, sided, outputs):
    got = route(**changes)
    print(changes, "->", got)
    assert got["kernels"] == (classic, sided or NONE, sided or NONE)
    assert got["two_sided"] == (1 if sided is not None else 0)
    for name, value in outputs.items():
        assert got[name] == value, name
    if "rate_sens" not in outputs:
        assert got["rate_sens"] == 0


def test_the_facts_are_the_struct_of_the_header_and_null_arguments_are_refused():
    import os
    import re
    # 28 flags, counts and knob values (include/qocx.h: qocx_lindblad_facts)
    assert ctypes.sizeof(engine.LindbladFacts) == 28 * 4
    names = [name for name, _ in engine.LindbladFacts._fields_]
    assert names == list(BASE)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "qocx.h")).read(), flags=re.S)
    body = re.search(r"typedef struct qocx_lindblad_facts \{(.*?)\} qocx_lindblad_facts;", text, flags=re.S).group(1)
    declared = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            assert decl.startswith("int32_t "), decl
            declared += [name.strip() for name in decl[len("int32_t "):].split(",")]
    assert declared == names
    lib = engine.load_library()
    facts, out = engine.LindbladFacts(**BASE), (ctypes.c_int32 * 4)()
    one = ctypes.c_int32(0)
    null = ctypes.POINTER(ctypes.c_int32)()
    good = [ctypes.byref(facts), out, ctypes.byref(one), ctypes.byref(one), ctypes.byref(one), out]
    assert lib.qocx_debug_lindblad_route(*good) == 0
    for at in range(len(good)):
        args = list(good)
        args[at] = None if at == 0 else null
        assert lib.qocx_debug_lindblad_route(*args) != 0, at
