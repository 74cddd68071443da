// qocx_lindblad_route.h - which kernel a Lindblad launch takes, whether an evaluation runs two-sided, and the
// piece schedule: pure functions of plain facts. Host only, no HIP call; qocx_api_lindblad.hip fills the
// facts from its context (lindblad_facts), stores the form when a problem is set and computes the route once
// per evaluation; the launchers of qocx_lindblad*.hip switch on the kernel value and decide nothing.
// qocx_debug_lindblad_route / qocx_debug_lindblad_pieces (include/qocx.h) run the same functions without a
// context (tests/test_lindblad_route_host.py, tests/test_lindblad_pieces_host.py).
#ifndef QOCX_LINDBLAD_ROUTE_H
#define QOCX_LINDBLAD_ROUTE_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/qocx.h"

namespace qocx {

using LindbladFacts = qocx_lindblad_facts;  // include/qocx.h

// One enumerator per instantiation a Lindblad launch can take (the values of qocx_debug_lindblad_route); with
// per-member rates the same value names the twin of qocx_lindblad_rates.hip / qocx_lindblad4t_rates.hip.
enum class LindbladKernel : int {
    NONE,              // no kernel takes the problem
    ONE_WAVE_LDS,      // n <= 16, one wave per seed, everything in LDS: lindblad_kernel<1, false, false, false>
    ONE_WAVE_SCRATCH,  // ... densities, cotangents and stage derivatives in HBM scratch: <1, true, false, false>
    ONE_WAVE_32,       // 17 <= n <= 32, four tiles per matrix in one wave: LB<2, true, false>
    WAVES_NOPS2,       // n <= 16, nops + 2 waves per seed: <1, false, true, false>
    FOUR_WAVES,        // ... two operators, a wave per SIMD, the quarter-split stage loops: <1, false, true, true>
    FOUR_WAVES_Q2,     // ... the stage loop of the two-sided launches (substep_q2): <..., true, false, true>
    FOUR_WAVES_CHAIN,  // ... its chain form, two to four operators (substep_chain): <..., true, false, true, true>
    TILE4,             // 17 <= n <= 32, a tile per wave: lindblad4t_kernel<false> (qocx_lindblad4t.hip)
    TILE4_HERM,        // ... on Hermitian densities and cotangents: lindblad4t_kernel<true>
    TILE16             // 33 <= n <= 64: lindblad16t_kernel (qocx_lindblad16t.hip)
};

constexpr int LINDBLAD_LDS_LIMIT = 160 * 1024;  // bytes of LDS a workgroup may ask for
constexpr int LINDBLAD_MAX_CONTROLS = 8;        // QOCX_LINDBLAD_MAX_K (qocx_device.h)
constexpr int LINDBLAD_WAVES_MAX_OPS = 4;       // the several-wave stage loops of the one-tile engine
constexpr int LINDBLAD_TILE4_MAX_OPS = 4;       // the tile-per-wave kernel holds them in LDS (lindblad4t::MAX_OPS)
constexpr int LINDBLAD_TILE16_MAX_OPS = 8;      // the sixteen-wave kernel reads them from memory (lindblad16t::MAX_OPS)

// The launch form of a problem, decided when it is set and stored (qocx_ctx::Lindblad::form): pad_op has
// shaped the uploaded tables by then, and its knob may change afterwards.
struct LindbladForm {
    int scratch = 0;     // densities, cotangents and stage derivatives in per-seed HBM scratch, not in LDS
    int pad_op = 0;      // L = 1: a zero second operator behind the real one, for the four-wave launches
    int multi_wave = 0;  // the several-wave layout fits LDS
    int cache_gen = 0;   // ... with the constant generator dumps of the K controls beside it
};

// `lds(mode, nops)`: LDS bytes of one seed of the problem (lindblad_lds_size at its n, S, K). Reads n, nops,
// stage_tables, op_tables, lindblad_pad_operator and single_wave of the facts.
template <class Lds>
LindbladForm lindblad_form(const LindbladFacts& f, const Lds& lds) {
    LindbladForm m;
    const int L = f.nops;
    // densities, cotangents and stage derivatives live in LDS when they fit (n <= 16), else in per-seed HBM scratch
    m.scratch = (f.n > 16 || lds(0, L) > LINDBLAD_LDS_LIMIT) ? 1 : 0;
    // several waves per seed (generator terms | one per operator | control cotangents) whenever
    // that layout fits LDS: the recursion in time is serial, this shortens every stage
    // (ONE operator - the T1 problem - runs the several-wave launches as two, the second one zero: the
    // four-wave stage loops of section 14 exist for L = 2 only and are 1.5 times faster than the three-wave
    // form of L = 1 although they multiply by that zero: 17.2 -> 11.5 ms on configs[3]'s sizes)
    m.pad_op = (L == 1 && f.n <= 16 && !f.op_tables && f.lindblad_pad_operator != 0) ? 1 : 0;
    const int Lmw = m.pad_op ? 2 : L;
    m.multi_wave = (!m.scratch && L > 0 && L <= LINDBLAD_WAVES_MAX_OPS && lds(2, Lmw) <= LINDBLAD_LDS_LIMIT &&
                    !f.single_wave) ? 1 : 0;
    m.cache_gen = (m.multi_wave && !f.stage_tables && lds(3, Lmw) <= LINDBLAD_LDS_LIMIT) ? 1 : 0;
    return m;
}

// What an evaluation launches, piece by piece: a piece runs two-sided - forward launch (phase 1) beside the
// adjoint launch on the target (phase 2), then the combine kernel - where the route says so and the piece
// keeps its stage values (lindblad_group_pieces); every other piece is one classic launch (phase 0).
struct LindbladRoute {
    LindbladKernel kernel[3] = {LindbladKernel::NONE, LindbladKernel::NONE, LindbladKernel::NONE};  // by phase
    bool multi_wave = false;  // pieces run several waves per seed (LindbladArgs::multi_wave; nops with pad_op's zero)
    bool two_sided = false;
    bool rate_sens = false;   // the evaluation delivers rate sensitivities if every piece keeps its stage values
    bool stamps = false;      // knob lindblad_stamps: the launches get a stamp buffer ...
    bool stamped = false;     // ... and, diagnostic library only, the four-wave kernels run in their stamped builds
    int tile4 = 0, hermitian = 0, q2 = 0, chain = 0, ops_real = 0;  // LindbladArgs' flags of those names
    int side_limit = 0;       // up to this many seeds a two-sided piece's adjoint launch takes the side stream
};

inline LindbladRoute lindblad_route(const LindbladForm& m, const LindbladFacts& f) {
    typedef LindbladKernel LK;
    LindbladRoute r;
    const int n = f.n, L = f.nops;
    r.multi_wave = m.multi_wave && f.dbg_wave_mode != 1;
    r.tile4 = f.lindblad_4t != 0 ? 1 : 0;
    // (cotangents from the host need not be Hermitian; stage tables: the problem setter clears `hermitian`)
    r.hermitian = (f.hermitian && f.inj_count == 0 && f.lindblad_hermitian != 0) ? 1 : 0;
    r.q2 = f.lindblad_q2 != 0 ? 1 : 0;
    r.chain = f.lindblad_chain != 0 ? 1 : 0;
    r.ops_real = (f.ops_real && f.lindblad_real_ops != 0) ? 1 : 0;
    r.side_limit = f.lindblad_side_limit;
    const bool controls_ok = f.K <= LINDBLAD_MAX_CONTROLS;
    // 17 <= n <= 32: the tile-per-wave kernel (knob lindblad_4t; its Hermitian build reads constant generators
    // and no host cotangents), else the one-wave form; it alone knows the phases above one tile
    const bool tile4 = n > 16 && n <= 32 && r.tile4 && L <= LINDBLAD_TILE4_MAX_OPS && controls_ok &&
                       (!r.hermitian || (!f.stage_tables && f.inj_count == 0));
    // the operators of a several-wave launch, with the zero one of pad_op
    const int Lw = (r.multi_wave && m.pad_op) ? 2 : L;
    if (n > 32)  // the sixteen-wave kernel: static problems, the classic launch only
        r.kernel[0] = (n <= 64 && !f.stage_tables && !f.g_tables && !f.op_tables && L <= LINDBLAD_TILE16_MAX_OPS &&
                       controls_ok) ? LK::TILE16 : LK::NONE;
    else if (n > 16) r.kernel[0] = tile4 ? (r.hermitian ? LK::TILE4_HERM : LK::TILE4) : LK::ONE_WAVE_32;
    else if (m.scratch) r.kernel[0] = LK::ONE_WAVE_SCRATCH;
    else if (!r.multi_wave) r.kernel[0] = LK::ONE_WAVE_LDS;
    else r.kernel[0] = Lw == 2 ? LK::FOUR_WAVES : LK::WAVES_NOPS2;
    // Two-sided evaluation (LindbladArgs::phase): ONE final target-density cost and no host cotangents - the
    // adjoint then runs on the target beside the forward pass -, gradients, constant tables, a side stream, and
    // kernels that know the phases: the several-wave launches of one tile, the tile-per-wave kernel above
    // (n > 32: never - the kernel of qocx_lindblad16t.hip knows the classic launch only)
    const bool phases = n <= 16 ? (L >= 1 && r.multi_wave && !m.scratch) : (n <= 32 && tile4);
    r.two_sided = f.want_grad && f.unit_ok && f.inj_count == 0 && phases && !f.stage_tables &&
                  f.side_streams >= 1 && f.lindblad_two_sided != 0;
    if (r.two_sided) {
        // the stage loop of the two-sided launches (knob lindblad_q2: constant H0 / G_k, stage values kept, up to
        // four controls) and its chain form (knob lindblad_chain); else the loops of the classic launch
        const bool q2 = r.q2 && f.K <= 4;
        r.kernel[1] = n > 16                             ? r.kernel[0]
                      : q2 && r.chain && Lw >= 2         ? LK::FOUR_WAVES_CHAIN
                      : q2 && Lw == 2                    ? LK::FOUR_WAVES_Q2
                                                         : r.kernel[0];
        r.kernel[2] = r.kernel[1];
    }
    // Rate sensitivities of a sweep (qocx_lindblad_ratesens.hip): a launch behind every piece's combine launch
    r.rate_sens = f.sweep && f.want_rate_sens && f.want_grad && L >= 1 && L <= 4 && r.two_sided;
    r.stamps = f.lindblad_stamps != 0;
    r.stamped = r.stamps && Lw == 2;
    return r;
}

// One piece of an evaluation - one launch, or the three of a two-sided piece: `count` seeds of the group
// with sub-division count `ksub`, from position `first` of the launch order (lb.order).
struct LindbladPiece {
    int ksub = 0, first = 0, count = 0;
    // the forward pass keeps its stage values for the adjoint (else: recomputed); several waves per seed
    bool keep_stages = false, multi_wave = false;
};

// What decides the schedule: the stage budget (double2 elements), the record's debug knobs, the launch form
struct PieceRule {
    bool want_grad = false, multi_wave = false;
    size_t stage_budget = 0;
    int64_t dbg_stage_seeds = 0;
    int dbg_min_piece = 256, dbg_wave_mode = 0, cu_count = 1;
};

// THE schedule (plain C++ over integers), for one group of `Bg` seeds from position `first`, `per_seed` stage
// elements each; its pieces are appended in launch order. The stage values of the forward pass are kept for
// the adjoint (12 x the checkpoints of the seeds in flight); a group that does not fit goes in pieces that do,
// and only if a piece would fall below dbg_min_piece seeds does the adjoint recompute them instead (one piece,
// as without gradients). Several waves per seed whenever the kernel is built for the problem; batches beyond
// the CU count then go in rounds of one seed per CU. (Round 1 switched to one wave per seed, two seeds per CU,
// beyond 256 seeds; on configs[3] at 300 / 512 / 768 / 1024 seeds: 73.7 / 80.7 / 126.6 / 123.7 ms against 74.4 /
// 76.6 / 82.7 / 104.8 ms in rounds.) Returns the seeds the stage buffers are sized for: the kept piece BEFORE
// the round cap (0: none kept), which over-provisions a capped group: the footprint of old.
inline size_t lindblad_group_pieces(const PieceRule& r, int ksub, int first, int Bg, size_t per_seed,
                                    std::vector<LindbladPiece>& out) {
    int piece = Bg;
    bool keep = false;
    if (r.want_grad) {
        const size_t fit = r.dbg_stage_seeds > 0 ? (size_t)r.dbg_stage_seeds
                                                 : std::max<size_t>(1, r.stage_budget / per_seed);
        if (fit >= (size_t)Bg) { keep = true; }
        else if (fit >= (size_t)r.dbg_min_piece) { keep = true; piece = (int)fit; }
    }
    const size_t sized_for = keep ? (size_t)piece : 0;
    const bool multi = r.multi_wave && r.dbg_wave_mode != 1;
    if (multi && r.dbg_wave_mode != 2) piece = std::min(piece, r.cu_count);
    for (int p0 = 0; p0 < Bg; p0 += piece) out.push_back({ksub, first + p0, std::min(piece, Bg - p0), keep, multi});
    return sized_for;
}

}  // namespace qocx

#endif
