// qocx_action_route.h - whether an evaluation takes the matrix-free route (truncated Taylor sweeps,
// nothing factored) and which of its kernel families runs it: a pure function of plain facts. Host
// only, no HIP call; qocx_host_resident.hip fills the facts from its context once per evaluation,
// qocx_debug_action_route (include/qocx.h) runs the same function without one
// (tests/test_action_route_host.py).
#ifndef QOCX_ACTION_ROUTE_H
#define QOCX_ACTION_ROUTE_H

#include <algorithm>

#include "../../include/qocx.h"
#include "qocx_action.h"

namespace qocx {

bool action_eff_exact_supports(int Ke);  // qocx_action_eff.hip: the control counts its register build exists for

using ActionFacts = qocx_action_facts;  // include/qocx.h

struct ActionPlan {
    // (the values of qocx_debug_action_route)
    enum Kernel {
        NONE,           // the Pade route
        N32,            // 17 <= n <= 32, one state (qocx_action.hip)
        N32_EFF_EXACT,  // ... on Ke = 5 effective controls: every operator image in registers (qocx_action_eff.hip)
        STATES,         // ... two to four states, a wave per state (qocx_action_states.hip)
        COSTS,          // ... any device cost descriptors: the general adjoint, one-sided (qocx_action_costs.hip)
        N16,            // n <= 16 (qocx_action16.hip)
        N64             // 33 <= n <= 64, padded to 64 (qocx_action4.hip)
    };
    enum Table {
        PLAIN,  // launch_step_table (at 17 <= n <= 32 the one K1a reads too)
        EFF     // the table of qocx_action_eff.hip: veff and the degrees from the norms of the augmented operators
    };
    Kernel kernel = NONE;
    Table table = PLAIN;
    int channels = 0;     // controls per step as the sweeps see them: Ke on effective controls, else K
    int m_max = 0;        // the Taylor terms per step the buffers hold
    int degree_rule = 1;  // knob "action_degree", as both tables take it (decided on either route)
    bool fuse = false;    // knob "action_plan": each sweep of the two-sided schedule runs to the crossing in ONE launch
    bool on() const { return kernel != NONE; }
};

// One state, Hermitian H, 17 <= n <= 32, structured M2, one final TargetStateInfidelity: the evaluation
// needs exp(a_j) psi and exp(a_j)^H lambda, never the matrix - the sweeps apply the truncated Taylor
// series (degree per step from the step table) and leave its terms to the gradient kernel; no K1a, no
// LU, no stored factors. Independent of want_grad (a forward-only evaluation returns the same costs
// bit for bit), of the batch size, chunking and segmentation. "pade_order" = 13 keeps executing
// [13/13]. The degree is decided on the device; the host's bound sizes the buffers (m_max) and a
// step beyond them sends the evaluation back to the Pade route (eval_items: `allow` is 0 then).
inline ActionPlan action_plan(const ActionFacts& f) {
    ActionPlan p;
    p.degree_rule = f.action_degree != 0 ? 1 : 0;
    const int nb = f.n <= 16 ? 1 : f.n <= 32 ? 2 : f.n <= 64 ? 4 : 0;  // 16 x 16 tiles per side (33 <= n <= 64: padded to 64)
    const bool eff = f.eff_kind != 0;
    // Knob "action": 0 never, 1 (default) at 17 <= n <= 32, 2 also at 33 <= n <= 64 (qocx_action4.hip:
    // workgroups of three waves up to n = 48, of four above). There the step table - which at nb = 2 also
    // serves K1a - is launched for the sweeps alone; the Pade route above n = 32 knows no step table and
    // stays as it is.
    // Knob "action_states": 0 (default) one state only; 2 .. QOCX_ACTION_MAX_STATES: the most states per
    // seed that take the route at 17 <= n <= 32 (qocx_action_states.hip: a wave per state). unit_ok admits
    // several states for a coherent target only - one scalar for all of them.
    const bool states_ok = f.S == 1 || (nb == 2 && f.S >= 2 && f.S <= std::min(f.action_states, QOCX_ACTION_MAX_STATES));
    // what launch_step_table needs: it interpolates the K real controls and bounds with the norms of the G_k
    const bool table_ok = !f.explicit_gen && f.nodes == 1 && !eff && !f.dense && f.K > 0 && f.have_norms;
    // Knob "action_small": 0 (default) never at n <= 16; 1: there too (qocx_action16.hip: one wave per seed, its
    // four rows of 16 lanes the four real products of a complex one), with the step table launched for the
    // sweeps alone as above 32 - and without a look at "action". Opt-in: the Pade route at n <= 16 is what
    // existing callers measure and assert on.
    // Knob "action_eff": 0 (default) a problem on effective controls - M4 on a time-independent system, H
    // quadratic in the controls - never takes the route; 1: it does where it meets every other condition at
    // S = 1 under the unit adjoint (no "action_states", no "action_costs" there), on the kernels its size
    // selects under the knobs "action" and "action_small" as for a plain problem: its generator is linear in
    // the Ke effective controls over Hermitian operators (`hermitian` covers the Q_q; the commutators of
    // M4 are made Hermitian bit for bit), the step table of qocx_action_eff.hip writes veff and the degrees
    // from the norms of the augmented operators, and the chain kernel folds the Ke cotangents back as on the
    // Pade route. Opt-in: the Pade route is what existing callers measure and assert on for these problems.
    // (The gradient kernels up to n = 32 contract with the E images, the one above with the operators.)
    const bool eff_ok = eff && f.action_eff == 1 && !f.explicit_gen && f.nodes == 1 && !f.dense && f.K > 0 &&
                        f.S == 1 && f.have_eff_norms && (nb > 2 || f.have_e_img);
    const bool sized = eff_ok ? (nb == 2 ? f.action != 0 : nb == 1 ? f.action_small == 1 : (nb == 4 && f.action == 2))
                     : nb == 2 ? (f.action != 0 && table_ok && !f.one_wave_k1a)
                     : nb == 1 ? (f.action_small == 1 && table_ok)
                               : (nb == 4 && f.action == 2 && table_ok);
    // Knob "action_costs": 0 (default) the cost set must be the one final TargetStateInfidelity of the
    // unit adjoint; 1: a problem that meets every other condition at S = 1, 17 <= n <= 32 takes the route
    // under ANY set of device descriptors - step costs, several costs, forbidden states - on the kernels
    // of qocx_action_costs.hip, whose adjoint sweep carries the true cotangent: the unit adjoint is off there
    // (the scatter kernel applies no scalar) and the schedule is one-sided whatever "bidir" says. A
    // unit_ok problem keeps the kernels above whatever this knob says.
    // (Nothing here reads the inverse-image sweep, pack8 or umode: above n = 16 the inverse-image sweep exists
    // in latency mode only, which the route yields to by name, and at n <= 16, where it is the DEFAULT, the
    // route is decided without it - and the caller switches all three off, so that no buffer or launch
    // follows them.)
    // (the device's bound of a step is the host's up to the rounding of the interpolation; equality is admitted)
    const double bound1 = std::min(f.bound1, f.bound1_mid);
    const bool except_costs = f.allow && sized && states_ok && f.nt == 1 && f.hermitian && f.inj_count == 0 &&
                              !f.latency && !f.keep_step_states && f.pade_order == 0 &&
                              bound1 <= action_theta(QOCX_ACTION_MAX_DEGREE);
    const bool unit_costs = f.unit_ok && !f.has_step_costs && f.unit_adjoint != 0;
    const bool costs = except_costs && !eff && !f.unit_ok && f.action_costs == 1 && f.S == 1 && nb == 2 &&
                       f.cost_count > 0;
    if (!((except_costs && unit_costs) || costs)) return p;
    // Knob "action_eff_exact": 1 (default) Ke = 5 at 17 <= n <= 32 on the build that holds every operator
    // image in registers; 0: the build that streams every image past the second, as every other Ke > 2.
    p.kernel = costs ? ActionPlan::COSTS
             : f.S > 1 ? ActionPlan::STATES
             : nb == 2 ? (eff && action_eff_exact_supports(f.Ke) && f.action_eff_exact != 0 ? ActionPlan::N32_EFF_EXACT
                                                                                             : ActionPlan::N32)
             : nb == 1 ? ActionPlan::N16
                       : ActionPlan::N64;
    p.table = eff ? ActionPlan::EFF : ActionPlan::PLAIN;
    p.channels = eff ? f.Ke : f.K;
    // Knob "action_degree": 1 (default) the degree of a step is the lesser of the Al-Mohy-Higham degree of
    // its 1-norm bound and the degree the remainder of a NORMAL generator needs at its spectral-norm bound
    // (qocx_action.h: action_degree_rule); 0: the 1-norm alone. The predicate above stays on the 1-norm;
    // only the buffers follow the rule - the host's two bounds of the same control maxima.
    const double bound2 = std::min(f.bound2, f.bound2_mid);
    p.m_max = std::min(QOCX_ACTION_MAX_DEGREE,
                       action_degree_rule(bound1 * (1 + 1e-9), bound2 * (1 + 1e-9), p.degree_rule));
    p.fuse = f.action_plan != 0;
    return p;
}

}  // namespace qocx

#endif
