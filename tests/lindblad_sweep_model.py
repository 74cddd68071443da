"""
lindblad_sweep_model.py - TEST INFRASTRUCTURE for LindbladSweep: the NumPy restatement of the rate
sensitivities of the device scheme (qocx_lindblad_ratesens.hip) on top of tests/lindblad_model.py,
and a stand-in backend that takes Lindblad sweeps on the host.

In the notation of lindblad_model.evaluate_with_grad (kb carries hh, Y_i are the stage values), with
rates c_l gamma_l:

    dE/dc_l = sum over sub-intervals, stages i, densities s of
              Re tr( kb_{i,s}^H  gamma_l ( L_l Y_{i,s} L_l^H - 1/2 (L_l^H L_l Y_{i,s} + Y_{i,s} L_l^H L_l) ) )

the exact derivative of the discrete scheme on its frozen grid.

Nothing here is imported by the product.
"""

import numpy as np

from tests import lindblad_model as lm
from tests.oracle_backend import OracleBackend


def scaled_system(system, factors):
    """`system` with the rates factors * gammas (a static StructuredLindblad)."""
    return lm.StructuredLindblad(system.h0, system.g, np.asarray(factors) * system.gammas,
                                 system.ops)


def rate_sensitivities(system, controls, initial_densities, evolution_time, system_eval_count,
                       costs, cost_eval_step=1, subdivision=None, factors=None,
                       piecewise_constant=False):
    """
    (error, dE/dc (L,)) of `system` with the rates factors * system.gammas (default 1): the adjoint
    recursion of lindblad_model.evaluate_with_grad with the formula above accumulated in its stage
    loop. The derivative is with respect to the FACTORS: gamma_l below is system.gammas[l].
    piecewise_constant: as in lindblad_model.evaluate_with_grad.
    """
    L = len(system.gammas)
    factors = np.ones(L) if factors is None else np.asarray(factors, dtype=np.float64)
    run = scaled_system(system, factors)
    controls = np.asarray(controls, dtype=np.float64)
    nc, k = controls.shape
    xs = np.linspace(0, evolution_time, nc)
    n_steps = system_eval_count - 1
    umax = np.max(np.abs(controls), axis=0) if k else []
    grid = lm.substep_grid(evolution_time, system_eval_count,
                           nc + 1 if piecewise_constant else nc, run.norm_bound(umax),
                           subdivision=subdivision)
    from oracle import qoc_numpy as onp

    def control(t):
        return onp.interpolate_linear_set(t, xs, controls)

    def run_substep(rho, ta, tb):
        hh = tb - ta
        ua, ub = control(ta), control(tb)
        if piecewise_constant:
            j = int(np.floor(0.5 * (ta + tb) * nc / evolution_time))
            ua = ub = controls[min(max(j, 0), nc - 1)]
        ks, ys, gens = [], [], []
        for i in range(lm.STAGES):
            u = (1 - lm.RK_C[i]) * ua + lm.RK_C[i] * ub
            a = run.generator(u, ta + lm.RK_C[i] * hh)
            yi = rho + hh * sum((lm.RK_A[i, j] * ks[j] for j in range(i)), np.zeros_like(rho))
            ks.append(run.rhs(a, yi))
            ys.append(yi)
            gens.append(a)
        new = rho + hh * sum((lm.RK_B[i] * ks[i] for i in range(lm.STAGES)), np.zeros_like(rho))
        return new, ys, gens

    step_costs = [c for c in costs if c.requires_step_evaluation]
    rho = np.asarray(initial_densities, dtype=np.complex128)
    error, checkpoints, hits = 0.0, [], {}
    for step in range(system_eval_count):
        if step % cost_eval_step == 0 and step != 0:
            for c in step_costs:
                error = error + c.cost(controls, rho, step)
                hits.setdefault(step, []).append(c)
        if step == n_steps:
            break
        for ta, tb in grid[step]:
            checkpoints.append((step, ta, tb, rho))
            rho = run_substep(rho, ta, tb)[0]
    final = rho
    for c in costs:
        if not c.requires_step_evaluation:
            error = error + c.cost(controls, final, n_steps)
            hits.setdefault(n_steps, []).append(c)

    sens = np.zeros(L)
    lam = np.zeros_like(final)
    for c in hits.get(n_steps, []):
        lam = lam + c.states_bar(controls, final, n_steps)
    ops = system.ops
    ldl = [lm.h(op) @ op for op in ops]
    for step, ta, tb, rho0 in reversed(checkpoints):
        hh = tb - ta
        _, ys, gens = run_substep(rho0, ta, tb)
        ybar_stage = [None] * lm.STAGES
        lam_new = lam.copy()
        for i in range(lm.STAGES - 1, -1, -1):
            kb = hh * lm.RK_B[i] * lam
            for j in range(i + 1, lm.STAGES):
                if lm.RK_A[j, i] != 0:
                    kb = kb + hh * lm.RK_A[j, i] * ybar_stage[j]
            ybar_stage[i] = run.rhs_adjoint(gens[i], kb)
            lam_new = lam_new + ybar_stage[i]
            for l in range(L):
                for s in range(ys[i].shape[0]):
                    y = ys[i][s]
                    d = ops[l] @ y @ lm.h(ops[l]) - 0.5 * (ldl[l] @ y + y @ ldl[l])
                    sens[l] += system.gammas[l] * np.real(np.trace(lm.h(kb[s]) @ d))
        lam = lam_new
        if abs(ta - step * (evolution_time / n_steps)) < 1e-14 * max(1.0, evolution_time):
            for c in hits.get(step, []):
                lam = lam + c.states_bar(controls, rho0, step)
    return error, sens


class LindbladSweepStandIn(OracleBackend):
    """The oracle backend plus set_lindblad_sweep: seed b is expanded into item b on the host and
    evaluated on the (K_r + J)-channel problem it was given, with the rates rate_scales[b] * gamma,
    and the items' results go back to the seeds as the engine takes them (grad_b = s_b * item
    gradient, the fixed channels dropped; the channel sensitivities are the plain sums over the
    knots, the rate sensitivities those of rate_sensitivities above). `log` records the calls."""

    def __init__(self):
        super().__init__()
        self.log = []
        self.received = []
        self.swp = None
        self.want_rates = False

    def set_lindblad_problem(self, *a, **kw):
        self.log.append("set_lindblad_problem")
        super().set_lindblad_problem(*a, **kw)
        self.problem_kw = kw
        self.swp = None

    def set_lindblad_sweep(self, scales, offsets, rate_scales=None):
        self.log.append("set_lindblad_sweep")
        K = self.lb["K"]
        J = 0 if offsets is None else np.asarray(offsets).shape[1]
        B = next(len(a) for a in (scales, offsets, rate_scales) if a is not None)
        scales = np.ones((B, K - J)) if scales is None else np.asarray(scales, dtype=np.float64)
        offsets = np.zeros((B, 0)) if offsets is None else np.asarray(offsets, dtype=np.float64)
        assert scales.shape == (B, K - J) and offsets.shape == (B, J)
        if rate_scales is not None:
            rate_scales = np.asarray(rate_scales, dtype=np.float64)
            assert rate_scales.shape == (B, len(self.lb_system.gammas))
            assert not self.problem_kw.get("fixed_subdivision"), "rates need a static problem"
        self.received.append((dict(self.lb), scales.copy(), offsets.copy(),
                              None if rate_scales is None else rate_scales.copy()))
        self.swp = (scales, offsets, rate_scales)

    def lindblad_sweep_want_rate_sensitivities(self, on):
        self.log.append("want_rates %d" % bool(on))
        self.want_rates = bool(on)

    def _items(self, controls):
        p = self.lb
        scales, offsets, _ = self.swp
        kr = scales.shape[1]
        u = np.asarray(controls, dtype=np.float64).reshape(-1, p["Nc"], kr)
        assert u.shape[0] == scales.shape[0], "a sweep takes exactly its own seed count"
        items = np.empty((u.shape[0], p["Nc"], p["K"]))
        items[..., :kr] = scales[:, None, :] * u
        items[..., kr:] = offsets[:, None, :]
        return u, items

    def evaluate_lindblad(self, controls, want_grad=True, want_final=True):
        if self.swp is None:
            return super().evaluate_lindblad(controls, want_grad, want_final)
        self.log.append("evaluate_lindblad grad=%d" % bool(want_grad))
        scales, offsets, rates = self.swp
        kr = scales.shape[1]
        u, items = self._items(controls)
        base = self.lb_system
        cost, grads, final = [], [], []
        self.item_grads, self.seed_controls, self.rate_sens = None, u, None
        rate_rows = []
        for b in range(u.shape[0]):
            if rates is not None:
                self.lb_system = scaled_system(base, rates[b])
            try:
                c, g, f = super().evaluate_lindblad(items[b:b + 1], want_grad, want_final)
            finally:
                self.lb_system = base
            self.calls -= 1
            cost.append(c[0])
            final.append(f[0])
            if want_grad:
                grads.append(g[0])
                if self.want_rates:
                    p = self.lb
                    rate_rows.append(rate_sensitivities(
                        base, items[b], p["rho0"], p["T"], p["N"], self.lb_costs, p["ces"],
                        subdivision=self.lb_subdivision,
                        factors=None if rates is None else rates[b])[1])
        self.calls += 1
        if want_grad:
            self.item_grads = np.stack(grads)
            if self.want_rates:
                self.rate_sens = np.stack(rate_rows)
        return (np.array(cost), None if not want_grad
                else scales[:, None, :] * self.item_grads[..., :kr], np.stack(final))

    def lindblad_sweep_sensitivities(self):
        self.log.append("lindblad_sweep_sensitivities")
        kr = self.swp[0].shape[1]
        g = self.item_grads
        return (np.sum(self.seed_controls * g[..., :kr], axis=1), np.sum(g[..., kr:], axis=1),
                self.rate_sens)
