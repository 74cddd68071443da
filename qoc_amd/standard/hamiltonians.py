"""
hamiltonians.py - Hamiltonians whose structure the engine can use beyond linearity.

QuadraticHamiltonian is a `hamiltonian(controls, time)` callable like any other (every entry
point and the oracle take it as such). Its type tells the Schroedinger evaluator that

    H(r, t) = H0(t) + sum_k r_k G_k(t) + sum_(k <= l) r_k r_l Q_kl

in the real controls r, so under MagnusPolicy.M2 the engine evaluates it on the device as a
problem linear in the effective controls (r_k, r_k r_l) - no call of the callable per step or
per evaluation (qocx_set_quadratic_terms). The Piccolo Hamiltonian of the reference's report
(report.tex:22-32, an AC-Stark term in epsilon_sb^2) has this form.

HamiltonianEnsemble is NOT a callable: it is M copies of a linear or quadratic Hamiltonian with
scaled controls and fixed perturbation terms, all driven by the same controls (robust GRAPE). The
Schroedinger evaluator sets it up as one structured problem whose extra control channels are the
perturbation matrices, and the engine expands every seed into its M members on the device
(qocx_set_ensemble). A QuadraticHamiltonian base keeps its terms on the device as well, each
optionally scaled per member (quadratic_scales, qocx_set_ensemble_quadratic_scales). On the Lindblad
path every member may scale the dissipation rates as well (rate_scales, an uncertain T1 / T2:
qocx_lindblad_set_ensemble_rates).

HamiltonianSweep is not a callable either: it is B systems, each with controls of its own - scaled
controls and fixed terms per SEED (a gate-time sweep, a calibration family). The Schroedinger
evaluator sets it up as the ensemble's structured problem and the engine expands seed b into item b
on the device (qocx_set_sweep).

LindbladSweep is the sweep of the Lindblad entry points: seed b also has dissipation rates of its own
(rate_scales), and its durations scale the rates with the Hamiltonian (qocx_lindblad_set_sweep).
"""

import numbers

import numpy as np


class QuadraticHamiltonian(object):
    """
    H = QuadraticHamiltonian(linear_hamiltonian, quadratic_terms)

    linear_hamiltonian :: (controls, time) -> (n x n) - real-linear in the controls, time
        dependence allowed (what qoc_amd.core.structure.probe_hamiltonian accepts).
    quadratic_terms :: sequence of (k, l, Q) with 0 <= k <= l, Q a constant complex (n x n)
        matrix. k and l index the REAL controls: the controls themselves for real controls;
        Re u_j -> 2 j and Im u_j -> 2 j + 1 for complex ones (so |u_j|^2 Q is the two terms
        (2j, 2j, Q) and (2j+1, 2j+1, Q)). Repeated (k, l) pairs add up.

    H(controls, time) = linear_hamiltonian(controls, time) + sum r_k r_l Q_kl.
    """

    def __init__(self, linear_hamiltonian, quadratic_terms):
        if not callable(linear_hamiltonian):
            raise ValueError("linear_hamiltonian must be a callable (controls, time) -> matrix")
        merged, order, shape = {}, [], None
        for entry in quadratic_terms:
            try:
                k, l, q = entry
            except (TypeError, ValueError):
                raise ValueError("each quadratic term must be a tuple (k, l, Q), got {!r}"
                                 "".format(entry))
            for idx in (k, l):
                if isinstance(idx, bool) or not isinstance(idx, numbers.Integral):
                    raise ValueError("quadratic term indices must be integers, got {!r}"
                                     "".format((k, l)))
            k, l = int(k), int(l)
            if not 0 <= k <= l:
                raise ValueError("quadratic term indices must satisfy 0 <= k <= l, got ({}, {})"
                                 "".format(k, l))
            q = np.array(q, dtype=np.complex128)
            if q.ndim != 2 or q.shape[0] != q.shape[1]:
                raise ValueError("quadratic term ({}, {}): Q must be a square matrix, got shape {}"
                                 "".format(k, l, q.shape))
            if shape is not None and q.shape != shape:
                raise ValueError("quadratic term ({}, {}): Q has shape {}, the others {}"
                                 "".format(k, l, q.shape, shape))
            shape = q.shape
            if not np.all(np.isfinite(q)):
                raise ValueError("quadratic term ({}, {}): Q is not finite".format(k, l))
            if (k, l) in merged:
                merged[(k, l)] = merged[(k, l)] + q
            else:
                merged[(k, l)] = q
                order.append((k, l))
        self.linear_hamiltonian = linear_hamiltonian
        self.pairs = np.array(order, dtype=np.int32).reshape(-1, 2)
        self.matrices = (np.stack([merged[p] for p in order]) if order
                         else np.zeros((0, 0, 0), dtype=np.complex128))
        self.hilbert_size = None if shape is None else shape[0]

    @property
    def max_index(self):
        """The largest real-control index the quadratic terms use (-1 without terms)."""
        return int(self.pairs.max()) if len(self.pairs) else -1

    def check_real_control_count(self, real_control_count, hilbert_size=None):
        """Raise ValueError unless every index is < real_control_count (and Q is n x n)."""
        if self.max_index >= real_control_count:
            raise ValueError("quadratic term index {} out of range for {} real controls"
                             "".format(self.max_index, real_control_count))
        if (hilbert_size is not None and self.hilbert_size is not None
                and self.hilbert_size != hilbert_size):
            raise ValueError("quadratic term matrices are {0} x {0}, the system is {1} x {1}"
                             "".format(self.hilbert_size, hilbert_size))

    def __call__(self, controls, time):
        out = np.asarray(self.linear_hamiltonian(controls, time), dtype=np.complex128)
        if not len(self.pairs):
            return out
        if controls is None:
            raise ValueError("a QuadraticHamiltonian with quadratic terms needs controls")
        u = np.asarray(controls)
        r = np.empty(2 * u.shape[-1]) if np.iscomplexobj(u) else np.asarray(u, dtype=np.float64)
        if np.iscomplexobj(u):
            r[0::2], r[1::2] = u.real, u.imag
        self.check_real_control_count(r.shape[0])
        for (k, l), q in zip(self.pairs, self.matrices):
            out = out + (r[k] * r[l]) * q
        return out

    def __repr__(self):
        return "QuadraticHamiltonian({!r}, {} quadratic terms)".format(
            self.linear_hamiltonian, len(self.pairs))


def _real_array(value, name, ndim):
    out = np.asarray(value)
    if np.iscomplexobj(out):
        raise ValueError("{} must be real".format(name))
    out = np.array(out, dtype=np.float64)
    if out.ndim != ndim:
        raise ValueError("{} must have {} dimensions, got shape {}".format(name, ndim, out.shape))
    if not np.all(np.isfinite(out)):
        raise ValueError("{} is not finite".format(name))
    return out


class HamiltonianEnsemble(object):
    """
    E = HamiltonianEnsemble(hamiltonian, perturbations=None, offsets=None, control_scales=None,
                            weights=None, quadratic_scales=None, rate_scales=None)

    M copies of a system, all driven by the same controls (robust GRAPE). Member m is

        H_m(u, t) = hamiltonian(s_m * u, t) + sum_j offsets[m, j] D_j

    and, for a QuadraticHamiltonian base with real channels r of u and terms (k_q, l_q, Q_q),

        H_m(u, t) = linear(s_m * u, t) + sum_j offsets[m, j] D_j
                    + sum_q quadratic_scales[m, q] (s_m,kq r_kq) (s_m,lq r_lq) Q_q

    hamiltonian :: (controls, time) -> (n x n), real-linear in the controls (time dependence
        allowed), or a QuadraticHamiltonian (MagnusPolicy.M2).
    perturbations :: (J, n, n) complex - the fixed matrices D_j (detuning, crosstalk, ...).
    offsets :: (M, J) real - delta_mj; given exactly when perturbations are.
    control_scales :: (M, control_count) real - s_mk (amplitude errors); a complex control's
        scale multiplies its real and imaginary parts alike. Default: all 1.
    weights :: (M,) real >= 0 - w_m; default 1 / M.
    quadratic_scales :: (M, Q) real - c_mq, member m's factor of the base's q-th merged quadratic
        term, in the order of hamiltonian.pairs (an uncertain Stark coefficient). Only for a
        QuadraticHamiltonian base with Q terms. Default: all 1.

    rate_scales :: (M, L) real, finite and >= 0 - c_mi, member m's factor of the i-th dissipation
        rate of the problem's lindblad_data: gamma_mi = c_mi * gamma_i (an uncertain T1 / T2). Lindblad
        entry points only, with L the number of Lindblad operators and a time-independent system
        (hamiltonian and lindblad_data). Default: every member takes the rates as given.

    M is read from whichever of offsets, control_scales, weights, quadratic_scales and rate_scales is
    given; they must agree.
    Passed as the `hamiltonian` of evolve_schroedinger_discrete, grape_schroedinger_discrete or
    grape_schroedinger_discrete_batch, the cost is sum_m w_m c_m over the members' device costs
    (costs of the controls alone are added once), and the gradient is that of this sum. The
    object is not itself callable: member(m) is member m as a plain callable.
    """

    def __init__(self, hamiltonian, perturbations=None, offsets=None, control_scales=None,
                 weights=None, quadratic_scales=None, rate_scales=None):
        if isinstance(hamiltonian, HamiltonianSweep):
            raise NotImplementedError(
                "a HamiltonianSweep inside a HamiltonianEnsemble is not evaluated: the engine "
                "takes a sweep or an ensemble per problem (sweep x ensemble is out of scope)")
        if not callable(hamiltonian):
            raise ValueError("hamiltonian must be a callable (controls, time) -> matrix")
        counts = {}
        if perturbations is not None:
            perturbations = np.array(perturbations, dtype=np.complex128)
            if perturbations.ndim != 3 or perturbations.shape[1] != perturbations.shape[2]:
                raise ValueError("perturbations must be (J, n, n), got shape {}"
                                 "".format(perturbations.shape))
            if not np.all(np.isfinite(perturbations)):
                raise ValueError("perturbations is not finite")
            if offsets is None:
                raise ValueError("perturbations need offsets of shape (M, J)")
        if offsets is not None:
            if perturbations is None:
                raise ValueError("offsets need perturbations (the matrices D_j they multiply)")
            offsets = _real_array(offsets, "offsets", 2)
            if offsets.shape[1] != perturbations.shape[0]:
                raise ValueError("offsets must be (M, J) with J = {} perturbations, got shape {}"
                                 "".format(perturbations.shape[0], offsets.shape))
            counts["offsets"] = offsets.shape[0]
        if control_scales is not None:
            control_scales = _real_array(control_scales, "control_scales", 2)
            counts["control_scales"] = control_scales.shape[0]
        if weights is not None:
            weights = _real_array(weights, "weights", 1)
            if np.any(weights < 0):
                raise ValueError("weights must be >= 0")
            counts["weights"] = weights.shape[0]
        if quadratic_scales is not None:
            if not isinstance(hamiltonian, QuadraticHamiltonian):
                raise ValueError("quadratic_scales need a QuadraticHamiltonian base, got {!r}"
                                 "".format(hamiltonian))
            quadratic_scales = _real_array(quadratic_scales, "quadratic_scales", 2)
            if quadratic_scales.shape[1] != len(hamiltonian.pairs):
                raise ValueError("quadratic_scales must be (M, Q) with Q = {} quadratic terms, got "
                                 "shape {}".format(len(hamiltonian.pairs), quadratic_scales.shape))
            counts["quadratic_scales"] = quadratic_scales.shape[0]
        if rate_scales is not None:
            rate_scales = _real_array(rate_scales, "rate_scales", 2)
            if np.any(rate_scales < 0):
                raise ValueError("rate_scales must be >= 0 (they multiply dissipation rates)")
            counts["rate_scales"] = rate_scales.shape[0]
        if not counts:
            raise ValueError("an ensemble needs offsets, control_scales or weights (M is read "
                             "from them)")
        if len(set(counts.values())) > 1:
            raise ValueError("offsets, control_scales, weights, quadratic_scales and rate_scales "
                             "disagree on the member count: {}"
                             "".format(", ".join("{} {}".format(k, v) for k, v in counts.items())))
        M = next(iter(counts.values()))
        if M == 0:
            raise ValueError("an ensemble needs at least one member (M = 0 in {})"
                             "".format(", ".join(counts)))
        self.hamiltonian = hamiltonian
        self.perturbations = perturbations
        self.offsets = offsets
        self.control_scales = control_scales
        self.weights = weights if weights is not None else np.full(M, 1.0 / M)
        self.quadratic_scales = quadratic_scales
        self.rate_scales = rate_scales
        self.member_count = M

    @property
    def perturbation_count(self):
        """J, the number of perturbation matrices."""
        return 0 if self.perturbations is None else self.perturbations.shape[0]

    @property
    def hilbert_size(self):
        """n of the perturbation matrices (None without them)."""
        return None if self.perturbations is None else self.perturbations.shape[1]

    def real_channel_scales(self, control_count, complex_controls):
        """s_mk per real control channel, (M, K_r): the scales as given for real controls, each
        repeated for Re and Im of a complex control (channels 2k and 2k + 1)."""
        if self.control_scales is None:
            kr = control_count * (2 if complex_controls else 1)
            return np.ones((self.member_count, kr))
        if self.control_scales.shape[1] != control_count:
            raise ValueError("control_scales must be (M, control_count) = ({}, {}), got shape {}"
                             "".format(self.member_count, control_count,
                                       self.control_scales.shape))
        if complex_controls:
            return np.repeat(self.control_scales, 2, axis=1)
        return self.control_scales.copy()

    def member(self, m):
        """Member m as a plain callable (controls, time) -> (n x n)."""
        m = int(m)
        if not 0 <= m < self.member_count:
            raise IndexError("member {} out of range for {} members".format(m, self.member_count))
        base = self.hamiltonian
        scales = None if self.control_scales is None else self.control_scales[m]
        shift = None
        if self.perturbations is not None:
            shift = np.einsum("j,jab->ab", self.offsets[m].astype(np.complex128),
                              self.perturbations)

        quadratic = isinstance(base, QuadraticHamiltonian) and len(base.pairs) > 0
        term_scales = None if self.quadratic_scales is None else self.quadratic_scales[m]

        def hamiltonian(controls, time):
            u = controls
            if scales is not None and controls is not None:
                u = np.asarray(controls) * scales
            if not quadratic:
                out = np.asarray(base(u, time), dtype=np.complex128)
                return out if shift is None else out + shift
            # a quadratic base: its linear part on the scaled controls, and the terms here -
            # c_mq (s r)_k (s r)_l Q_q in the real channels r of the controls
            out = np.asarray(base.linear_hamiltonian(u, time), dtype=np.complex128)
            if shift is not None:
                out = out + shift
            if u is None:
                raise ValueError("a QuadraticHamiltonian with quadratic terms needs controls")
            u = np.asarray(u)
            if np.iscomplexobj(u):
                r = np.empty(2 * u.shape[-1])
                r[0::2], r[1::2] = u.real, u.imag
            else:
                r = np.asarray(u, dtype=np.float64)
            base.check_real_control_count(r.shape[0])
            for q, ((k, l), mat) in enumerate(zip(base.pairs, base.matrices)):
                c = 1.0 if term_scales is None else term_scales[q]
                out = out + (c * (r[k] * r[l])) * mat
            return out
        return hamiltonian

    def member_lindblad_data(self, m, lindblad_data):
        """Member m's lindblad_data as a plain callable time -> (c_m * dissipators, operators): the
        problem's own where the ensemble has no rate_scales."""
        m = int(m)
        if not 0 <= m < self.member_count:
            raise IndexError("member {} out of range for {} members".format(m, self.member_count))
        if not callable(lindblad_data):
            raise ValueError("lindblad_data must be a callable time -> (dissipators, operators)")
        if self.rate_scales is None:
            return lindblad_data
        factors = self.rate_scales[m]

        def member_data(time):
            dissipators, operators = lindblad_data(time)
            dissipators = np.asarray(dissipators)
            if dissipators.shape != factors.shape:
                raise ValueError("rate_scales must be (M, L) with L = {} Lindblad operators, got shape "
                                 "{}".format(dissipators.shape[0] if dissipators.ndim else 0,
                                             self.rate_scales.shape))
            return factors * dissipators, operators
        return member_data

    def __repr__(self):
        rates = "" if self.rate_scales is None else ", rate_scales {}".format(
            "x".join(str(d) for d in self.rate_scales.shape))
        return "HamiltonianEnsemble({!r}, {} members, {} perturbations{})".format(
            self.hamiltonian, self.member_count, self.perturbation_count, rates)


class HamiltonianSweep(object):
    """
    W = HamiltonianSweep(hamiltonian, perturbations=None, offsets=None, control_scales=None)

    B systems, each driven by controls of its own (a gate-time sweep, a calibration family) - the
    complement of a HamiltonianEnsemble, which drives M systems with one pulse. Seed b is

        H_b(u, t) = hamiltonian(s_b * u, t) + sum_j offsets[b, j] D_j

    hamiltonian :: (controls, time) -> (n x n), real-linear in the controls (time dependence
        allowed); not a QuadraticHamiltonian, a HamiltonianEnsemble or another sweep.
    perturbations :: (J, n, n) complex - the fixed matrices D_j.
    offsets :: (B, J) real - delta_bj; given exactly when perturbations are.
    control_scales :: (B, control_count) real - s_bk; a complex control's scale multiplies its
        real and imaginary parts alike. Default: all 1.

    B is read from whichever of offsets and control_scales is given; they must agree.
    Passed as the `hamiltonian` of grape_schroedinger_discrete_batch (B = initial_controls.shape[0])
    or of SchroedingerEvaluator (evaluate_batch with a batch of B), seed b is optimised or
    evaluated on system b; the engine expands the seeds on the device (qocx_set_sweep) and returns
    sweep_sensitivities, d error_b / d s_bk and d error_b / d delta_bj. The object is not itself
    callable: member(b) is seed b's system as a plain callable, slice(lo, hi) the sweep of a
    contiguous block of seeds.

    HamiltonianSweep.durations(...) builds the sweep in which seed b runs for its own evolution
    time.
    """

    time_scaled = False
    evolution_times = None
    reference_time = None
    searches_duration = False   # durations(time_bounds=...): tau_b is optimised as well
    time_bounds = None
    time_weight = 0.0

    def __init__(self, hamiltonian, perturbations=None, offsets=None, control_scales=None,
                 _more_counts=None):
        if not callable(hamiltonian):
            raise ValueError("hamiltonian must be a callable (controls, time) -> matrix")
        counts = dict(_more_counts or {})  # (a subclass's own tables: LindbladSweep's rate_scales)
        if perturbations is not None:
            perturbations = np.array(perturbations, dtype=np.complex128)
            if perturbations.ndim != 3 or perturbations.shape[1] != perturbations.shape[2]:
                raise ValueError("perturbations must be (J, n, n), got shape {}"
                                 "".format(perturbations.shape))
            if not np.all(np.isfinite(perturbations)):
                raise ValueError("perturbations is not finite")
            if offsets is None:
                raise ValueError("perturbations need offsets of shape (B, J)")
        if offsets is not None:
            if perturbations is None:
                raise ValueError("offsets need perturbations (the matrices D_j they multiply)")
            offsets = _real_array(offsets, "offsets", 2)
            if offsets.shape[1] != perturbations.shape[0]:
                raise ValueError("offsets must be (B, J) with J = {} perturbations, got shape {}"
                                 "".format(perturbations.shape[0], offsets.shape))
            counts["offsets"] = offsets.shape[0]
        if control_scales is not None:
            control_scales = _real_array(control_scales, "control_scales", 2)
            counts["control_scales"] = control_scales.shape[0]
        if not counts:
            raise ValueError("a sweep needs offsets or control_scales (B is read from them)")
        if len(set(counts.values())) > 1:
            raise ValueError("{} disagree on the seed count: {}".format(
                " and ".join(sorted(counts)) if _more_counts else "offsets and control_scales",
                ", ".join("{} {}".format(k, v) for k, v in counts.items())))
        B = next(iter(counts.values()))
        if B == 0:
            raise ValueError("a sweep needs at least one seed (B = 0 in {})"
                             "".format(", ".join(counts)))
        self.hamiltonian = hamiltonian
        self.perturbations = perturbations
        self.offsets = offsets
        self.control_scales = control_scales
        self.seed_count = B
        self._source = None          # durations(): the user's hamiltonian, whose drift is D_0
        self._extra_perturbations = None
        self._tau = None
        self._user_scales = control_scales   # s0, delta0 of time_gradients: the values before tau
        self._user_offsets = offsets

    @classmethod
    def durations(cls, hamiltonian, evolution_times, reference_time, control_scales=None,
                  perturbations=None, offsets=None, time_bounds=None, time_weight=0.0):
        """
        The sweep in which seed b runs for evolution_times[b]: with tau_b = T_b / reference_time,

            tau_b * hamiltonian(u, t)  on  [0, reference_time]

        is the system on [0, T_b] - exact for a time-independent hamiltonian under every Magnus
        policy (scaling H is scaling time). The sweep's base is hamiltonian(u, t) - hamiltonian(0, t),
        its first fixed matrix D_0 = hamiltonian(0, .) with offset tau_b, every control scale and
        every further offset is multiplied by tau_b. The caller passes evolution_time =
        reference_time to the entry point.

        evolution_times :: (B,) finite and > 0; reference_time :: finite and > 0.
        control_scales, perturbations, offsets: as in the constructor, before the factor tau_b.
        A time-dependent hamiltonian is a ValueError: here when control_scales tell the control
        count, else when the sweep meets its problem (the probe of qoc_amd.core.structure).
        The sweep carries evolution_times, reference_time and time_scaled = True;
        time_gradients() turns its sensitivities into d error_b / d T_b.

        time_bounds = (T_min, T_max), finite with 0 < T_min <= T_max, turns the sweep into a duration
        search (minimum-time GRAPE): evolution_times are the STARTING durations (inside the box, else
        ValueError) and tau_b becomes one more optimised parameter of seed b in
        grape_schroedinger_discrete_batch - the last entry of its flat parameter vector, stepped by
        the optimizer with the controls' rule and learning rate. Each iteration tau_b is clipped IN
        PLACE to [T_min, T_max] / reference_time before the controls are expanded: the optimizer's
        own parameter is clipped, exactly as real controls are clipped by max_control_norms (and so
        it is with complex controls and a ControlBasis too, whose controls are clipped as copies).
        time_weight = lambda >= 0, finite (needs time_bounds), prices time linearly: the error of seed b
        is E_b(u_b, tau_b) + lambda * tau_b, the time term one product and one rounding, added last -
        after the state costs and the costs of the controls. The sweep then carries
        searches_duration = True, time_bounds and time_weight; member(b) stays the system at the
        STARTING duration. Without time_bounds the sweep is what it is without these two arguments.
        """
        time_weight = float(time_weight)
        if time_bounds is None:
            if time_weight != 0.0:  # (NaN included)
                raise ValueError("time_weight needs time_bounds (the box of a duration search)")
        else:
            try:
                t_min, t_max = (float(v) for v in time_bounds)
            except (TypeError, ValueError):
                raise ValueError("time_bounds must be (T_min, T_max)")
            if not (np.isfinite(t_min) and np.isfinite(t_max)):
                raise ValueError("time_bounds must be finite")
            if not 0 < t_min <= t_max:
                raise ValueError("time_bounds must be ordered: 0 < T_min <= T_max")
            if not np.isfinite(time_weight) or time_weight < 0:
                raise ValueError("time_weight must be finite and >= 0")
            time_bounds = (t_min, t_max)
        if not callable(hamiltonian):
            raise ValueError("hamiltonian must be a callable (controls, time) -> matrix")
        if isinstance(hamiltonian, (QuadraticHamiltonian, HamiltonianEnsemble, HamiltonianSweep)):
            raise NotImplementedError(
                "a duration sweep needs a plain hamiltonian linear in the controls, got {!r}"
                "".format(hamiltonian))
        times = _real_array(evolution_times, "evolution_times", 1)
        if times.shape[0] == 0:
            raise ValueError("a sweep needs at least one seed (evolution_times is empty)")
        if np.any(times <= 0):
            raise ValueError("evolution_times must be > 0")
        reference_time = float(reference_time)
        if not np.isfinite(reference_time) or reference_time <= 0:
            raise ValueError("reference_time must be finite and > 0")
        B = times.shape[0]
        tau = times / reference_time
        user_offsets = None
        if perturbations is not None or offsets is not None:
            # (the constructor's checks, on the user's own values)
            probe = cls(hamiltonian, perturbations, offsets, None)
            if probe.seed_count != B:
                raise ValueError("offsets are for {} seeds, evolution_times for {}"
                                 "".format(probe.seed_count, B))
            perturbations, user_offsets = probe.perturbations, probe.offsets
        user_scales = None
        if control_scales is not None:
            user_scales = _real_array(control_scales, "control_scales", 2)
            if user_scales.shape[0] != B:
                raise ValueError("control_scales are for {} seeds, evolution_times for {}"
                                 "".format(user_scales.shape[0], B))

        def base(controls, time):
            u = np.asarray(controls)
            return (np.asarray(hamiltonian(u, time), dtype=np.complex128)
                    - np.asarray(hamiltonian(np.zeros_like(u), time), dtype=np.complex128))

        self = cls.__new__(cls)
        self.hamiltonian = base
        self._source = hamiltonian
        self._extra_perturbations = perturbations   # D_1 ..: the user's; D_0 is resolved later
        self.perturbations = None
        columns = [tau[:, None]]
        if user_offsets is not None:
            columns.append(tau[:, None] * user_offsets)
        self.offsets = np.concatenate(columns, axis=1)
        self._user_scales = user_scales
        self._user_offsets = np.concatenate(
            [np.ones((B, 1))] + ([user_offsets] if user_offsets is not None else []), axis=1)
        # (scales of all 1 are kept implicit until the control count is known)
        self.control_scales = None if user_scales is None else tau[:, None] * user_scales
        self._tau = tau
        self.seed_count = B
        self.time_scaled = True
        self.evolution_times = times
        self.reference_time = reference_time
        if time_bounds is not None:
            if np.any(times < time_bounds[0]) or np.any(times > time_bounds[1]):
                raise ValueError("evolution_times (the starting durations) must lie inside "
                                 "time_bounds = {}".format(time_bounds))
            self.searches_duration = True
            self.time_bounds = time_bounds
            self.time_weight = time_weight
        if user_scales is not None:
            self.resolve(user_scales.shape[1], False, None,
                         [0.0, reference_time / 3.0, reference_time])
        return self

    @classmethod
    def duration_search(cls, hamiltonian, evolution_times, reference_time, time_bounds,
                        time_weight=0.0, control_scales=None, perturbations=None, offsets=None):
        """The duration search under a name of its own: exactly what durations(..., time_bounds=,
        time_weight=) builds (see there). time_bounds is required."""
        if time_bounds is None:
            raise ValueError("time_bounds must be (T_min, T_max)")
        return cls.durations(hamiltonian, evolution_times, reference_time,
                             control_scales=control_scales, perturbations=perturbations,
                             offsets=offsets, time_bounds=time_bounds, time_weight=time_weight)

    @property
    def perturbation_count(self):
        """J, the number of fixed matrices (a duration sweep: the drift D_0 among them)."""
        return 0 if self.offsets is None else self.offsets.shape[1]

    @property
    def hilbert_size(self):
        """n of the fixed matrices (None without them, or before a duration sweep is resolved)."""
        return None if self.perturbations is None else self.perturbations.shape[1]

    def resolve(self, control_count, complex_controls, hilbert_size, times):
        """The fixed matrices (J, n, n) for a problem with this control count; None for J = 0. A
        duration sweep forms D_0 = hamiltonian(0, .) here and raises ValueError when hamiltonian
        depends on time at `times` (structure.probe_hamiltonian's own decision)."""
        if not self.time_scaled:
            return self.perturbations
        from qoc_amd.core import structure
        if control_count < 1:
            raise NotImplementedError("a HamiltonianSweep needs at least one control")
        zero = np.zeros(control_count, dtype=np.complex128 if complex_controls else np.float64)
        drift = np.asarray(self._source(zero, times[0]), dtype=np.complex128)
        if drift.ndim != 2 or drift.shape[0] != drift.shape[1]:
            raise ValueError("hamiltonian returned shape {}, expected a square matrix"
                             "".format(drift.shape))
        n = drift.shape[0] if hilbert_size is None else hilbert_size
        h0, g = structure.probe_hamiltonian(self._source, n, control_count, complex_controls,
                                            list(times))
        if h0.shape[0] != 1:
            raise ValueError(
                "a duration sweep needs a time-independent hamiltonian: scaling H by T_b / "
                "reference_time is scaling time only then (hamiltonian(controls, time) depends "
                "on time)")
        if not np.all(np.isfinite(h0)):
            raise ValueError("hamiltonian(0, .) is not finite")
        extra = self._extra_perturbations
        if extra is not None and extra.shape[1] != n:
            raise ValueError("perturbations are {0} x {0}, the system is {1} x {1}".format(
                extra.shape[1], n))
        self.perturbations = h0 if extra is None else np.concatenate([h0, extra], axis=0)
        return self.perturbations

    def real_channel_scales(self, control_count, complex_controls):
        """s_bk per real control channel, (B, K_r): the scales as given for real controls, each
        repeated for Re and Im of a complex control (channels 2k and 2k + 1)."""
        scales = self.control_scales
        if scales is None:
            scales = np.ones((self.seed_count, control_count))
            if self.time_scaled:
                scales = scales * self._tau[:, None]
        if scales.shape[1] != control_count:
            raise ValueError("control_scales must be (B, control_count) = ({}, {}), got shape {}"
                             "".format(self.seed_count, control_count, scales.shape))
        if complex_controls:
            return np.repeat(scales, 2, axis=1)
        return scales.copy()

    @property
    def tau_bounds(self):
        """The box of a duration search in units of reference_time: (T_min, T_max) / reference_time."""
        return (self.time_bounds[0] / self.reference_time,
                self.time_bounds[1] / self.reference_time)

    def base_tables(self, control_count, complex_controls):
        """(s0 (B, K_r) or None for all 1, delta0 (B, J)) of a duration sweep: its tables before the
        factor tau_b, per real control channel (the drift column of delta0 is 1)."""
        if not self.time_scaled:
            raise ValueError("base_tables belong to a duration sweep (HamiltonianSweep.durations)")
        scales = self._user_scales
        if scales is not None:
            if scales.shape[1] != control_count:
                raise ValueError("control_scales must be (B, control_count) = ({}, {}), got shape "
                                 "{}".format(self.seed_count, control_count, scales.shape))
            scales = np.repeat(scales, 2, axis=1) if complex_controls else scales.copy()
        return scales, self._user_offsets.copy()

    def member(self, b):
        """Seed b's system as a plain callable (controls, time) -> (n x n). For a duration sweep
        that is tau_b * hamiltonian(u, t) (a duration search: at the starting duration)."""
        b = int(b)
        if not 0 <= b < self.seed_count:
            raise IndexError("seed {} out of range for {} seeds".format(b, self.seed_count))
        base, source = self.hamiltonian, self._source
        scales = None if self.control_scales is None else self.control_scales[b]
        if scales is None and self.time_scaled:
            scales = self._tau[b]
        offsets = None if self.offsets is None else self.offsets[b]
        fixed = self._extra_perturbations if self.time_scaled else self.perturbations
        first = 1 if self.time_scaled else 0
        shift = None
        if fixed is not None:
            shift = np.einsum("j,jab->ab", offsets[first:].astype(np.complex128), fixed)

        def hamiltonian(controls, time):
            u = np.asarray(controls) * scales if scales is not None else controls
            out = np.asarray(base(u, time), dtype=np.complex128)
            if source is not None:  # the drift D_0 = hamiltonian(0, .), times tau_b
                out = out + offsets[0] * np.asarray(
                    source(np.zeros_like(np.asarray(controls)), time), dtype=np.complex128)
            return out if shift is None else out + shift
        return hamiltonian

    def slice(self, lo, hi):
        """The sweep of seeds lo .. hi - 1 (what a rank of a communicator evaluates)."""
        lo, hi = int(lo), int(hi)
        if not 0 <= lo < hi <= self.seed_count:
            raise IndexError("slice [{}, {}) out of range for {} seeds (at least one seed)"
                             "".format(lo, hi, self.seed_count))
        import copy
        out = copy.copy(self)
        for name in ("offsets", "control_scales", "_user_scales", "_user_offsets",
                     "evolution_times", "_tau"):
            value = getattr(self, name, None)
            if value is not None:
                setattr(out, name, value[lo:hi].copy())
        out.seed_count = hi - lo
        return out

    def time_gradients(self, scale_sens, offset_sens):
        """d error_b / d T_b (B,) of a duration sweep from its sensitivities (the chain rule through
        tau_b = T_b / reference_time): (sum_k dE/ds_bk s0_bk + sum_j dE/ddelta_bj delta0_bj) /
        reference_time with s0, delta0 the values before the factor tau_b (delta0 = 1 for D_0).
        scale_sens :: (B, control_count), offset_sens :: (B, J)."""
        if not self.time_scaled:
            raise ValueError("time_gradients belong to a duration sweep "
                             "(HamiltonianSweep.durations)")
        scale_sens = np.asarray(scale_sens, dtype=np.float64)
        offset_sens = np.asarray(offset_sens, dtype=np.float64)
        s0 = np.ones_like(scale_sens) if self._user_scales is None else self._user_scales
        if scale_sens.shape != s0.shape or offset_sens.shape != self._user_offsets.shape:
            raise ValueError("sensitivities must be (B, control_count) and (B, J) = {}, got {} "
                             "and {}".format(self._user_offsets.shape, scale_sens.shape,
                                             offset_sens.shape))
        return (np.sum(scale_sens * s0, axis=1)
                + np.sum(offset_sens * self._user_offsets, axis=1)) / self.reference_time

    def __repr__(self):
        return "HamiltonianSweep({!r}, {} seeds, {} fixed matrices{})".format(
            self._source if self._source is not None else self.hamiltonian, self.seed_count,
            self.perturbation_count, ", durations" if self.time_scaled else "")


class LindbladSweep(HamiltonianSweep):
    """
    W = LindbladSweep(hamiltonian, perturbations=None, offsets=None, control_scales=None,
                      rate_scales=None)

    A HamiltonianSweep for the Lindblad entry points: B open systems, each driven by controls of
    its own. Seed b is the Lindblad problem with

        H_b(u, t) = hamiltonian(s_b * u, t) + sum_j offsets[b, j] D_j

    and the dissipation rates rate_scales[b] * dissipators of the problem's lindblad_data; the
    operators, the initial densities and the costs are shared. A type of its own because its
    durations scale the rates as well - a plain HamiltonianSweep stays refused on the Lindblad path.

    hamiltonian, perturbations, offsets, control_scales: as for a HamiltonianSweep.
    rate_scales :: (B, L) real, finite and >= 0 - c_bl, seed b's factor of the l-th dissipation rate,
        L the number of Lindblad operators. Default: every seed takes the rates as given. With them
        the system must be time independent (hamiltonian, drives and lindblad_data): the engine
        holds a time-dependent control-free generator in per-stage tables, one set, not B.

    B is read from whichever of offsets, control_scales and rate_scales is given; they must agree.
    Passed as the `hamiltonian` of grape_lindblad_discrete_batch (B = initial_controls.shape[0]) or of
    LindbladEvaluator (evaluate_batch with a batch of B); the engine expands the seeds on the device
    (qocx_lindblad_set_sweep). The result's sweep_sensitivities holds control_scales
    (B x control_count), offsets (B x J) and rate_scales (B x L) = d error_b / d c_bl, and for a
    duration sweep evolution_time_gradients (B). The last two exist only where the engine's
    sensitivity evaluation ran two-sided, and are None elsewhere: that takes ONE cost, a final
    TargetDensityInfidelity (no step cost, no second cost), 1 to 4 Lindblad operators, a
    time-independent system, and stage values that fit the device memory.
    member(b) and member_lindblad_data(b, lindblad_data) are seed b's system as plain callables,
    slice(lo, hi) the sweep of a contiguous block of seeds.

    LindbladSweep.durations(...) builds the sweep in which seed b runs for its own evolution time,
    LindbladSweep.duration_search(...) the one in which that time is optimised with the pulse.
    """

    def __init__(self, hamiltonian, perturbations=None, offsets=None, control_scales=None,
                 rate_scales=None):
        more = None
        if rate_scales is not None:
            rate_scales = _rate_scales_array(rate_scales)
            more = {"rate_scales": rate_scales.shape[0]}
        HamiltonianSweep.__init__(self, hamiltonian, perturbations, offsets, control_scales,
                                  _more_counts=more)
        self.rate_scales = rate_scales
        self._user_rates = rate_scales   # c0 of time_gradients: the values before tau

    @classmethod
    def durations(cls, hamiltonian, evolution_times, reference_time, control_scales=None,
                  perturbations=None, offsets=None, rate_scales=None, time_bounds=None,
                  time_weight=0.0):
        """
        The sweep in which seed b runs for evolution_times[b]: what HamiltonianSweep.durations
        builds, with rate_scales additionally multiplied by tau_b = T_b / reference_time -

            tau_b * (the whole Lindbladian)  on  [0, reference_time]

        is the open system on [0, T_b], exact for a time-independent system (scaling the
        Lindbladian is scaling time). The caller passes evolution_time = reference_time.
        rate_scales :: (B, L) or None (all 1), before the factor tau_b. Every seed has rates of its
        own here, so the system must be time independent - lindblad_data included.
        time_bounds is a NotImplementedError here: the sweep this constructor builds has its
        per-seed generators fixed by the host. LindbladSweep.duration_search builds the search.
        """
        if time_bounds is not None or time_weight != 0.0:
            raise NotImplementedError(
                "LindbladSweep.durations builds fixed durations: its per-seed generators and "
                "sub-division counts are built on the host from tau_b = T_b / reference_time. "
                "LindbladSweep.duration_search(..., time_bounds, time_weight) builds the search, "
                "whose generators follow tau_b on the device")
        return cls._durations(hamiltonian, evolution_times, reference_time, control_scales,
                              perturbations, offsets, rate_scales, None, 0.0)

    @classmethod
    def duration_search(cls, hamiltonian, evolution_times, reference_time, time_bounds,
                        time_weight=0.0, control_scales=None, perturbations=None, offsets=None,
                        rate_scales=None):
        """
        The duration search of open systems (minimum-time GRAPE under T1 / T2): seed b is

            tau_b * (the whole Lindbladian)  on  [0, reference_time],   tau_b = T_b / reference_time,

        as in LindbladSweep.durations, and tau_b is one more optimised parameter of seed b in
        grape_lindblad_discrete_batch - the last entry of its flat parameter vector on the host
        loop, beside the controls on the device -, clipped in place to time_bounds /
        reference_time every iteration and stepped with the controls' rule and learning rate.
        The error of seed b is E_b(u_b, tau_b) + time_weight * tau_b, the time term one product and
        one sum, added last. Under dissipation E_b has a minimum in T_b of its own, so
        time_weight = 0 already has something to find.

        evolution_times are the STARTING durations; time_bounds = (T_min, T_max) and time_weight as
        in HamiltonianSweep.durations, with the same ValueErrors; control_scales, perturbations,
        offsets and rate_scales are the values before the factor tau_b. member(b) and
        member_lindblad_data(b, .) stay the system at the starting duration.

        The gradient with respect to tau_b needs the rate sensitivities, which exist where the
        evaluation runs two-sided: ONE state cost, a final TargetDensityInfidelity (costs of the
        controls alone may join it), 1 to 4 Lindblad operators, a time-independent system.
        LindbladEvaluator refuses anything else by name. Against LindbladSweep.durations at the
        same durations the search agrees to rounding, not bit for bit: tau * sum (c0 gamma) L^H L
        and sum (tau c0 gamma) L^H L round differently.
        """
        if time_bounds is None:
            raise ValueError("time_bounds must be (T_min, T_max)")
        return cls._durations(hamiltonian, evolution_times, reference_time, control_scales,
                              perturbations, offsets, rate_scales, time_bounds, time_weight)

    @classmethod
    def _durations(cls, hamiltonian, evolution_times, reference_time, control_scales,
                   perturbations, offsets, rate_scales, time_bounds, time_weight):
        self = super(LindbladSweep, cls).durations(hamiltonian, evolution_times, reference_time,
                                                   control_scales, perturbations, offsets,
                                                   time_bounds, time_weight)
        user_rates = None
        if rate_scales is not None:
            user_rates = _rate_scales_array(rate_scales)
            if user_rates.shape[0] != self.seed_count:
                raise ValueError("rate_scales are for {} seeds, evolution_times for {}"
                                 "".format(user_rates.shape[0], self.seed_count))
        self._user_rates = user_rates
        # (rates of all 1 are kept implicit until the operator count is known: resolved_rate_scales)
        self.rate_scales = None if user_rates is None else self._tau[:, None] * user_rates
        return self

    @property
    def has_rates(self):
        """Seed b decays with rates of its own (rate_scales given, or a duration sweep)."""
        return self.rate_scales is not None or self.time_scaled

    def resolved_rate_scales(self, operator_count):
        """c_bl for a problem with this many Lindblad operators, (B, L); None where every seed takes
        the rates as given. A duration sweep without rate_scales has c_bl = tau_b."""
        L = int(operator_count)
        rates = self.rate_scales
        if rates is None:
            if not self.time_scaled:
                return None
            rates = np.repeat(self._tau[:, None], L, axis=1)
        if rates.shape[1] != L:
            raise ValueError("rate_scales must be (B, L) with L = {} Lindblad operators of "
                             "lindblad_data, got shape {}".format(L, rates.shape))
        return rates

    def base_rates(self, operator_count):
        """c0 (B, L) of a duration sweep, its rate factors before the factor tau_b; None for all 1."""
        if not self.time_scaled:
            raise ValueError("base_rates belong to a duration sweep (LindbladSweep.durations)")
        rates = self._user_rates
        if rates is not None and rates.shape[1] != int(operator_count):
            raise ValueError("rate_scales must be (B, L) with L = {} Lindblad operators of "
                             "lindblad_data, got shape {}".format(int(operator_count), rates.shape))
        return None if rates is None else rates.copy()

    def member_lindblad_data(self, b, lindblad_data):
        """Seed b's lindblad_data as a plain callable time -> (c_b * dissipators, operators): the
        problem's own where the sweep has no rates of its own."""
        b = int(b)
        if not 0 <= b < self.seed_count:
            raise IndexError("seed {} out of range for {} seeds".format(b, self.seed_count))
        if not callable(lindblad_data):
            raise ValueError("lindblad_data must be a callable time -> (dissipators, operators)")
        if not self.has_rates:
            return lindblad_data

        def member_data(time):
            dissipators, operators = lindblad_data(time)
            dissipators = np.asarray(dissipators)
            factors = self.resolved_rate_scales(dissipators.shape[0] if dissipators.ndim else 0)
            return factors[b] * dissipators, operators
        return member_data

    def slice(self, lo, hi):
        """The sweep of seeds lo .. hi - 1, rates included (what a rank of a communicator
        evaluates)."""
        out = HamiltonianSweep.slice(self, lo, hi)
        lo, hi = int(lo), int(hi)
        for name in ("rate_scales", "_user_rates"):
            value = getattr(self, name, None)
            if value is not None:
                setattr(out, name, value[lo:hi].copy())
        return out

    def time_gradients(self, scale_sens, offset_sens, rate_sens=None):
        """d error_b / d T_b (B,) of a duration sweep: HamiltonianSweep.time_gradients plus the rate
        part sum_l dE/dc_bl c0_bl / reference_time with c0 the rate factors before tau_b (all 1
        without rate_scales) - c_bl = tau_b c0_bl, so this is sum_l c_bl dE/dc_bl / tau_b /
        reference_time. rate_sens :: (B, L); None or L = 0: no rates, the Hamiltonian part alone."""
        out = HamiltonianSweep.time_gradients(self, scale_sens, offset_sens)
        if rate_sens is None:
            return out
        rate_sens = np.asarray(rate_sens, dtype=np.float64)
        c0 = np.ones_like(rate_sens) if self._user_rates is None else self._user_rates
        if rate_sens.shape != c0.shape:
            raise ValueError("rate sensitivities must be (B, L) = {}, got {}".format(
                c0.shape, rate_sens.shape))
        return out + np.sum(rate_sens * c0, axis=1) / self.reference_time

    def __repr__(self):
        rates = "" if self.rate_scales is None else ", rate_scales {}".format(
            "x".join(str(d) for d in self.rate_scales.shape))
        return "LindbladSweep({!r}, {} seeds, {} fixed matrices{}{})".format(
            self._source if self._source is not None else self.hamiltonian, self.seed_count,
            self.perturbation_count, rates, ", durations" if self.time_scaled else "")


def _rate_scales_array(rate_scales):
    rate_scales = _real_array(rate_scales, "rate_scales", 2)
    if np.any(rate_scales < 0):
        raise ValueError("rate_scales must be >= 0 (they multiply dissipation rates)")
    return rate_scales
