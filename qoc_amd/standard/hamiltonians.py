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
