"""
hamiltonians.py - Hamiltonians whose structure the engine can use beyond linearity.

QuadraticHamiltonian is a `hamiltonian(controls, time)` callable like any other (every entry
point and the oracle take it as such). Its type tells the Schroedinger evaluator that

    H(r, t) = H0(t) + sum_k r_k G_k(t) + sum_(k <= l) r_k r_l Q_kl

in the real controls r, so under MagnusPolicy.M2 the engine evaluates it on the device as a
problem linear in the effective controls (r_k, r_k r_l) - no call of the callable per step or
per evaluation (qocx_set_quadratic_terms). The Piccolo Hamiltonian of the reference's report
(report.tex:22-32, an AC-Stark term in epsilon_sb^2) has this form.
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
