"""
controlbasis.py - a linear map between the optimizer's parameters and the control knots.

The GRAPE drivers optimise one number per control knot. With a ControlBasis they optimise P
coefficients per control instead and evaluate the pulse u = M c, M :: (control_eval_count x P): a
few smooth basis functions (ControlBasis.sine: zero at both ends), or a pulse as it leaves the
transfer function of a signal generator (ControlBasis.gaussian_filter). The gradient of the error in
the coefficients is M^T (d error / d u).

Both directions run in ONE defined order, which the device kernels of qoc_amd/csrc/qocx_ctrlbasis.hip
follow, so that the host loop and the device-resident loop give the same bits:
  expand   u[j, k] = sum over p = 0 .. P-1 in increasing order, acc = acc + M[j, p] * c[p, k]
  project  h[p, k] = sum over j = 0 .. Nc-1 in increasing order, acc = acc + M[j, p] * g[j, k]
starting from +0.0, the product and the sum each rounded on its own (no fused multiply-add). A
complex array maps its real and its imaginary part separately through the same real matrix.
"""

import numpy as np


class ControlBasis(object):
    """
    matrix :: (control_eval_count x P) real and finite, P >= 1: column p is basis function p at the
    control knots. Fields: matrix, knot_count (control_eval_count), coefficient_count (P).
    """

    def __init__(self, matrix):
        matrix = np.asarray(matrix)
        if matrix.ndim != 2 or matrix.shape[0] < 1 or matrix.shape[1] < 1:
            raise ValueError("ControlBasis: matrix must be (control_eval_count x P) with P >= 1, "
                             "got shape {}".format(matrix.shape))
        if np.iscomplexobj(matrix) or not (np.issubdtype(matrix.dtype, np.floating)
                                           or np.issubdtype(matrix.dtype, np.integer)):
            raise ValueError("ControlBasis: matrix must be real")
        matrix = np.array(matrix, dtype=np.float64)  # a private, contiguous copy
        if not np.isfinite(matrix).all():
            raise ValueError("ControlBasis: matrix must be finite")
        matrix.setflags(write=False)
        self.matrix = matrix
        self.knot_count = int(matrix.shape[0])
        self.coefficient_count = int(matrix.shape[1])

    def __repr__(self):
        return "ControlBasis({} knots, {} coefficients)".format(self.knot_count,
                                                                self.coefficient_count)

    # ---- the two maps ---------------------------------------------------------------------------
    def _expand_real(self, c):
        m = self.matrix
        acc = np.zeros(c.shape[:-2] + (self.knot_count, c.shape[-1]))
        for p in range(self.coefficient_count):
            acc = acc + m[:, p][:, None] * c[..., p, :][..., None, :]
        return acc

    def _project_real(self, g):
        m = self.matrix
        acc = np.zeros(g.shape[:-2] + (self.coefficient_count, g.shape[-1]))
        for j in range(self.knot_count):
            acc = acc + m[j, :][:, None] * g[..., j, :][..., None, :]
        return acc

    @staticmethod
    def _by_parts(real_map, array, rows, what):
        array = np.asarray(array)
        if array.ndim < 2 or array.shape[-2] != rows:
            raise ValueError("ControlBasis: {} must be (... x {} x control_count), got shape {}"
                             "".format(what, rows, array.shape))
        if np.iscomplexobj(array):
            real = real_map(np.asarray(array.real, dtype=np.float64))
            out = np.empty(real.shape, dtype=np.complex128)
            out.real = real
            out.imag = real_map(np.asarray(array.imag, dtype=np.float64))
            return out
        return real_map(np.asarray(array, dtype=np.float64))

    def expand(self, coefficients):
        """coefficients (... x P x control_count), real or complex -> the pulse
        (... x control_eval_count x control_count), a new array."""
        return self._by_parts(self._expand_real, coefficients, self.coefficient_count,
                              "coefficients")

    def project(self, grads):
        """grads (... x control_eval_count x control_count) -> (... x P x control_count): the
        transpose map, which takes d error / d controls to d error / d coefficients."""
        return self._by_parts(self._project_real, grads, self.knot_count, "grads")

    def fit(self, controls):
        """Least-squares coefficients (... x P x control_count) of a given pulse
        (... x control_eval_count x control_count): a start for the drivers from an existing pulse."""
        controls = np.asarray(controls)
        if controls.ndim < 2 or controls.shape[-2] != self.knot_count:
            raise ValueError("ControlBasis: controls must be (... x {} x control_count), got shape "
                             "{}".format(self.knot_count, controls.shape))
        lead = np.moveaxis(controls, -2, 0)
        columns = lead.reshape(self.knot_count, -1)
        matrix = self.matrix.astype(columns.dtype) if np.iscomplexobj(columns) else self.matrix
        solution = np.linalg.lstsq(matrix, columns, rcond=None)[0]
        solution = solution.reshape((self.coefficient_count,) + lead.shape[1:])
        return np.ascontiguousarray(np.moveaxis(solution, 0, -2))

    # ---- constructors ---------------------------------------------------------------------------
    @classmethod
    def sine(cls, control_eval_count, count):
        """Columns sin(pi p j / (Nc - 1)), p = 1 .. count, at the knots j = 0 .. Nc - 1: every pulse
        is exactly zero at both ends."""
        control_eval_count, count = int(control_eval_count), int(count)
        if control_eval_count < 2 or count < 1:
            raise ValueError("ControlBasis.sine needs control_eval_count >= 2 and count >= 1")
        j = np.arange(control_eval_count, dtype=np.float64)[:, None]
        p = np.arange(1, count + 1, dtype=np.float64)[None, :]
        matrix = np.sin(np.pi * p * j / (control_eval_count - 1))
        matrix[0, :] = 0.0   # (sin(pi p) in floating point is a rounding error, not zero)
        matrix[-1, :] = 0.0
        return cls(matrix)

    @classmethod
    def gaussian_filter(cls, control_eval_count, sigma):
        """P = Nc: knot j is the Gaussian average, of width sigma knots, of the coefficients around
        j, every row normalised to sum 1 - a band-limited signal generator."""
        control_eval_count, sigma = int(control_eval_count), float(sigma)
        if control_eval_count < 1 or not (sigma > 0) or not np.isfinite(sigma):
            raise ValueError("ControlBasis.gaussian_filter needs control_eval_count >= 1 and a "
                             "finite sigma > 0")
        j = np.arange(control_eval_count, dtype=np.float64)
        matrix = np.exp(-0.5 * np.square((j[:, None] - j[None, :]) / sigma))
        matrix = matrix / np.sum(matrix, axis=1)[:, None]
        return cls(matrix)
