"""
controlcosts.py - the four built-in costs that depend on the controls only.

Values follow qoc/standard/costs/controlnorm.py:48-73, controlvariation.py:47-75,
controlarea.py:43-67 and controlbandwidthmax.py:52-77: O(control_eval_count * control_count)
NumPy, with closed-form `controls_bar` in qoc's gradient convention (d/dRe + i d/dIm for complex
controls) in place of autograd. The single-seed drivers and evaluate_batch call these on the host.

The device-resident multi-start drivers evaluate the same formulas on the GPU
(qoc_amd/csrc/qocx_ctrlcost.hip): `control_descriptor(control_count, control_eval_count,
complex_controls)` returns the dict engine.set_control_costs() takes - or None when the host must
keep the cost so that its Python behaviour survives (shapes that do not match the problem, the
NameError of ControlArea without max_control_norms, a bandwidth cost without penalised bins).
"""

import numpy as np

from qoc_amd.engine import (CONTROL_AREA, CONTROL_BANDWIDTH_MAX, CONTROL_NORM,
                            CONTROL_VARIATION)
from qoc_amd.models.cost import Cost


def _abs2(z):
    return np.real(z * np.conjugate(z))


def _match_dtype(grad, controls):
    return grad if np.iscomplexobj(controls) else np.real(grad)


def _per_control(values, control_count):
    """`values` as a float64 (control_count,) array; None if absent; False if it has another
    shape or is not real (the host keeps such a cost)."""
    if values is None:
        return None
    array = np.asarray(values)
    if array.shape != (control_count,) or not np.isrealobj(array) or array.dtype == object:
        return False
    return np.array(array, dtype=np.float64)


class ControlNorm(Cost):
    """Mean squared modulus of the (normalised, weighted) controls."""
    name = "control_norm"
    requires_step_evaluation = False
    uses_states = False

    def __init__(self, control_count, control_eval_count, control_weights=None,
                 cost_multiplier=1., max_control_norms=None):
        super().__init__(cost_multiplier=cost_multiplier)
        self.control_weights = control_weights
        self.controls_size = control_eval_count * control_count
        self.max_control_norms = max_control_norms

    def cost(self, controls, states, system_eval_step):
        if self.max_control_norms is not None:
            controls = controls / self.max_control_norms
        if self.control_weights is not None:
            controls = controls[:, ] * self.control_weights
        return np.sum(_abs2(controls)) / self.controls_size * self.cost_multiplier

    def controls_bar(self, controls, states, system_eval_step):
        factor = np.ones(controls.shape[1])
        if self.max_control_norms is not None:
            factor = factor / self.max_control_norms
        if self.control_weights is not None:
            factor = factor * self.control_weights
        return (2 * self.cost_multiplier / self.controls_size) * controls * factor ** 2

    def control_descriptor(self, control_count, control_eval_count, complex_controls):
        max_norms = _per_control(self.max_control_norms, control_count)
        weights = _per_control(self.control_weights, control_count)
        if (max_norms is False or weights is False
                or self.controls_size != control_eval_count * control_count):
            return None
        return dict(kind=CONTROL_NORM, multiplier=self.cost_multiplier / self.controls_size,
                    max_norms=max_norms, weights=weights)


class ControlVariation(Cost):
    """Mean squared modulus of the order-n finite differences of the controls."""
    name = "control_variation"
    requires_step_evaluation = False
    uses_states = False

    def __init__(self, control_count, control_eval_count, cost_multiplier=1.,
                 max_control_norms=None, order=1):
        super().__init__(cost_multiplier=cost_multiplier)
        self.max_control_norms = max_control_norms
        self.diffs_size = control_count * (control_eval_count - order)
        self.order = order
        self.cost_normalization_constant = self.diffs_size * (2 ** self.order)

    def _normalised(self, controls):
        if self.max_control_norms is not None:
            return controls / self.max_control_norms
        return controls

    def cost(self, controls, states, system_eval_step):
        diffs = np.diff(self._normalised(controls), axis=0, n=self.order)
        return np.sum(_abs2(diffs)) / self.cost_normalization_constant * self.cost_multiplier

    def controls_bar(self, controls, states, system_eval_step):
        back = (2 * self.cost_multiplier / self.cost_normalization_constant) * np.diff(
            self._normalised(controls), axis=0, n=self.order)
        for _ in range(self.order):  # transpose of one forward difference
            grown = np.zeros((back.shape[0] + 1, back.shape[1]), dtype=back.dtype)
            grown[1:] += back
            grown[:-1] -= back
            back = grown
        return self._normalised(back)

    def control_descriptor(self, control_count, control_eval_count, complex_controls):
        max_norms = _per_control(self.max_control_norms, control_count)
        order = self.order
        if (max_norms is False or not isinstance(order, (int, np.integer))
                or not 1 <= order < control_eval_count
                or self.diffs_size != control_count * (control_eval_count - order)):
            return None
        return dict(kind=CONTROL_VARIATION, order=int(order), max_norms=max_norms,
                    multiplier=self.cost_multiplier / self.cost_normalization_constant)


class ControlArea(Cost):
    """Modulus of the discrete integral of each normalised control."""
    name = "control_area"
    requires_step_evaluation = False
    uses_states = False

    def __init__(self, control_count, control_eval_count, cost_multiplier=1.,
                 max_control_norms=None):
        super().__init__(cost_multiplier=cost_multiplier)
        self.control_count = control_count
        self.control_size = control_count * control_eval_count
        self.max_control_norms = max_control_norms

    def cost(self, controls, states, system_eval_step):
        if self.max_control_norms is None:
            # the reference reads an unbound local here (controlarea.py:58 vs :64)
            raise NameError("name 'normalized_controls' is not defined")
        normalized_controls = controls / self.max_control_norms
        total = 0
        for i in range(self.control_count):
            total = total + np.abs(np.sum(normalized_controls[:, i]))
        return total / self.control_size * self.cost_multiplier

    def controls_bar(self, controls, states, system_eval_step):
        sums = np.sum(controls / self.max_control_norms, axis=0)
        moduli = np.abs(sums)
        direction = np.where(moduli > 0, sums / np.where(moduli > 0, moduli, 1), 0)
        row = (self.cost_multiplier / self.control_size) * direction / self.max_control_norms
        return _match_dtype(np.tile(row, (controls.shape[0], 1)), controls)

    def control_descriptor(self, control_count, control_eval_count, complex_controls):
        max_norms = _per_control(self.max_control_norms, control_count)
        if (max_norms is None or max_norms is False or self.control_count != control_count
                or self.control_size != control_count * control_eval_count):
            return None  # (without max_control_norms cost() raises the reference's NameError)
        return dict(kind=CONTROL_AREA, multiplier=self.cost_multiplier / self.control_size,
                    max_norms=max_norms)


class ControlBandwidthMax(Cost):
    """Spectral weight of each control above its maximum bandwidth.

    The sample spacing of the DFT is taken from the `evolution_time` given HERE:
    evolution_time / (control_eval_count - 1), the knot spacing of InterpolationPolicy.LINEAR.
    Under InterpolationPolicy.PIECEWISE_CONSTANT the rows are T / control_eval_count apart: pass
    evolution_time = T (control_eval_count - 1) / control_eval_count for frequencies in the same
    units."""
    name = "control_bandwidth_max"
    requires_step_evaluation = False
    uses_states = False

    def __init__(self, control_count, control_eval_count, evolution_time, max_bandwidths,
                 cost_multiplier=1.):
        super().__init__(cost_multiplier=cost_multiplier)
        self.max_bandwidths = max_bandwidths
        self.control_count = control_count
        dt = evolution_time / (control_eval_count - 1)
        self.freqs = np.fft.fftfreq(control_eval_count, d=dt)

    def cost(self, controls, states, system_eval_step):
        total = 0
        for i, max_bandwidth in enumerate(self.max_bandwidths):
            magnitudes = np.abs(np.fft.fft(controls[:, i]))
            penalised = magnitudes[np.nonzero(self.freqs >= max_bandwidth)[0]]
            total = total + np.sum(penalised) / (penalised.shape[0] * np.max(penalised))
        return total / self.control_count * self.cost_multiplier

    def controls_bar(self, controls, states, system_eval_step):
        count = controls.shape[0]
        out = np.zeros(controls.shape, dtype=np.complex128)
        for i, max_bandwidth in enumerate(self.max_bandwidths):
            spectrum = np.fft.fft(controls[:, i])
            magnitudes = np.abs(spectrum)
            index = np.nonzero(self.freqs >= max_bandwidth)[0]
            penalised = magnitudes[index]
            top = np.max(penalised)
            weight = np.zeros(count)
            weight[index] = 1.0 / (index.shape[0] * top)
            weight[index[int(np.argmax(penalised))]] -= np.sum(penalised) / (index.shape[0] * top * top)
            spectrum_bar = weight * spectrum / np.where(magnitudes > 0, magnitudes, 1)
            out[:, i] = np.fft.ifft(spectrum_bar) * count * (self.cost_multiplier / self.control_count)
        return _match_dtype(out, controls)

    def control_descriptor(self, control_count, control_eval_count, complex_controls):
        bandwidths = _per_control(self.max_bandwidths, control_count)
        if (bandwidths is None or bandwidths is False or self.control_count != control_count
                or self.freqs.shape[0] != control_eval_count):
            return None
        bins = [np.nonzero(self.freqs >= b)[0].astype(np.int32) for b in bandwidths]
        if any(len(b) == 0 for b in bins):
            return None  # (numpy.max of an empty array raises in cost())
        return dict(kind=CONTROL_BANDWIDTH_MAX, bins=bins,
                    multiplier=self.cost_multiplier / self.control_count)
