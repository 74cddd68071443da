"""
control_cost_model.py - a NumPy restatement of the device arithmetic of the costs of the controls
alone (qoc_amd/csrc/qocx_ctrlcost.hip) and of the complex clip of the resident drivers
(qocx_optim.hip: clip_complex_kernel).

Controls are in the engine's layout, real (Nc x Kr) arrays in which a complex control k is the
channels 2k (Re) and 2k + 1 (Im); descriptors are the dicts of control_descriptor(). Elementwise
expressions are written in the kernel's operation order, sums over a seed in the kernel's order
(256 strided partial sums, then a binary tree), and the bandwidth cost as its two products with the
|P| x Nc matrix of twiddles taken from one table at the reduced phases (j f) mod Nc. It pins the
formulas without a GPU: tests compare it with cost() / controls_bar() of the Python classes, and it
stands in for the engine in the host tests of the resident drivers.
"""

import numpy as np

from qoc_amd.engine import (CONTROL_AREA, CONTROL_BANDWIDTH_MAX, CONTROL_NORM,
                            CONTROL_VARIATION)

THREADS = 256


def block_sum(values):
    """Sum of a flat array as a 256-thread workgroup forms it: thread t adds the elements t,
    t + 256, ... in order, then the partial sums meet in a binary tree."""
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    padded = np.zeros((-(-max(values.size, 1) // THREADS)) * THREADS)
    padded[:values.size] = values
    part = np.zeros(THREADS)
    for row in padded.reshape(-1, THREADS):
        part = part + row
    s = THREADS // 2
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def pairwise_sum(x):
    """One part (Re or Im) of a contiguous complex array summed as NumPy's add reduction does it:
    up to 64 entries in four strided partial sums plus a tail, longer ranges split at
    (len - len % 8) / 2."""
    n = len(x)
    if n < 4:
        r = 0.0
        for v in x:
            r = r + v
        return r
    if n <= 64:
        r, i = [x[0], x[1], x[2], x[3]], 4
        while i < n - n % 4:
            r = [r[j] + x[i + j] for j in range(4)]
            i += 4
        out = (r[0] + r[1]) + (r[2] + r[3])
        for v in x[i:]:
            out = out + v
        return out
    half = (n - n % 8) // 2
    return pairwise_sum(x[:half]) + pairwise_sum(x[half:])


def _quotient(u, mx, cplx):
    return u * (1.0 / mx) if cplx else u / mx


def _per_channel(values, K, cplx):
    values = np.ones(K) if values is None else np.asarray(values, dtype=np.float64)
    return np.repeat(values, 2) if cplx else values


def twiddles(nc):
    """exp(-2 pi i m / nc), m = 0 .. nc - 1, rounded from extended precision."""
    two_pi = 2 * np.arccos(np.longdouble(-1))
    theta = two_pi * np.arange(nc, dtype=np.longdouble) / np.longdouble(nc)
    return np.cos(theta).astype(np.float64) - 1j * np.sin(theta).astype(np.float64)


def _bandwidth(u, desc, cplx, want_grad):
    nc, kr = u.shape
    K = kr // 2 if cplx else kr
    table = twiddles(nc)
    total = 0.0
    grad = np.zeros_like(u)
    for k in range(K):
        bins = np.asarray(desc["bins"][k], dtype=np.int64)
        tw = table[(bins[:, None] * np.arange(nc)[None, :]) % nc]  # |P| x Nc
        if cplx:
            a, b = tw @ u[:, 2 * k], tw @ u[:, 2 * k + 1]
            x = (a.real - b.imag) + 1j * (a.imag + b.real)
        else:
            x = tw @ u[:, k]
        mag = np.hypot(x.real, x.imag)
        top, arg = np.max(mag), int(np.argmax(mag))
        summed = block_sum(mag)
        scale = len(bins) * top
        total = total + summed / scale
        if want_grad:
            w = np.full(len(bins), 1.0 / scale)
            w[arg] = 1.0 / scale - summed / (scale * top)
            ybar = (w * x) * (1.0 / np.where(mag > 0, mag, 1.0))
            back = np.conj(tw).T @ ybar  # Nc
            if cplx:
                grad[:, 2 * k] = back.real * desc["multiplier"]
                grad[:, 2 * k + 1] = back.imag * desc["multiplier"]
            else:
                grad[:, k] = back.real * desc["multiplier"]
    return total * desc["multiplier"], grad


def control_costs(controls, descriptors, complex_controls, want_grad=True):
    """(sum of the control costs, its gradient (Nc x Kr) or None) of ONE control set: first the
    descriptors of the seed kernel in their order, then the bandwidth costs in theirs."""
    u = np.asarray(controls, dtype=np.float64)
    nc, kr = u.shape
    cplx = bool(complex_controls)
    K = kr // 2 if cplx else kr
    total, grad = 0.0, np.zeros_like(u)
    for d in descriptors:
        mult = d["multiplier"]
        mx = _per_channel(d.get("max_norms"), K, cplx)
        if d["kind"] == CONTROL_NORM:
            w = _per_channel(d.get("weights"), K, cplx)
            x = _quotient(u, mx, cplx) * w
            total = total + block_sum(x * x) * mult
            f = (1.0 / mx) * w
            grad = grad + ((2.0 * mult) * u) * (f * f)
        elif d["kind"] == CONTROL_VARIATION:
            diffs = _quotient(u, mx, cplx)
            for _ in range(d["order"]):
                diffs = diffs[1:] - diffs[:-1]
            total = total + block_sum(diffs * diffs) * mult
            back = (2.0 * mult) * diffs
            for _ in range(d["order"]):
                grown = np.zeros((back.shape[0] + 1, kr))
                grown[1:] = back
                grown[:-1] = grown[:-1] - back
                back = grown
            grad = grad + _quotient(back, mx, cplx)
        elif d["kind"] == CONTROL_AREA:
            x = _quotient(u, mx, cplx)
            if cplx and kr == 2:  # one contiguous complex column: NumPy sums it pairwise
                sums = np.array([pairwise_sum(x[:, 0]), pairwise_sum(x[:, 1])])
            else:  # knot by knot, as numpy.sum(..., axis=0) adds the rows
                sums = np.zeros(kr)
                for row in x:
                    sums = sums + row
            mod = np.repeat(np.hypot(sums[0::2], sums[1::2]), 2) if cplx else np.abs(sums)
            area = 0.0
            for m in (mod[0::2] if cplx else mod):
                area = area + m
            total = total + area * mult
            direction = np.where(mod > 0, _quotient(sums, np.where(mod > 0, mod, 1.0), cplx), 0.0)
            grad = grad + np.tile(_quotient(mult * direction, mx, cplx), (nc, 1))
    for d in descriptors:
        if d["kind"] == CONTROL_BANDWIDTH_MAX:
            value, g = _bandwidth(u, d, cplx, want_grad)
            total = total + value
            grad = grad + g
    return total, (grad if want_grad else None)


def clip_complex(params, max_norms):
    """(..., 2K) parameters -> the controls the resident drivers evaluate: every complex control
    clipped by its modulus, the parameters untouched."""
    params = np.asarray(params, dtype=np.float64)
    out = params.copy()
    re, im = params[..., 0::2], params[..., 1::2]
    mod = np.hypot(re, im)
    mx = np.broadcast_to(np.asarray(max_norms, dtype=np.float64), mod.shape)
    over = mx < mod
    inv = 1.0 / np.where(over, mod, 1.0)
    out[..., 0::2] = np.where(over, (re * inv) * mx, re)
    out[..., 1::2] = np.where(over, (im * inv) * mx, im)
    return out
