"""
CPU tests of the two host functions behind the degrees of the matrix-free route, through the library's
context-free debug entry points (no GPU call): qocx_debug_spectral_bound - an upper bound of the spectral
radius of a Hermitian matrix, never below it and at most 1 % above - against numpy.linalg.eigvalsh, and
qocx_debug_action_degree - qoc_amd/csrc/qocx_action.h's action_degree_rule - against its NumPy twin
(tests/action_degree_model.py).
"""

import ctypes

import numpy as np
import pytest

from qoc_amd import engine
from tests import action_degree_model as dm
from tests import action_model as am


def spectral_bound(m):
    lib = engine.load_library()
    m = np.ascontiguousarray(m, dtype=np.complex128)
    out = ctypes.c_double(-1.0)
    rc = lib.qocx_debug_spectral_bound(m.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                       m.shape[0], ctypes.byref(out))
    assert rc == 0
    return out.value


def gue(rng, n):
    g = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    return (g + g.conj().T) / 2


def rotated(rng, eigenvalues):
    """A Hermitian matrix with the given spectrum in a random basis."""
    n = len(eigenvalues)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    m = (q * np.asarray(eigenvalues, dtype=np.float64)) @ q.conj().T
    return (m + m.conj().T) / 2


def cases():
    rng = np.random.default_rng(11)
    out = [("gue n=%d" % n, gue(rng, n)) for n in (1, 2, 17, 32, 33, 64)]
    out.append(("diagonal", np.diag(rng.standard_normal(20)).astype(np.complex128)))
    v = rng.standard_normal(24) + 1j * rng.standard_normal(24)
    out.append(("rank one", -np.outer(v, v.conj())))
    out.append(("degenerate top pair", rotated(rng, [2.5, -2.5] + list(rng.uniform(-2.4, 2.4, 28)))))
    out.append(("flat spectrum", rotated(rng, rng.choice([-1.0, 1.0], 64))))  # the largest overshoot: n^(1/512)
    out.append(("scaled 1e-150", 1e-150 * gue(rng, 32)))
    out.append(("scaled 1e150", 1e150 * gue(rng, 32)))
    return out


@pytest.mark.parametrize("name,m", cases(), ids=[c[0] for c in cases()])
def test_spectral_bound_is_above_the_spectral_radius_and_within_one_percent(name, m):
    rho = float(np.abs(np.linalg.eigvalsh(m)).max())
    bound = spectral_bound(m)
    print("{}: rho {:.6e} bound {:.6e} ratio - 1 = {:.3e}".format(name, rho, bound, bound / rho - 1))
    assert rho <= bound <= 1.01 * rho


def test_spectral_bound_of_the_zero_matrix_is_zero():
    for n in (1, 17, 64):
        assert spectral_bound(np.zeros((n, n))) == 0.0


def test_spectral_bound_of_a_non_finite_matrix_is_not_finite():
    """The engine then keeps the 1-norm (which refuses the problem as it always did)."""
    m = gue(np.random.default_rng(3), 8)
    for bad in (np.nan, np.inf):
        x = m.copy()
        x[2, 5] = x[5, 2] = bad
        assert not np.isfinite(spectral_bound(x))


def test_spectral_bound_rejects_sizes_it_was_not_written_for():
    lib = engine.load_library()
    out = ctypes.c_double(0.0)
    m = np.zeros(2 * 65 * 65)
    for n in (0, 65):
        assert lib.qocx_debug_spectral_bound(m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n,
                                             ctypes.byref(out)) != 0


def native_degree(bound1, bound2, rule):
    lib = engine.load_library()
    out = ctypes.c_int32(-1)
    assert lib.qocx_debug_action_degree(float(bound1), float(bound2), rule, ctypes.byref(out)) == 0
    return out.value


def test_native_degree_rule_equals_the_numpy_twin():
    edges = []
    for table in (am.THETA, dm.THETA_NORMAL):
        for th in table.values():
            edges += [th, float(np.nextafter(th, 0.0)), float(np.nextafter(th, np.inf)), 0.98 * th, 1.02 * th]
    rng = np.random.default_rng(9)
    grid = np.concatenate([edges, 10.0 ** rng.uniform(-17, 0.5, 300), [0.0, 1.09, 1.2, 5.0, np.inf, np.nan]])
    for rule in (0, 1):
        for b1 in grid:
            for b2 in (b1, 0.31 * b1, 0.999 * b1, np.nan):
                assert native_degree(b1, b2, rule) == dm.degree_rule(b1, b2, rule), (b1, b2, rule)
        for b2 in edges:  # the second table's edges under a 1-norm bound three times as large
            assert native_degree(3.0 * b2, b2, rule) == dm.degree_rule(3.0 * b2, b2, rule), (b2, rule)
    out = ctypes.c_int32(0)
    assert engine.load_library().qocx_debug_action_degree(0.1, 0.1, 2, ctypes.byref(out)) != 0


def test_the_knob_is_a_variant_knob_of_the_product_library():
    assert engine.load_library().qocx_knob_kind(b"action_degree") == 1
