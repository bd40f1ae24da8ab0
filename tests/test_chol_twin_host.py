"""CPU tests of ``tests/chol_twin.py``, the long-double truth of the blocked Cholesky solver's GPU tests
(``test_gpu_chol_blocked.py``): the twin against ``numpy.linalg.cholesky``, its closed-form small-order path against the
general one, and the float64 reference solve inside both acceptance bounds at every shape of the sweep, so that the
inputs (``cond`` in 1e2, 1e6, 1e10, fixed seeds) are known to be fair before a GPU sees them.

Measured here, the float64 reference over the whole sweep: ``e_ref`` between 0 (order 1, ``cond = 1e6``) and 9.0e-8 (orders
96 and 257, ``cond = 1e10``); the worst residual / bound 0.46 (order 1, where the bound is 8 u), 0.086 at order 2, 0.0010
at order 257; ``e_ref_U`` at most 5.0e-16 at ``cond = 1e2`` and 1.2e-11 at ``1e10``.  The per-case figures are tabulated in
``test_gpu_chol_blocked.py`` beside the GPU's.
"""

import numpy as np
import pytest

import chol_twin as ct


@pytest.fixture(scope="module")
def cases():
    return {shape: ct.Case(*shape) for shape in ct.SWEEP}


@pytest.mark.parametrize("shape", ct.SWEEP, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_inside_bounds(cases, shape):
    """``solve_f64`` passes the backward and the forward assertion, and the twin's factor is numpy's to rounding."""
    c = cases[shape]
    n = c.n
    for t in range(c.nmat):
        e, ratio = c.measure(t, c.x_ref[t])
        print(f"chol twin {shape} cond {ct.CONDS[t]:.0e}: e_ref {e:.3e} residual / bound {ratio:.3e} e_ref_U {c.e_ref_u[t]:.3e}")
        assert np.isfinite(c.x_ref[t]).all()
        assert ratio <= 1.0, (shape, t, ratio)
        assert e == c.e_ref[t] and e <= ct.forward_limit(c.e_ref[t], n)
        # the twin reproduces numpy's factor to n 2**-52 of the largest entry where the rounding of G itself moves the
        # factor by less than that (cond = 1e2); at 1e6 and 1e10 numpy's own factor is cond x u away from the truth
        # (e_ref_U, printed above), so there the twin is checked as a factor of G instead
        if ct.CONDS[t] == 1e2:
            umax = float(np.abs(c.U[t]).max())
            assert np.abs(c.u_ref[t] - c.U[t].astype(np.float64)).max() <= n * 2.0**-52 * umax
        # |U^T U - G| <= gamma_{n+1} |U|^T |U| holds for a float64 factorisation, the
        # long-double one is far inside it at every condition number
        uu = c.U[t]
        g = np.triu(c.G[t]).astype(ct.LD)
        g = g + np.triu(g, 1).T
        assert np.all(np.abs(uu.T @ uu - g) <= ct.LD(ct.gamma(n + 1)) * (np.abs(uu).T @ np.abs(uu)))
        assert not np.tril(uu, -1).any()


def test_twin_against_numpy_well_conditioned():
    """At ``cond = 1e2`` the rounding of G moves the factor by less than one unit: the twin and numpy agree to ``n
    2**-52`` of the largest entry, outright."""
    for n in (1, 2, 33, 97, 257):
        rng = np.random.default_rng(n)
        g = ct.spd(n, 1e2, rng)
        u = ct.chol_upper_ld(g).astype(np.float64)
        assert np.abs(u - np.linalg.cholesky(g).T).max() <= n * 2.0**-52 * np.abs(u).max()


def test_upper_triangle_only():
    """The twin reads the upper triangle alone: NaN below the diagonal changes nothing."""
    c = ct.Case(33, 2)
    for g, u in zip(c.poisoned(), c.U):
        assert np.array_equal(ct.chol_upper_ld(g), u)
        assert np.isfinite(ct.residual(g, c.x_ref[0], c.Y[0]).astype(np.float64)).all()


def test_spd_properties():
    rng = np.random.default_rng(5)
    for n, cond in ((1, 1e6), (2, 1e2), (65, 1e10)):
        g = ct.spd(n, cond, rng)
        assert g.dtype == np.float64 and np.array_equal(g, g.T)
        lam = np.linalg.eigvalsh(g)
        assert lam[0] > 0.5 and (n == 1 or abs(lam[-1] / lam[0] / cond - 1.0) < 1e-3)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_small_closed_form(n):
    """The closed-form path is the general substitution, operation for operation."""
    c = ct.Case(n, 300, conds=(1e2, 1e10))
    for u, y, x in zip(c.U, c.Y, c.X):
        assert np.array_equal(ct.solve_rows_small_ld(u, y), x)


def test_schur_pivot():
    rng = np.random.default_rng(97)
    g = ct.spd(97, 1e6, rng)
    u = ct.chol_upper_ld(g)
    for j in (0, 40, 96):
        s = ct.schur_pivot_ld(g, j)
        assert abs(float(s / (u[j, j] * u[j, j])) - 1.0) < 1e-15
    g[96, 96] = float(ct.LD(g[96, 96]) - ct.schur_pivot_ld(g, 96) - 1)
    assert abs(float(ct.schur_pivot_ld(g, 96)) + 1.0) < 1e-6
    with pytest.raises(np.linalg.LinAlgError, match="pivot 96"):
        ct.chol_upper_ld(g)


def test_bound_catches_a_lost_term():
    """A solution that is wrong by one part in 1e10 in one component, the size of error the task-level tests cannot
    see, is far outside the backward bound at every conditioning of the sweep."""
    c = ct.Case(33, 4)
    for t in range(c.nmat):
        x = c.x_ref[t].copy()
        k = int(np.argmax(np.abs(x[0])))
        x[0, k] *= 1.0 + 1e-10
        assert c.measure(t, x)[1] > 10.0
