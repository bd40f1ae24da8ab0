"""Covariance kernels of the Gaussian-process regridder and their band forms (``draco/util/kernels.py``).

NumPy on the host, written from the kernels' definitions with the reference's signatures.  The device evaluates the
same expressions (``csrc/gp.hip``, ``dmm_gp_fill``) for products of ``gaussian``, ``rational`` and ``matern`` kernels;
``periodic`` and ``moving_average`` exist here only.

``pair_kernel`` is the element-wise form, ``k(x[i], y[i])`` instead of the matrix ``k(x[i], y[j])``, with the same
floating-point expressions: the host decides the band height of a day's kernel matrix from it without forming the matrix.
"""

from __future__ import annotations

import warnings

import numpy as np
from scipy import linalg as la

__all__ = [
    "convert_band_diagonal",
    "euclidean_difference_kernel",
    "gaussian_kernel",
    "get_kernel",
    "is_hermitian_positive_definite",
    "matern_kernel",
    "moving_average_inverse_kernel",
    "pair_kernel",
    "periodic_kernel",
    "rational_kernel",
    "squared_difference_kernel",
]

DEVICE_KERNELS = ("gaussian", "rational", "matern")


def get_kernel(name, **kernel_params):
    """A covariance matrix by name: ``gaussian``, ``rational``, ``matern``, ``periodic`` or ``moving_average``.

    A full matrix is returned whatever ``banded`` says (the keyword is no longer used); see
    :func:`convert_band_diagonal`.
    """
    if "banded" in kernel_params:
        warnings.warn("The `banded` keyword is not longer used")
    funcs = {
        "gaussian": gaussian_kernel,
        "rational": rational_kernel,
        "matern": matern_kernel,
        "periodic": periodic_kernel,
        "moving_average": moving_average_inverse_kernel,
    }
    func = funcs.get(name.lower())
    if func is None:
        raise ValueError(f"Invalid kernel type: '{name}'. Valid kernels: {list(funcs.keys())}")
    return func(**kernel_params)


# ---------------------------------------------------------------------------------------------------------- kernels
def _gaussian(sq, alpha):
    return (alpha**2) * np.exp(-0.5 * sq)


def _rational(sq, alpha, a):
    return (alpha**2) * (1 + sq / (2 * a)) ** -a


def _matern(dist, alpha, nu):
    """Matern covariance of the scaled distance ``dist`` (which is overwritten) for nu = 3/2 or 5/2."""
    if nu not in {1.5, 2.5}:
        raise ValueError(f"Invalid value `nu`={nu}. Only values of (1.5, 2.5) are currently supported.")
    if nu == 1.5:
        dist *= np.sqrt(3)
        C = 1.0 + dist
    else:
        dist *= np.sqrt(5)
        C = 1.0 + dist + dist**2 / 3.0
    C *= np.exp(-dist)
    C *= alpha**2
    return C


def gaussian_kernel(N, width, alpha, **kwargs):
    """``alpha^2 exp(-d^2 / 2)``, ``d`` the separation in units of ``width``; shape ``(N[0], N[1])``.

    ``N``: a count (samples ``0 ... N - 1``), an array of positions, or a pair of either for a cross-covariance.
    """
    return _gaussian(squared_difference_kernel(N, width), alpha)


def rational_kernel(N, width, alpha, a, **kwargs):
    """Rational quadratic kernel ``alpha^2 (1 + d^2 / (2 a))^-a``."""
    return _rational(squared_difference_kernel(N, width), alpha, a)


def matern_kernel(N, width, alpha, nu, **kwargs):
    """Matern kernel for ``nu`` = 1.5 (``alpha^2 (1 + r) exp(-r)``, ``r = sqrt(3) d``) or 2.5
    (``alpha^2 (1 + r + r^2 / 3) exp(-r)``, ``r = sqrt(5) d``)."""
    if nu not in {1.5, 2.5}:
        raise ValueError(f"Invalid value `nu`={nu}. Only values of (1.5, 2.5) are currently supported.")
    return _matern(euclidean_difference_kernel(N, width), alpha, nu)


def periodic_kernel(N, width, alpha, p, **kwargs):
    """Exp-sine-squared kernel ``alpha^2 exp(-2 sin^2(pi d / p))``.  Host only."""
    C = np.sin(np.pi * euclidean_difference_kernel(N, width) / p)
    C = np.exp(-2 * C**2)
    C *= alpha**2
    return C


def moving_average_inverse_kernel(N, width, alpha, periodic=True):
    """Inverse covariance ``alpha (I - W)^T (I - W)`` of a smoothness prior, ``W`` the average over a window of ``width``
    points around each of ``N`` points (wrapped if ``periodic``, else cut at the ends).  Host only."""
    W = np.zeros((N, N))
    for i in range(N):
        lo, hi = i - (width - 1) // 2, i + (width + 1) // 2
        if not periodic:
            lo, hi = max(0, lo), min(hi, N)
        v = np.arange(lo, hi)
        W[i][v % N] = 1.0 / len(v)
    IW = np.identity(N) - W
    return alpha * (IW.T @ IW)


def pair_kernel(name, x, y, width, alpha, **params):
    """``k(x[i], y[i])`` of the ``gaussian``, ``rational`` or ``matern`` kernel, element for element the value the matrix
    functions give for that pair of positions."""
    d = np.asarray(x, dtype=np.float64) / width - np.asarray(y, dtype=np.float64) / width
    name = name.lower()
    if name == "gaussian":
        return _gaussian(d**2, alpha)
    if name == "rational":
        return _rational(d**2, alpha, params["a"])
    if name == "matern":
        return _matern(np.abs(d), alpha, params["nu"])  # (|d| is what sqrt(d^2) rounds to)
    raise NotImplementedError(f"the '{name}' kernel has no element-wise form")


# ------------------------------------------------------------------------------------------------ distance functions
def _scaled_positions(N, width):
    if isinstance(N, int | np.ndarray):
        N = (N, N)
    if isinstance(width, int | float):
        width = (width, width)
    if len(N) != 2 or len(width) != 2:
        raise ValueError(f"Invalid parameters. Got N={N} and width={width}.")
    i0 = np.arange(N[0]) if isinstance(N[0], int) else N[0]
    i1 = np.arange(N[1]) if isinstance(N[1], int) else N[1]
    return i0 / width[0], i1 / width[1]


def squared_difference_kernel(N, width):
    """Squared separations ``(x_i / width - y_j / width)^2``."""
    i0, i1 = _scaled_positions(N, width)
    return np.subtract.outer(i0, i1) ** 2


def euclidean_difference_kernel(N, width):
    """Separations ``|x_i / width - y_j / width|`` (as the square root of the square, like a distance in more
    dimensions)."""
    i0, i1 = _scaled_positions(N, width)
    return np.sqrt(np.subtract.outer(i0, i1) ** 2)


# --------------------------------------------------------------------------------------------------------- utilities
def is_hermitian_positive_definite(x):
    """Whether ``x`` is Hermitian and has a Cholesky factor."""
    if not la.ishermitian(x):
        return False
    try:
        la.cholesky(x, lower=False)
    except la.LinAlgError:
        return False
    return True


def band_rows(x, tol=1.0e-8):
    """``M`` of :func:`convert_band_diagonal`: half the largest number of entries above ``tol`` in a row, plus one."""
    x = np.asarray(x)
    return int(np.sum(x > tol, axis=-1).max() // 2 + 1)


def convert_band_diagonal(x, tol=1.0e-8, which="full"):
    """Band form of the symmetric band-diagonal ``n x n`` matrix ``x`` for ``scipy.linalg.solveh_banded``.

    The band has ``M = band_rows(x, tol)`` diagonals; whatever lies beyond them is dropped, whatever its size.
    ``which = "lower"``: ``[M, n]``, row ``d`` holds diagonal ``d`` from column 0.  ``"upper"``: ``[M, n]``, row 0 holds
    the main diagonal and row ``M - d`` diagonal ``d`` from column ``d`` (the reference's arrangement, kept as it is).
    ``"full"``: ``[2 M - 1, n]``, rows ``1 ...`` of the upper form above the lower form.
    """
    if which not in {"full", "upper", "lower"}:
        raise ValueError(f"Got invalid argument `which`={which}. Only `full`, `upper`, or `lower` are accepted.")
    x = np.asarray(x)
    n, M = x.shape[0], band_rows(x, tol)
    lower = np.zeros((M, n), dtype=x.dtype)
    upper = np.zeros((M, n), dtype=x.dtype)
    for d in range(M):
        lower[d, : n - d] = x.diagonal(d)
        upper[-d, d:] = x.diagonal(-d)
    if which == "lower":
        return lower
    if which == "upper":
        return upper
    return np.concatenate([upper[1:], lower])


def _get_band_inds(R, tol=1.0e-4):
    """``(start, end)`` int32 per row of ``R``: the first column whose magnitude exceeds ``tol`` and one past the last;
    ``(0, 0)`` for a row without one."""
    u = np.abs(R) > tol
    start = np.argmax(u, axis=-1)
    end = R.shape[-1] - np.argmax(u[..., ::-1], axis=-1)
    end[~np.any(u, axis=-1)] = 0
    return start.astype(np.int32), end.astype(np.int32)
