"""Long-double truth for the blocked Cholesky solver of ``csrc/chol_blocked.hip`` (``dl_factor`` + ``dl_solve_rows``,
reached through ``dmm_mfilter_solve``), and the inputs and measures its tests share.  NumPy only.

* ``chol_upper_ld``   unblocked ``G = U^T U`` in long double, reading the upper triangle only;
* ``solve_rows_ld``   the two substitutions ``z U = y``, ``x U^T = z`` on the rows of ``Y``, in long double;
  ``solve_rows_small_ld`` is the same written out in closed form for orders 1 to 3 (millions of rows);
* ``spd``             ``Q diag(lambda) Q^T`` with log-spaced ``lambda`` in ``[1, cond]``, symmetrised exactly, float64;
  the truth of a solve is the inverse of that float64 matrix;
* ``solve_f64``       the float64 reference: ``numpy.linalg.cholesky`` and two triangular solves;
* ``residual_bound``  the componentwise a-priori bound on ``|G x - y|`` of a Cholesky solve.

Measures.  Backward (derived): for a Cholesky solve ``|G x - y| <= gamma_{3n+1} |U|^T |U| |x|`` componentwise, ``gamma_k
= k u / (1 - k u)``, ``u = 2**-53`` (Higham, Accuracy and Stability of Numerical Algorithms, theorem 10.4).  The tests
use the twin's ``U`` in place of the computed factor, so nothing of the code under test enters the bound, and allow
twice the bound for that substitution and for fma contraction.  Forward (measured): ``e = max |x - x*| / max |x*|`` per
matrix, ``x*`` the long-double solution rounded to float64; required ``e <= max(4 e_ref, n 2**-52)``, ``e_ref`` the
same measure of ``solve_f64``: the margin 4 is for another summation order, the floor one rounding per accumulated
term.
"""

import numpy as np

try:
    from scipy.linalg import solve_triangular as _solve_triangular
except ImportError:  # (the reference solve then goes through numpy.linalg.solve on the factors)
    _solve_triangular = None

LD = np.longdouble
U = 2.0**-53

CONDS = (1e2, 1e6, 1e10)
# (order, right-hand sides): 1 and 2, around the 32-row block and the 64 tile, one past a tile with a one-row last block
SWEEP = [(1, 1), (1, 257), (2, 3), (31, 64), (32, 65), (33, 1), (63, 255), (64, 256), (65, 257), (95, 63), (96, 64), (97, 65),
         (128, 3), (129, 513), (257, 129)]


def chol_upper_ld(G):
    """``U`` upper triangular with ``U^T U = G``, long double; only ``G[i][j]``, ``j >= i``, is read."""
    G = np.asarray(G)
    n = G.shape[0]
    Uf = np.zeros((n, n), dtype=LD)
    for j in range(n):
        row = G[j, j:].astype(LD) - Uf[:j, j] @ Uf[:j, j:]
        if not row[0] > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        d = np.sqrt(row[0])
        Uf[j, j] = d
        Uf[j, j + 1 :] = row[1:] / d
    return Uf


def schur_pivot_ld(G, j):
    """``G[j][j] - sum_{k < j} U[k][j]^2``: the pivot the factorisation meets at row ``j`` (upper triangle of ``G``)."""
    Uf = chol_upper_ld(np.asarray(G)[:j, :j]) if j else np.zeros((0, 0), dtype=LD)
    col = np.asarray(G)[:j, j].astype(LD)
    w = np.zeros(j, dtype=LD)  # U[:j, :j]^T w = G[:j, j]
    for c in range(j):
        w[c] = (col[c] - Uf[:c, c] @ w[:c]) / Uf[c, c]
    return LD(np.asarray(G)[j, j]) - w @ w


def solve_rows_ld(Uf, Y):
    """The rows ``x`` of ``U^T U x = y`` for the rows ``y`` of ``Y [nrow][n]``, long double."""
    Uf = np.asarray(Uf, dtype=LD)
    n = Uf.shape[0]
    X = np.array(Y, dtype=LD)
    for c in range(n):  # z U = y
        X[:, c] = (X[:, c] - X[:, :c] @ Uf[:c, c]) / Uf[c, c]
    for c in range(n - 1, -1, -1):  # x U^T = z
        X[:, c] = (X[:, c] - X[:, c + 1 :] @ Uf[c, c + 1 :]) / Uf[c, c]
    return X


def solve_rows_small_ld(Uf, Y):
    """``solve_rows_ld`` for ``n <= 3`` written out, every operation one long-double array operation over the rows."""
    Uf = np.asarray(Uf, dtype=LD)
    n = Uf.shape[0]
    assert 1 <= n <= 3 and Y.shape[1] == n
    y = [Y[:, c].astype(LD) for c in range(n)]
    X = np.empty(Y.shape, dtype=LD)
    if n == 1:
        X[:, 0] = y[0] / Uf[0, 0] / Uf[0, 0]
        return X
    if n == 2:
        z0 = y[0] / Uf[0, 0]
        z1 = (y[1] - z0 * Uf[0, 1]) / Uf[1, 1]
        x1 = z1 / Uf[1, 1]
        X[:, 1] = x1
        X[:, 0] = (z0 - x1 * Uf[0, 1]) / Uf[0, 0]
        return X
    z0 = y[0] / Uf[0, 0]
    z1 = (y[1] - z0 * Uf[0, 1]) / Uf[1, 1]
    z2 = (y[2] - (z0 * Uf[0, 2] + z1 * Uf[1, 2])) / Uf[2, 2]
    x2 = z2 / Uf[2, 2]
    x1 = (z1 - x2 * Uf[1, 2]) / Uf[1, 1]
    X[:, 2] = x2
    X[:, 1] = x1
    X[:, 0] = (z0 - (x1 * Uf[0, 1] + x2 * Uf[0, 2])) / Uf[0, 0]
    return X


def spd(n, cond, rng):
    """Symmetric positive definite float64 ``Q diag(lambda) Q^T``, ``lambda`` log-spaced over ``[1, cond]``; order 1,
    which has no spread, gets the midpoint ``sqrt(cond)`` (``lambda = 1`` would make the solve the identity map)."""
    q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    lam = np.logspace(0.0, np.log10(cond), n) if n > 1 else np.sqrt([cond])
    g = (q * lam[np.newaxis, :]) @ q.T
    return np.ascontiguousarray(0.5 * (g + g.T))  # (a + b and b + a round alike: symmetric to the bit)


def solve_f64(G, Y):
    """The float64 reference: ``(X [nrow][n], U)`` with ``U`` the transposed ``numpy.linalg.cholesky`` factor."""
    low = np.linalg.cholesky(G)
    rhs = np.ascontiguousarray(Y.T)
    if _solve_triangular is not None:
        z = _solve_triangular(low, rhs, lower=True)
        x = _solve_triangular(low.T, z, lower=False)
    else:
        x = np.linalg.solve(low.T, np.linalg.solve(low, rhs))
    return np.ascontiguousarray(x.T), np.ascontiguousarray(low.T)


def gamma(k):
    return k * U / (1.0 - k * U)


def residual_bound(U_ld, x, n):
    """``2 gamma_{3n+1} |U|^T |U| |x|`` for the rows of ``x [nrow][n]``, long double (the factor 2: see the module)."""
    a = np.abs(np.asarray(U_ld, dtype=LD))
    return LD(2.0 * gamma(3 * n + 1)) * ((np.abs(np.asarray(x)).astype(LD) @ a.T) @ a)


def residual(G, x, Y):
    """``G x - y`` for the rows of ``x``, ``Y``, in long double; ``G`` symmetric from its upper triangle."""
    g = np.triu(np.asarray(G)).astype(LD)
    g = g + np.triu(g, 1).T
    return np.asarray(x).astype(LD) @ g - np.asarray(Y).astype(LD)


def backward_ratio(G, U_ld, x, Y, rows=slice(None)):
    """The worst ``|G x - y| / bound`` over the elements of ``rows`` (0 / 0 counts as 0); at most 1 passes."""
    x, Y = np.asarray(x)[rows], np.asarray(Y)[rows]
    res, bnd = np.abs(residual(G, x, Y)), residual_bound(U_ld, x, np.asarray(G).shape[0])
    if not np.all(np.isfinite(res.astype(np.float64))):
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(res == 0, LD(0), res / bnd)
    return float(q.max())


def forward_err(x, truth, rows=slice(None)):
    """``max |x - x*| / max |x*|`` with ``x*`` the truth rounded to float64; the scale is that of all rows."""
    t = np.asarray(truth, dtype=np.float64)
    return float(np.abs(np.asarray(x)[rows] - t[rows]).max() / np.abs(t).max())


def forward_limit(e_ref, n):
    return max(4.0 * e_ref, n * 2.0**-52)


class Case:
    """One batch of the sweep: ``G [nmat][n][n]`` (one matrix per entry of ``conds``), ``Y [nmat][nrow][n]``, the
    long-double factors ``U`` and solutions ``X`` (``X64``: rounded to float64), and the float64 reference's ``x_ref``,
    ``u_ref`` with their forward errors ``e_ref``, ``e_ref_u`` per matrix."""

    def __init__(self, n, nrow, conds=CONDS, seed=None, small=False):
        rng = np.random.default_rng([20261018, n, nrow] if seed is None else seed)
        self.n, self.nrow, self.nmat = n, nrow, len(conds)
        self.G = np.stack([spd(n, c, rng) for c in conds])
        self.Y = rng.normal(size=(self.nmat, nrow, n))
        self.U = [chol_upper_ld(g) for g in self.G]
        solve = solve_rows_small_ld if small else solve_rows_ld
        self.X = [solve(u, y) for u, y in zip(self.U, self.Y)]
        self.X64 = [x.astype(np.float64) for x in self.X]
        self.xmax = [float(np.abs(x).max()) for x in self.X64]
        ref = [solve_f64(g, y) for g, y in zip(self.G, self.Y)]
        self.x_ref, self.u_ref = [r[0] for r in ref], [r[1] for r in ref]
        self.e_ref = [forward_err(x, t) for x, t in zip(self.x_ref, self.X64)]
        self.e_ref_u = [forward_err(u, t) for u, t in zip(self.u_ref, self.U)]

    def poisoned(self):
        """``G`` with NaN in the strict lower triangle: what the GPU gets."""
        g = self.G.copy()
        g[:, np.tril(np.ones((self.n, self.n), dtype=bool), -1)] = np.nan
        return g

    def measure(self, t, x, rows=slice(None)):
        """``(e, worst residual / bound)`` of a solution ``x [nrow][n]`` of matrix ``t``."""
        e = float(np.abs(np.asarray(x)[rows] - self.X64[t][rows]).max() / self.xmax[t])
        return e, backward_ratio(self.G[t], self.U[t], x, self.Y[t], rows)
