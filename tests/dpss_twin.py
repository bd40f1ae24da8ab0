"""NumPy twin of the DPSS inpainting of ``draco_amd/util/dpss.py`` (``csrc/dpss.hip``): the reference's
``dpss.filter`` / ``dpss.inpaint`` / ``dpss.flag_above_cutoff`` and the column loop of ``DPSSFilter._filter`` restated
with the basis ``A`` as an input, in float64 or in ``np.longdouble``.

Per column (``x`` complex, ``Ni`` weights, ``W`` mask, ``Si`` the regulariser):

1. ``xhat = sum(W x) inz(sum W)``;  2. ``xp = A^T (Ni (x - xhat))``;  3. ``C = A^T diag(Ni) A + Si I``;
4. ``C = U^T U``, ``b = C^-1 xp``;  5. ``xfilt = A b + xhat``;  6. all ``Ni`` zero: ``b = 0``, solved weight 0;
7. solved variance = diag ``F N F^H``, ``F = A C^-1 A^T Ni``, ``N = inz(Ni)``; solved weight its ``inz``;
8. PCHIP (SciPy, float64 in both precisions: its inputs are exact weights) of ``inz(Ni)`` through the samples where
   ``W`` is set, evaluated at every index, negative values set to 0, added to the solved variance; weight = ``inz``;
   fewer than two valid samples: no interpolant;
9. ``inpaint`` puts ``x`` and ``Ni`` back where ``W`` is set;  10. the task multiplies the weights by
   ``flag_above_cutoff(Ni > 0, cutoff)``.

The long-double truth forms step 7 directly (``variance="direct"``: ``var_i = sum_j F_ij^2 N_j``, the reference's
einsum); the float64 twin forms it as the library does (``variance="identity"``: ``var_i = |z_i|^2 - Si |y_i|^2`` with
``z_i = U^-T a_i``, ``y_i = U^-1 z_i``), so its error against the truth includes whatever the identity cancels.
The long-double Cholesky and substitutions are those of ``tests/chol_twin.py``.
"""

import numpy as np
from scipy.interpolate import PchipInterpolator

import chol_twin

LD = np.longdouble
FLOOR_VIS = 2.0**-22  # float32 rounding of the output, doubled
FLOOR_W = 2.0**-21


def inz(x):
    x = np.asarray(x)
    out = np.zeros_like(x)
    nz = x != 0
    out[nz] = 1 / x[nz]
    return out


def _factor(Cm, ld):
    return chol_twin.chol_upper_ld(Cm) if ld else np.ascontiguousarray(np.linalg.cholesky(Cm).T)


def _solve_rows(U, Y, ld, forward_only=False):
    """Rows ``x`` of ``U^T U x = y`` (or of ``U^T z = y``) for the rows ``y`` of ``Y``."""
    if ld:
        if not forward_only:
            return chol_twin.solve_rows_ld(U, Y)
        X = np.array(Y, dtype=LD)
        for c in range(U.shape[0]):
            X[:, c] = (X[:, c] - X[:, :c] @ U[:c, c]) / U[c, c]
        return X
    from scipy.linalg import solve_triangular

    z = solve_triangular(U, np.ascontiguousarray(Y.T), trans="T", lower=False)
    if forward_only:
        return np.ascontiguousarray(z.T)
    return np.ascontiguousarray(solve_triangular(U, z, lower=False).T)


def solve_column(xp, Ni, A, Si, ld=False, variance=None):
    """``(b, var)`` of one column: ``b = C^-1 xp`` (complex) and the solved variance; ``None`` if every ``Ni`` is zero.
    Raises ``numpy.linalg.LinAlgError`` where ``C`` is not positive definite."""
    if np.all(Ni == 0):
        return None
    variance = variance or ("direct" if ld else "identity")
    ft = LD if ld else np.float64
    A, Ni = A.astype(ft), Ni.astype(ft)
    Cm = (A.T * Ni[np.newaxis, :]) @ A
    Cm[np.diag_indices_from(Cm)] += ft(Si)
    U = _factor(Cm, ld)
    rhs = np.stack([xp.real, xp.imag]).astype(ft)
    sol = _solve_rows(U, rhs, ld)
    b = sol[0] + 1j * sol[1]
    if variance == "identity":
        Z = _solve_rows(U, A, ld, forward_only=True)
        Y = _solve_rows(U, A, ld)
        var = np.sum(Z * Z, axis=1) - ft(Si) * np.sum(Y * Y, axis=1)
    else:
        beta = _solve_rows(U, A * Ni[:, np.newaxis], ld)  # [n][k]: row j = C^-1 a_j Ni_j
        F = A @ beta.T
        var = (F * F) @ inz(Ni)
    return b, var


def filter_columns(x, Ni, A, W, Si, ld=False, put_back=False, variance=None):
    """``dpss.filter`` (``put_back=False``) or ``dpss.inpaint`` of ``x [n, ncol]``, ``Ni``, ``W`` with the real basis
    ``A [n, k]``: ``(xfilt, wfilt)`` in complex / real float64 or long double."""
    ft, ct = (LD, np.clongdouble) if ld else (np.float64, np.complex128)
    x, Ni, W, A = np.asarray(x).astype(ct), np.asarray(Ni).astype(ft), np.asarray(W, dtype=bool), np.asarray(A).astype(ft)
    n, ncol = x.shape
    xf, wf = np.zeros((n, ncol), dtype=ct), np.zeros((n, ncol), dtype=ft)
    samples = np.arange(n)
    for c in range(ncol):
        w = W[:, c]
        xhat = np.sum(x[w, c]) / ft(w.sum()) if w.any() else ct(0)
        xp = A.T @ (Ni[:, c] * (x[:, c] - xhat))
        sol = solve_column(xp, Ni[:, c], A, Si, ld, variance)
        if sol is None:
            b, vi = np.zeros(A.shape[1], dtype=ct), np.zeros(n, dtype=ft)
        else:
            b, var = sol
            vi = inz(inz(var))
        xf[:, c] = A @ b + xhat
        if w.sum() >= 2:
            wint = PchipInterpolator(samples[w], inz(Ni[w, c]).astype(np.float64), extrapolate=True)(samples)
            wint[wint < 0] = 0
            vi = vi + wint.astype(ft)
        wf[:, c] = inz(vi)
    if put_back:
        xf[W], wf[W] = x[W], Ni[W]
    return xf, wf


def flag_above_cutoff(W, fc):
    """``dpss.flag_above_cutoff`` along the first axis, sample by sample: a gap from ``ri`` to ``fi`` has ``dist = fi -
    ri`` (its width minus one) and is kept where ``dist < fc``; a gap that reaches the end is never paired with a
    falling edge and keeps ``dist = 0``; everything before the first valid sample, and from the last valid sample on,
    has ``dist = 2 fc``; with no valid sample only the last sample has."""
    W = np.asarray(W, dtype=bool)
    if fc is None:
        return W
    n, ncol = W.shape
    fc32 = np.float32(fc)
    dist = np.zeros(W.shape, dtype=np.float32)
    for c in range(ncol):
        valid = np.flatnonzero(W[:, c])
        i = 0
        while i < n:
            if W[i, c]:
                i += 1
                continue
            j = i
            while j + 1 < n and not W[j + 1, c]:
                j += 1
            if j + 1 < n:  # a falling edge exists
                dist[i : j + 1, c] = j - i
            i = j + 1
        lb, rb = (valid[0], valid[-1]) if valid.size else (0, n - 1)
        dist[:lb, c] = 2 * fc32
        dist[rb:, c] = 2 * fc32
    return dist < fc32


def task_columns(vis, weight, axis, bases, amap, Si, cutoff, inpaint=True, ld=False, variance=None):
    """The column loop of ``DPSSFilter._filter`` on ``vis [freq, stack, ra]``: ``axis`` 0 (frequency) or 2 (RA), stack
    entry ``s`` uses ``bases[amap[s]]``.  Returns ``(vis, weight)`` rounded to complex64 / float32."""
    vo, wo = np.zeros(vis.shape, dtype=np.complex64), np.zeros(weight.shape, dtype=np.float32)
    for s in range(vis.shape[1]):
        x, Ni = (vis[:, s, :], weight[:, s, :]) if axis == 0 else (vis[:, s, :].T, weight[:, s, :].T)
        M = Ni > 0
        xf, wf = filter_columns(x, Ni, bases[amap[s]], M, Si, ld, inpaint, variance)
        wf = wf * flag_above_cutoff(M, cutoff)
        xf, wf = xf.astype(np.complex64), wf.astype(np.float32)
        if axis == 0:
            vo[:, s, :], wo[:, s, :] = xf, wf
        else:
            vo[:, s, :], wo[:, s, :] = xf.T, wf.T
    return vo, wo


def rel_err(got, truth):
    """``max |got - truth| / max |truth|``."""
    got, truth = np.asarray(got), np.asarray(truth)
    ct = np.clongdouble if np.iscomplexobj(truth) or np.iscomplexobj(got) else LD
    return float(np.abs(got.astype(ct) - truth.astype(ct)).max() / np.abs(truth.astype(ct)).max())


def weight_err(got, truth):
    """``(largest elementwise relative error where the truth is non-zero, zero patterns equal)``."""
    got, truth = np.asarray(got), np.asarray(truth)
    nz = truth != 0
    same = bool(np.array_equal(got != 0, nz))
    if not nz.any():
        return 0.0, same
    g, t = got[nz].astype(LD), truth[nz].astype(LD)
    return float(np.max(np.abs(g - t) / np.abs(t))), same
