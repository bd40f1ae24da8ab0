"""Long-double twin of the Gaussian-process regridder's chain (``draco_amd/util/gaussian_process.py``, ``csrc/gp.hip``),
on the same band-truncated kernel matrix: banded Cholesky factorisation, the two triangular solves, the band edges of
the projection and the two banded products.  The truth of ``tests/test_gpu_gp.py``; ``tests/golden/gp.npz`` pins it to
the reference (``tests/gen_golden_gp.py``).  NumPy only.
"""

import numpy as np

LD = np.longdouble
TOL = 1.0e-8


def band_truncate(K, M):
    """``K`` with everything beyond ``M`` diagonals either side dropped."""
    n = K.shape[0]
    d = np.abs(np.subtract.outer(np.arange(n), np.arange(n)))
    return np.where(d < M, K, 0.0)


def band_cholesky(K, M):
    """Lower factor of the band-truncated ``K`` in long double, ``None`` if a pivot is not positive."""
    n = K.shape[0]
    K = np.asarray(K, dtype=LD)
    L = np.zeros((n, n), dtype=LD)
    for i in range(n):
        lo = max(0, i - M + 1)
        for j in range(lo, i):
            L[i, j] = (K[i, j] - L[i, lo:j] @ L[j, lo:j]) / L[j, j]
        d = K[i, i] - L[i, lo:i] @ L[i, lo:i]
        if not d > 0:
            return None
        L[i, i] = np.sqrt(d)
    return L


def project(K, Kstar, M):
    """``A = Kstar K_M^-1 [nk, n]`` in long double, ``K_M`` the band-truncated ``K``; ``None`` if not positive definite."""
    L = band_cholesky(K, M)
    if L is None:
        return None
    n = K.shape[0]
    Y = np.array(np.asarray(Kstar, dtype=LD).T)
    for i in range(n):
        lo = max(0, i - M + 1)
        Y[i] = (Y[i] - L[i, lo:i] @ Y[lo:i]) / L[i, i]
    for i in range(n - 1, -1, -1):
        hi = min(n, i + M)
        Y[i] = (Y[i] - L[i + 1 : hi, i] @ Y[i + 1 : hi]) / L[i, i]
    return Y.T


def band_inds(A, tol=TOL):
    u = np.abs(A) > tol
    start = np.argmax(u, axis=-1)
    end = A.shape[-1] - np.argmax(u[..., ::-1], axis=-1)
    end[~np.any(u, axis=-1)] = 0
    return start.astype(np.int32), end.astype(np.int32)


def inz32(x):
    x = np.asarray(x, dtype=np.float32)
    return np.where(x == 0, np.float32(0), np.float32(1) / np.where(x == 0, np.float32(1), x)).astype(np.float32)


def apply(A, start, end, x, w):
    """One frequency: ``A [nk, n]``, ``x [n, nstack]`` complex64, ``w [n, nstack]`` float32 of the selected samples ->
    ``(xout [nk, nstack] complex128 before the rounding to complex64, var [nk, nstack] long double, wout float32)``.
    ``wout`` is the float32 chain: the variance rounded to float32, inverted in float32, negatives zeroed; a stack
    without a positive weight is zero."""
    nk, nst = A.shape[0], x.shape[1]
    v = inz32(w).astype(LD)
    xr, xim = x.real.astype(LD), x.imag.astype(LD)
    outr = np.zeros((nk, nst), dtype=LD)
    outi = np.zeros((nk, nst), dtype=LD)
    var = np.zeros((nk, nst), dtype=LD)
    for b in range(nk):
        s, e = start[b], end[b]
        a = np.asarray(A[b, s:e], dtype=LD)
        outr[b] = a @ xr[s:e]
        outi[b] = a @ xim[s:e]
        var[b] = (a * a) @ v[s:e]
    live = np.any(v > 0, axis=0)
    outr[:, ~live] = outi[:, ~live] = var[:, ~live] = 0
    wout = inz32(var.astype(np.float32))
    neg = wout < 0
    wout[neg] = 0
    xout = outr.astype(np.float64) + 1j * outi.astype(np.float64)
    xout[neg] = 0
    return xout, var, wout


def resample(data, weight, K, Kstar, mt, M_of=None):
    """The chain on ``data`` / ``weight [nfreq, nt, nstack]`` with host matrices ``K [nt, nt]``, ``Kstar [nout, nt]`` and
    the kept rows ``mt [nfreq, nout]``: ``(xout complex128, wout float32) [nfreq, nout, nstack]`` and per frequency the
    dict of ``A`` (long double), ``start``, ``end``, ``M``, ``mi`` (``None`` for a frequency that is skipped).  Raises
    ``np.linalg.LinAlgError`` if a truncated matrix is not positive definite."""
    nfreq, nt, nst = data.shape
    nout = Kstar.shape[0]
    xout = np.zeros((nfreq, nout, nst), dtype=np.complex128)
    wout = np.zeros((nfreq, nout, nst), dtype=np.float32)
    parts, cache = [], {}
    for ii in range(nfreq):
        mi = np.any(weight[ii] > 0, axis=-1)
        if not mt[ii].any() or not mi.any():
            parts.append(None)
            continue
        key = mi.tobytes() + mt[ii].tobytes()
        if key not in cache:
            Kd = K[mi][:, mi]
            M = int(np.sum(Kd > TOL, axis=-1).max() // 2 + 1) if M_of is None else M_of(Kd)
            A = project(Kd, Kstar[mt[ii]][:, mi], M)
            if A is None:
                raise np.linalg.LinAlgError(f"frequency {ii}: the truncated kernel matrix is not positive definite")
            start, end = band_inds(A)
            cache[key] = {"A": A, "start": start, "end": end, "M": M, "mi": mi}
        p = cache[key]
        xo, _, wo = apply(p["A"], p["start"], p["end"], data[ii][mi], weight[ii][mi])
        xout[ii, mt[ii]] = xo
        wout[ii, mt[ii]] = wo
        parts.append(p)
    return xout, wout, parts
