"""Twins of the Wiener delay transform of a filtered ring map (``draco/analysis/powerspec.py:118-458``), host NumPy.

* :func:`build` / :func:`apply` with ``ld=True``: long double throughout, with a complex long-double Cholesky
  factorisation of the valid block; rounded once at the end this is the truth of ``tests/golden/wienerdelay.npz`` and
  of the GPU tests.
* the same functions with ``ld=False``: the float64 NumPy form (NumPy's own factorisation).

The per-task constants ``F [freq, delay]``, ``Sdiag [delay]`` and ``window [freq]`` are inputs: the reference and the
tasks form them on the host with the same float64 expressions (:func:`constants`), so they are part of the problem, not
of the error.  ``F S F^H`` is formed here, in the precision of the twin.

``rel_err(a, t) = max |a - t| / max |t|`` as in the other twins.
"""

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
DF = 0.390625


def rel_err(a, t):
    a, t = np.asarray(a), np.asarray(t)
    den = np.abs(t).max() if t.size else 0.0
    if den == 0:
        return float(np.abs(a).max()) if a.size else 0.0
    return float(np.abs(a.astype(t.dtype) - t).max() / den)


def from_q64(q):
    """int16 numerators over 64 -> float64 (exact)."""
    return np.asarray(q, dtype=np.float64) / 64.0


def inv0(x):
    x = np.asarray(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0, x.dtype.type(0), 1 / np.where(x == 0, x.dtype.type(1), x))


def constants(freq, window, prior_amp, prior_scale):
    """``(tau, F, Sdiag)`` in float64 with the reference's expressions, from the window values."""
    dfreq = np.median(np.abs(np.diff(freq)))
    ntau = np.sum(window > 0, dtype=int)
    tau = np.fft.fftshift(np.fft.fftfreq(ntau, d=dfreq))
    tau = tau[tau >= 0.0]
    F = np.exp(2.0j * np.pi * np.outer(freq, tau)) / np.sqrt(ntau)
    Sdiag = prior_amp * np.exp(-2.0 * np.pi * prior_scale * np.abs(tau))
    return tau, F, Sdiag


def cholesky_ld(A):
    """Lower Cholesky factor of a complex Hermitian positive definite matrix in long double (the lower triangle is
    read); raises ``numpy.linalg.LinAlgError`` at a pivot that is not positive."""
    n = A.shape[0]
    L = np.zeros((n, n), dtype=CLD)
    for j in range(n):
        d = A[j, j].real - (np.abs(L[j, :j]) ** 2).sum()
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ np.conj(L[j, :j])) / L[j, j].real
    return L


def inverse_ld(A):
    """``A^-1`` of a Hermitian positive definite matrix through :func:`cholesky_ld`."""
    n = A.shape[0]
    L = cholesky_ld(A)
    Z = np.zeros((n, n), dtype=CLD)  # L Z = I
    eye = np.eye(n, dtype=CLD)
    for i in range(n):
        Z[i] = (eye[i] - L[i, :i] @ Z[:i]) / L[i, i].real
    return Z.conj().T @ Z


def covariance(K, C, w, b, FSFT, win_mask):
    """``(A, H, M)`` of one pixel: ``K, C [n, n]``, ``w, b [n]``, in the precision of the arguments."""
    r = np.sqrt(inv0(w * np.diagonal(C))) * win_mask
    M = win_mask & (w > 0)
    H = M[:, np.newaxis] * K
    A = H @ (FSFT * b[:, np.newaxis] * b) @ H.T + C * (r[:, np.newaxis] * r[np.newaxis, :])
    return A, H, M


def build(K, C, w, dbp, F, Sdiag, window, ld=True, pixels=None):
    """The operator ``[npol, nra, nel, ndelay, nfreq]`` (complex long double or complex128) from ``K, C [npol, n, n,
    nra]``, ``w [npol, n, nra, nel]``, ``dbp [npol, n, nel]``.  ``pixels``: only these ``(pol, ra, el)`` (the rest
    stays zero)."""
    R, Z = (LD, CLD) if ld else (np.float64, np.complex128)
    npol, n, nra, nel = w.shape
    nd = F.shape[1]
    K, C, w, dbp, Sdiag, window = (np.asarray(a, dtype=R) for a in (K, C, w, dbp, Sdiag, window))
    F = np.asarray(F, dtype=Z)
    FT = F.T.conj()
    FSFT = (F * Sdiag[np.newaxis, :]) @ FT
    win_mask = window > 0
    D = np.zeros((npol, nra, nel, nd, n), dtype=Z)
    todo = pixels if pixels is not None else [(p, r, e) for p in range(npol) for r in range(nra) for e in range(nel)]
    for p, r, e in todo:
        A, H, M = covariance(K[p, :, :, r], C[p, :, :, r], w[p, :, r, e], np.sqrt(dbp[p, :, e]), FSFT, win_mask)
        valid = np.flatnonzero(M)
        if valid.size == 0:
            continue
        sub = A[np.ix_(valid, valid)]
        A_inv = np.zeros((n, n), dtype=Z)
        A_inv[np.ix_(valid, valid)] = inverse_ld(sub) if ld else np.linalg.inv(_posdef(sub))
        D[p, r, e] = Sdiag[:, np.newaxis] * ((FT @ H.T) @ A_inv) * window
    return D


def _posdef(sub):
    np.linalg.cholesky(sub)  # (raises LinAlgError like the reference's cho_factor)
    return sub


def cond_valid(K, C, w, dbp, F, Sdiag, window):
    """The largest 2-norm condition number of the valid block of ``A`` over all pixels (float64)."""
    npol, n, nra, nel = w.shape
    FSFT = (F * Sdiag[np.newaxis, :]) @ F.T.conj()
    worst = 0.0
    for p in range(npol):
        for r in range(nra):
            for e in range(nel):
                A, _, M = covariance(K[p, :, :, r], C[p, :, :, r], w[p, :, r, e], np.sqrt(dbp[p, :, e]), FSFT, window > 0)
                v = np.flatnonzero(M)
                if v.size:
                    worst = max(worst, float(np.linalg.cond(A[np.ix_(v, v)])))
    return worst


def apply(op, m, w, ld=True):
    """``(spectrum [npol nel, nra, ndelay], weight)`` from ``op [npol, nra, nel, ndelay, nfreq]``, ``m, w [npol, nfreq,
    nra, nel]``: ``spectrum = op m``, ``weight = inv0(|op|^2 inv0(w))``."""
    R, Z = (LD, CLD) if ld else (np.float64, np.complex128)
    op = np.asarray(op).astype(Z)
    m, w = np.asarray(m, dtype=R), np.asarray(w, dtype=R)
    npol, nra, nel, nd, n = op.shape
    mt = m.transpose(0, 2, 3, 1)  # [pol, ra, el, freq]
    vt = inv0(w).transpose(0, 2, 3, 1)
    spec = (op * mt[:, :, :, np.newaxis, :]).sum(axis=-1)
    var = ((op.real**2 + op.imag**2) * vt[:, :, :, np.newaxis, :]).sum(axis=-1)
    to_bl = lambda a: a.transpose(0, 2, 1, 3).reshape(npol * nel, nra, nd)  # noqa: E731
    return to_bl(spec), to_bl(inv0(var))


def case_inputs(z, name):
    """The inputs of case ``name`` of the golden file as float64 arrays and its configuration."""
    g = lambda k: z[f"{name}/{k}"]  # noqa: E731
    if f"{name}/K" in z.files:
        K, C = g("K"), g("C")
    else:
        K = kmatrix(g("Q"), g("kmask"))
        C = cov_of(K, from_q64(g("var_q64")))
    cfg = {"window": str(g("window")), "prior_amp": float(g("prior_amp")), "prior_scale": float(g("prior_scale"))}
    for k in ("window_lower_freq", "window_upper_freq"):
        v = float(g(k))
        cfg[k] = None if np.isnan(v) else v
    return {"K": K, "C": C, "w": from_q64(g("w_q64")), "dbp": from_q64(g("dbp_q64")), "map": from_q64(g("map_q64")), "freq": g("freq"), "cfg": cfg}


def kmatrix(Q, kmask):
    """``K [npol, n, n, nra] = diag(mask)(I + Q / 64)``: exact in float64."""
    npol, n, _, nra = Q.shape
    eye = np.eye(n)[np.newaxis, :, :, np.newaxis]
    return kmask[:, :, np.newaxis, :] * (eye + np.asarray(Q, dtype=np.float64) / 64.0)


def cov_of(K, var):
    """``C = K diag(var) K^T`` per (pol, ra); ``var [npol, n, nra]``.  With ``K`` and ``var`` multiples of 1 / 64 of a
    few bits every product and sum is exact in float64."""
    return np.einsum("pgfr,pfr,phfr->pghr", K, var, K)
