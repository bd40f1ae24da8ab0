"""NumPy twin of the NRML delay power spectrum estimator (``draco/analysis/delayopt.py``): the model (data
covariance, masked Fourier matrix, noise, starting spectrum) and value, gradient and Hessian (exact and Fisher) of the
maximum a posteriori problem at a point ``x = log S``, in two forms:

* the f64 form: dense float64 / complex128 products and LAPACK's Cholesky, as the reference;
* the truth (``truth=True``): ``numpy.longdouble`` throughout -- window, Fourier matrix with arguments reduced in
  integers, covariance, the Cholesky factorisation of the real embedding (``chol_twin.chol_upper_ld``) and the solves --
  rounded once to float64 at the end.

A cut channel (``Ni == 0`` or a window coefficient that is exactly zero) is removed, as ``LogLikePS`` removes the zero
rows of ``MF``.  ``rel_err(a, b) = max |a - b| / max |b|``.
"""

import numpy as np
import scipy.linalg as la

import chol_twin
from delay_twin import LD, PI_LD, rel_err, window  # noqa: F401

CLD = np.clongdouble
BOUNDS = (1e-15, 1e10)


def matern_inverse(N):
    """``Ci`` of the reference's prior: ``inv(matern(N, width=5, nu=1.5) + 1e-8 I)``, float64 (an input of both forms)."""
    d = np.sqrt(np.subtract.outer(np.arange(N) / 5, np.arange(N) / 5) ** 2)
    d *= np.sqrt(3)
    K = (1.0 + d) * np.exp(-d)
    return la.inv(K + np.identity(N) * 1e-8)


def model(data, N, Ni, fsel, win, truth=False):
    """``dict(X, MF, Nm, nsamp, live, S0)``: the covariance of the windowed data, the masked Fourier matrix, the noise
    variance, the rows that are not cut, and the starting spectrum in its closed form: the variance over the samples of
    ``(1 / N) sum_f keep_f d_f exp(+2 pi i f a / N)`` on the unwindowed data, ``keep_f = |w_f| > 1e-3 max |w|`` over the
    channels with ``Ni != 0``."""
    rt, ct, pi = (LD, CLD, PI_LD) if truth else (np.float64, np.complex128, np.pi)
    fsel = np.asarray(fsel, dtype=np.int64)
    data = np.asarray(data).astype(ct)
    nsamp = data.shape[0]
    ang = 2 * pi * ((fsel[:, None] * np.arange(N, dtype=np.int64)[None, :]) % N).astype(rt) / rt(N)
    E = (np.cos(ang) - 1j * np.sin(ang)).astype(ct)
    w = np.ones(len(fsel), dtype=rt) if win is None else window(fsel, N, win, truth)
    Ni = np.asarray(Ni, dtype=np.float64)
    dw = data * w[None, :]
    X = dw.T @ dw.conj() / rt(nsamp)
    MF = E * w[:, None]
    MF[Ni == 0] = 0
    live = (Ni != 0) & (w != 0)
    wl = np.abs(w[Ni != 0])
    keep = (Ni != 0) & (np.abs(w) > rt(1e-3) * (wl.max() if wl.size else 0))
    z = (data * keep[None, :]) @ E.conj() / rt(N)
    zm = z.mean(axis=0)
    S0 = (np.abs(z - zm[None, :]) ** 2).mean(axis=0)
    Nm = np.zeros(len(fsel), dtype=rt)
    Nm[Ni != 0] = 1 / Ni[Ni != 0].astype(rt)
    return dict(X=X, MF=MF, Nm=Nm, nsamp=nsamp, live=live, S0=S0, w=w, keep=keep)


def covariance(m, x, bounds=BOUNDS):
    """``C = MF diag(S) MF^H + diag(Nm)`` on the rows that are not cut."""
    lo, hi = sorted(np.log(b) for b in bounds)
    MF = m["MF"][m["live"]]
    S = np.exp(np.clip(np.asarray(x, dtype=MF.real.dtype), lo, hi))
    Cm = (MF * S[None, :]) @ MF.conj().T
    Cm[np.diag_indices_from(Cm)] += m["Nm"][m["live"]]
    return Cm, MF, S


def evaluate(m, x, Ci, truth=False, bounds=BOUNDS):
    """``dict(value, grad, hess, fisher)`` of likelihood plus prior at ``x``, float64 (the truth rounded once).  Raises
    ``numpy.linalg.LinAlgError`` if ``C`` is not positive definite."""
    rt = LD if truth else np.float64
    live = m["live"]
    Cm, MF, S = covariance(m, x, bounds)
    X = m["X"][live][:, live]
    n = MF.shape[0]
    U = MF * np.sqrt(S)[None, :]
    if truth:
        G = np.block([[Cm.real, -Cm.imag], [Cm.imag, Cm.real]])
        Uf = chol_twin.chol_upper_ld(G)
        lndet = np.log(np.diag(Uf)).sum()  # log det G = 2 log det C = 2 sum log diag

        def solve(B):
            rows = np.concatenate([B.real, B.imag], axis=0).T
            sol = chol_twin.solve_rows_ld(Uf, rows).T
            return sol[:n] + 1j * sol[n:]
    else:
        ch = la.cho_factor(Cm, check_finite=False)
        lndet = 2 * np.log(np.diag(ch[0]).real).sum()

        def solve(B):
            return la.cho_solve(ch, B, check_finite=False)
    Ut = solve(U)
    R = (X - Cm) @ Ut
    ns = rt(m["nsamp"])
    xr = np.asarray(x, dtype=rt)
    cix = Ci.astype(rt) @ xr
    value = ns * (lndet + np.trace(solve(X)).real) + xr @ cix / 2
    t = -(Ut.conj() * R).real.sum(axis=0)
    grad = ns * t + cix
    P = U.conj().T @ Ut
    Q = Ut.conj().T @ R
    fisher = (P * P.T.conj()).real  # P is Hermitian, so this is Re(P_ab^2) = Pr^2 - Pi^2: the reference's form, not |P_ab|^2
    hess = fisher + 2 * (Q * P.conj()).real
    hess[np.diag_indices_from(hess)] += t
    return dict(value=np.float64(value), grad=grad.astype(np.float64), hess=(ns * hess + Ci).astype(np.float64), fisher=(ns * fisher + Ci).astype(np.float64))


def cond(m, x):
    """The 2-norm condition number of ``C`` at ``x`` (float64 form)."""
    return float(np.linalg.cond(np.asarray(covariance(m, x)[0], dtype=np.complex128)))
