"""Long-double twin of the delay null-space filter (``draco_amd/util/filters.py::null_filter``, ``DelayFilter``,
``DelayFilterBase``): the truth the GPU tests and the committed reference vectors are measured against.

Plain NumPy written from the formula.  The Fourier matrix of the symmetric modes ``linspace(-c, c, K)`` is taken in
its real form ``Fr`` (columns ``sqrt2 cos(2 pi f_k s)``, ``sqrt2 sin(2 pi f_k s)`` for ``f_k > 0``, ones for the zero mode
of an odd ``K``; rows scaled by mask and window), ``Fr Fr^T = F F^H``.  Its SVD is a one-sided Jacobi in
``numpy.longdouble`` (a round-robin sweep, all disjoint pairs of a step rotated at once), the kept subspace is
``sig > tol sig.max()``, the projector, the mask and the window are formed in long double and rounded once.
"""

import numpy as np

LD = np.longdouble
PI = np.arccos(LD(-1))
_WINDOW_COEF = {
    "uniform": (1.0, 0.0, 0.0, 0.0),
    "hann": (0.5, -0.5, 0.0, 0.0),
    "hanning": (0.5, -0.5, 0.0, 0.0),
    "hamming": (0.53836, -0.46164, 0.0, 0.0),
    "blackman": (0.42, -0.5, 0.08, 0.0),
    "nuttall": (0.355768, -0.487396, 0.144232, -0.012604),
    "blackman_nuttall": (0.3635819, -0.4891775, 0.1365995, -0.0106411),
    "blackman_harris": (0.35875, -0.48829, 0.14128, -0.01168),
}


def rel_err(a, b):
    """max |a - b| / max |b|."""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max() / np.abs(b).max())


def window_coef(samples, window):
    """The window of ``null_filter`` at the samples, long double (ones for a false ``window``)."""
    s = np.asarray(samples, dtype=np.float64).astype(LD)
    if not window:
        return np.ones(s.size, dtype=LD)
    name = "nuttall" if window is True else str(window)
    x = (s - s.min()) / (s.max() - s.min())
    a = [LD(c) for c in _WINDOW_COEF[name]]
    w = sum(a[i] * np.cos(2 * PI * i * x) for i in range(4))
    return np.where((x >= 0) & (x <= 1), w, LD(0))


def real_basis(samples, cutoff, mask, num_modes, window):
    """``Fr [n, K]`` in long double from the float64 samples and the float64 modes ``numpy.linspace`` gives."""
    s = np.asarray(samples, dtype=np.float64).astype(LD)
    K = int(num_modes)
    fmodes = np.linspace(-cutoff, cutoff, K)
    P = K // 2
    f = fmodes[K - P :].astype(LD)
    arg = (2 * PI * f)[np.newaxis, :] * s[:, np.newaxis]
    Fr = np.ones((s.size, K), dtype=LD)
    Fr[:, 0 : 2 * P : 2] = np.sqrt(LD(2)) * np.cos(arg)
    Fr[:, 1 : 2 * P : 2] = np.sqrt(LD(2)) * np.sin(arg)
    scale = np.asarray(mask).astype(bool).astype(LD) * window_coef(samples, window)
    return Fr * scale[:, np.newaxis]


def jacobi_svd(A, max_sweeps=60):
    """One-sided Jacobi on the columns of ``A`` (long double, not modified): ``(U sig, sig, sweeps)`` with the columns
    sorted by descending norm.  Pairs are skipped at ``|a_i . a_j| <= sqrt(n) eps |a_i| |a_j|`` (long-double eps) and where
    either norm is below ``1e-17`` of the largest: such a column is rounding noise in the span of the others, far under
    anything a float64 run can resolve, and rotating it would only shrink it by another factor eps per sweep."""
    A = np.array(A, dtype=LD)
    n, K = A.shape
    M = K + (K & 1)
    eps = np.sqrt(LD(n)) * np.finfo(LD).eps
    others = np.arange(1, M // 2)
    for sweep in range(1, max_sweeps + 1):
        moved = False
        nrm2 = (A * A).sum(axis=0)
        floor2 = LD(1e-34) * nrm2.max()
        for step in range(M - 1):
            a = np.concatenate([[M - 1], (step + others) % (M - 1)])
            b = np.concatenate([[step], (step - others) % (M - 1)])
            ok = (a < K) & (b < K)
            i, j = np.minimum(a, b)[ok], np.maximum(a, b)[ok]
            X, Y = A[:, i], A[:, j]
            al, be, ga = (X * X).sum(axis=0), (Y * Y).sum(axis=0), (X * Y).sum(axis=0)
            rot = (np.abs(ga) > eps * np.sqrt(al * be)) & (al >= floor2) & (be >= floor2)
            if not rot.any():
                continue
            moved = True
            gs = np.where(rot, ga, LD(1))
            zeta = (be - al) / (2 * gs)
            t = np.where(zeta >= 0, LD(1), LD(-1)) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
            c = 1 / np.sqrt(1 + t * t)
            s = c * t
            c, s = np.where(rot, c, LD(1)), np.where(rot, s, LD(0))
            A[:, i], A[:, j] = c * X - s * Y, s * X + c * Y
        if not moved:
            break
    else:
        raise RuntimeError("nullfilter_twin.jacobi_svd: no convergence")
    sig = np.sqrt((A * A).sum(axis=0))
    order = np.argsort(-sig, kind="stable")
    return A[:, order], sig[order], sweep


def null_filter_truth(samples, cutoff, mask, num_modes=200, tol=1e-8, window=True, type_="high", full=False):
    """The filter in long double; with ``full`` also ``(nkeep, sig)`` (``sig`` descending, long double)."""
    mask = np.asarray(mask).astype(bool)
    Fr = real_basis(samples, cutoff, mask, num_modes, window)
    US, sig, _ = jacobi_svd(Fr)
    nkeep = int((sig > LD(tol) * sig.max()).sum())
    U = US[:, :nkeep] / sig[:nkeep]
    proj = U @ U.T
    if type_ == "high":
        proj = np.eye(mask.size, dtype=LD) - proj
    proj = proj * (mask.astype(LD) * window_coef(samples, window))[np.newaxis, :]
    return (proj, nkeep, sig) if full else proj


def masks(weight2d):
    """``(f_mask, t_mask)`` of one item's weights ``[freq, other]``: the axis entries with the most positive samples."""
    pos = np.asarray(weight2d) > 0.0
    f_samp, t_samp = pos.sum(axis=1), pos.sum(axis=0)
    return f_samp == f_samp.max(), t_samp == t_samp.max()


def num_modes(freq, cut):
    return int(4.0 * np.ptp(freq) * cut + 0.5)


def filter_items(freq, cuts, data, weight, window, cache=None):
    """Filter ``data [freq, item, col]`` (any dtype) with ``weight [freq, item, col]`` and the cut of every item, in long
    double, rounded once to ``data``'s dtype; the weights are multiplied by the masks.  Returns ``(data, weight, info)``,
    ``info`` one ``(cut, K, f_mask, nkeep, sig)`` per distinct filter in order of first use."""
    cache = {} if cache is None else cache
    out, wout = np.array(data), np.array(weight)
    cplx = np.iscomplexobj(data)
    for it in range(data.shape[1]):
        fm, tm = masks(weight[:, it])
        K = num_modes(freq, cuts[it])
        key = (float(cuts[it]), K, fm.tobytes(), str(window))
        if key not in cache:
            nf, nkeep, sig = null_filter_truth(freq, cuts[it], fm, num_modes=K, window=window, full=True)
            cache[key] = (nf, (float(cuts[it]), K, fm, nkeep, sig))
        nf = cache[key][0]
        x = data[:, it]
        if cplx:
            y = (nf @ x.real.astype(LD)) + 1j * (nf @ x.imag.astype(LD))
        else:
            y = nf @ x.astype(LD)
        out[:, it] = y.astype(data.dtype)
        wout[:, it] = weight[:, it] * (fm[:, np.newaxis] & tm[np.newaxis, :]).astype(weight.dtype)
    return out, wout, [v[1] for v in cache.values()]
