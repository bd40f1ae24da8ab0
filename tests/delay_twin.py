"""NumPy twin of the delay spectrum estimators (``draco/analysis/delay.py:461-597, 877-1106, 1480-1710, 2102-2201``),
in two forms:

* the f64 form: the reference's algorithm in the reference's dtypes with the same BLAS / LAPACK calls (dense Fourier
  matrix, ``F^T N^-1 F`` as a matrix product, ``scipy.linalg.cho_factor`` / ``cho_solve``);
* the truth form (``truth=True``): ``numpy.longdouble`` throughout -- Fourier matrix with arguments reduced in integers,
  window, means, products, Cholesky factorisation and solves -- rounded once to complex128 at the end.

``rel_err(a, b) = max |a - b| / max |b|``.
"""

import numpy as np
import scipy.linalg as la

LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288")

WINDOWS = {
    "uniform": (1, 0, 0, 0),
    "hann": (0.5, -0.5, 0, 0),
    "hanning": (0.5, -0.5, 0, 0),
    "hamming": (0.53836, -0.46164, 0, 0),
    "blackman": (0.42, -0.5, 0.08, 0),
    "nuttall": (0.355768, -0.487396, 0.144232, -0.012604),
    "blackman_nuttall": (0.3635819, -0.4891775, 0.1365995, -0.0106411),
    "blackman_harris": (0.35875, -0.48829, 0.14128, -0.01168),
}


def rel_err(a, b):
    """max |a - b| / max |b|."""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def inz(x):
    x = np.asarray(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0, 0, 1 / np.where(x == 0, 1, x)).astype(x.dtype)


def window(num, den, name, truth=False):
    """The cosine-sum window ``sum_k a_k cos(2 pi k x)`` at ``x = num / den`` (integers), zero outside [0, 1]."""
    dt, pi = (LD, PI_LD) if truth else (np.float64, np.pi)
    x = np.asarray(num, dtype=dt) / dt(den)
    w = np.zeros(x.shape, dtype=dt)
    for k, a in enumerate(WINDOWS[name]):
        w += dt(a) * np.cos(2 * pi * k * x)
    w[(x < 0) | (x > 1)] = 0
    return w


def trig_tables(N, fsel, truth=False):
    """``cos`` and ``sin`` of ``2 pi f t / N`` as ``[nsel, N]`` tables.  The f64 form takes the angle as the product
    it is; the truth reduces ``f t`` modulo ``N`` in integers first."""
    f, t = np.asarray(fsel, dtype=np.int64), np.arange(N, dtype=np.int64)
    if truth:
        ang = 2 * PI_LD * (np.multiply.outer(f, t) % N).astype(LD) / LD(N)
    else:  # rounded as the reference's matrices are: (2 pi t) f / N in float64, no reduction
        ang = np.multiply.outer(f, 2 * np.pi * t) / N
    return np.cos(ang), np.sin(ang)


def fourier(N, fsel, complex_td, truth=False):
    """The real-valued Fourier matrix over the channels ``fsel``: rows are (Re, Im) per channel.  Real time domain
    ``[2 nsel, N]``: the pair is (cos, -sin).  Complex time domain ``[2 nsel, 2 N]``: per (channel, sample) the 2 x 2
    rotation ``[[cos, sin], [-sin, cos]]`` acting on (Re, Im) of the sample."""
    c, s = trig_tables(N, fsel, truth)
    if not complex_td:
        return np.stack([c, -s], axis=1).reshape(2 * c.shape[0], N)
    rot = np.stack([np.stack([c, s], axis=-1), np.stack([-s, c], axis=-1)], axis=1)  # [nsel, 2, N, 2]
    return rot.reshape(2 * c.shape[0], 2 * N)


def row_weights(N, Ni, fsel, complex_td, dt):
    """Inverse noise of the (Re, Im) rows: twice ``Ni`` on both, except that channels 0 and N / 2 of a real time
    domain are strictly real (``Ni`` on the real row, nothing on the imaginary one)."""
    Ni = np.asarray(Ni)
    nw = np.repeat(2 * Ni, 2).astype(dt)
    if not complex_td:
        edge = np.flatnonzero((np.asarray(fsel) == 0) | (np.asarray(fsel) == N // 2))
        nw[2 * edge] = Ni[edge]
        nw[2 * edge + 1] = 0
    return nw


def inverse_signal(delay_PS, complex_td, dt):
    """``1 / PS`` where it is non-zero; per (Re, Im) component, each of half the power, in the complex time domain."""
    Si = inz(np.asarray(delay_PS, dtype=dt))
    return 2 * np.repeat(Si, 2) if complex_td else Si


def cholesky_solve_ld(a, y):
    """Solve ``a x = y`` (``y [n, nrhs]``) through the long-double Cholesky factor ``a = U^T U``; raises
    ``numpy.linalg.LinAlgError`` on a non-positive pivot."""
    a = np.array(a, dtype=LD)
    y = np.array(y, dtype=LD)
    n = a.shape[0]
    for k in range(n):
        if not a[k, k] > 0:
            raise np.linalg.LinAlgError(f"pivot {k} is not positive")
        a[k, k:] /= np.sqrt(a[k, k])
        if k + 1 < n:
            a[k + 1 :, k + 1 :] -= a[k, k + 1 :, np.newaxis] * a[k, np.newaxis, k + 1 :]
    for k in range(n):  # U^T z = y
        y[k] /= a[k, k]
        if k + 1 < n:
            y[k + 1 :] -= a[k, k + 1 :, np.newaxis] * y[k][np.newaxis, :]
    for k in range(n - 1, -1, -1):  # U x = z
        y[k] /= a[k, k]
        if k > 0:
            y[:k] -= a[:k, k, np.newaxis] * y[k][np.newaxis, :]
    return y


def _whitened(N, Ni, fsel, win, complex_td, truth):
    """``A = sqrt(N^-1) W F`` (rows scaled by the window, then by the root inverse noise) and the two row scales."""
    dt = LD if truth else np.float64
    total = N if complex_td else N // 2 + 1
    root = np.sqrt(row_weights(N, Ni if not truth else np.asarray(Ni, dtype=LD), fsel, complex_td, dt))
    taper = np.repeat(window(fsel, total, win, truth), 2) if win is not None else np.ones(root.shape, dtype=dt)
    return fourier(N, fsel, complex_td, truth) * taper[:, np.newaxis] * root[:, np.newaxis], taper, root


def wiener_matrix(N, Ni, fsel, win, complex_td, delay_PS):
    """The Wiener matrix ``F^T N^-1 F + S^-1`` in float64, formed as a matrix product (for condition numbers and for
    the circulant check)."""
    A = _whitened(N, Ni, np.asarray(fsel), win, complex_td, False)[0]
    return A.T @ A + np.diag(inverse_signal(delay_PS, complex_td, np.float64))


def wiener(delay_PS, data, N, Ni, win="nuttall", fsel=None, complex_td=False, truth=False):
    """The Wiener-filter estimate ``(F^T N^-1 F + S^-1)^-1 F^T N^-1 d`` per sample: ``[nsample, N]``, real in the
    real time domain.  f64 form: dense products and LAPACK's Cholesky, as the reference; truth: long double."""
    dt = LD if truth else np.float64
    fsel = np.arange(N if complex_td else N // 2 + 1) if fsel is None else np.asarray(fsel)
    A, taper, root = _whitened(N, Ni, fsel, win, complex_td, truth)
    z = np.asarray(data)
    d = np.stack([z.real.astype(dt), z.imag.astype(dt)], axis=-1).reshape(z.shape[0], -1)  # (Re, Im) interleaved
    G = A.T @ A
    G[np.diag_indices_from(G)] += inverse_signal(delay_PS, complex_td, dt)
    y = A.T @ (d * taper * root).T
    x = cholesky_solve_ld(G, y).T if truth else la.cho_solve(la.cho_factor(G, check_finite=False), y, check_finite=False).T
    if not complex_td:
        return x
    pair = x.reshape(x.shape[0], -1, 2)
    return pair[..., 0] + 1j * pair[..., 1]


def fft_estimate(data, N, win="nuttall", truth=False):
    """``delay_spectrum_fft``: the window at ``arange(N) / N``, then the inverse FFT (a long-double DFT for the truth)."""
    if truth:
        z = np.asarray(data)
        if z.shape[-1] != N:
            raise ValueError("operands could not be broadcast together")
        w = window(np.arange(N), N, win, True) if win is not None else np.ones(N, dtype=LD)
        k = (np.arange(N)[:, np.newaxis] * np.arange(N)[np.newaxis, :]) % N
        arg = 2 * PI_LD * k.astype(LD) / LD(N)
        c, s = np.cos(arg), np.sin(arg)
        dr, di = z.real.astype(LD) * w, z.imag.astype(LD) * w
        return (dr @ c - di @ s) / LD(N) + 1j * ((dr @ s + di @ c) / LD(N))
    if win is not None:
        data *= window(np.arange(N), N, win)[np.newaxis]
    return np.fft.ifft(data, axis=-1)


def cut_data(data, weight, cfg, truth=False):
    """The cuts on one baseline's ``[sample, freq]`` block (averaged weights, no ``scale_freq``): ``(data, Ni, nzf,
    nzt)`` or ``None`` if the baseline is skipped.  A sample stays if its share of channels with positive weight is
    above ``time_frac``; a channel stays if its share of such samples, among those kept, is above ``freq_frac``.  The
    f64 form keeps the container's dtypes in the means, as the reference does; the truth takes them in long double."""
    good = weight > 0
    if not good.any():
        return None
    nzt = good.mean(axis=1) > cfg["time_frac"]
    with np.errstate(invalid="ignore"):
        nzf = good[nzt].mean(axis=0) > cfg["freq_frac"]
    if not nzf.any():
        return None
    # (samples first, then channels, as two selections: the memory order of the result decides the order of the
    # single-precision sums below, and the f64 form has to round as the reference does)
    data, weight = data[nzt][:, nzf], weight[nzt][:, nzf]
    if truth:
        data = data.astype(np.clongdouble) if np.iscomplexobj(data) else data.astype(LD)
        weight = weight.astype(LD)
    if cfg["remove_mean"]:
        data = data - data.mean(axis=0, keepdims=True)
    if not data.any():
        return None
    boost = LD(cfg["weight_boost"]) if truth else weight.dtype.type(cfg["weight_boost"])
    return data, weight.mean(axis=0) * boost, nzf, nzt


def evaluate(data_view, weight_view, prior, ndelay, channel_ind, cfg, estimator, truth=False):
    """``DelaySpectrumBase._evaluate`` on ``[baseline, sample, freq]`` views: ``(spectrum [baseline, sample, ndelay]``
    complex128, ``mask [baseline, sample])``.  ``cfg``: time_frac, freq_frac, remove_mean, weight_boost, window (None:
    no apodisation), complex_timedomain.  ``estimator``: 'wiener' (``prior [baseline, ndelay]``) or 'fft'."""
    nbase, nsample = data_view.shape[:2]
    spec = np.zeros((nbase, nsample, ndelay), dtype=np.complex128)
    mask = np.zeros((nbase, nsample), dtype=bool)
    for bi in range(nbase):
        t = cut_data(data_view[bi], weight_view[bi], cfg, truth)
        if t is None:
            mask[bi] = True
            continue
        data, weight, nzf, nzt = t
        if estimator == "wiener":
            y = wiener(np.fft.fftshift(prior[bi]), data, ndelay, weight, cfg["window"], channel_ind[nzf], cfg["complex_timedomain"], truth)
        else:
            y = fft_estimate(data, ndelay, cfg["window"], truth)
        spec[bi, nzt] = np.fft.fftshift(y, axes=-1)
        mask[bi][~nzt] = True
    return spec, mask


def power_spectrum(spec, mask=None):
    """``DelaySpectrumToPowerSpectrum.process``: ``(ps [baseline, ndelay], flagged [baseline])``."""
    w = None if mask is None else ~mask[..., np.newaxis]
    with np.errstate(invalid="ignore", divide="ignore"):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ps = np.var(spec, axis=1, where=w) if w is not None else np.var(spec, axis=1)
    nans = np.isnan(ps)
    ps[nans] = 0.0
    return ps, np.any(nans, axis=-1)
