"""Plain NumPy restatement of the DAYENU delay filter (``draco/analysis/dayenu.py:20-193, 776-975, 1125-1232``).

Two forms of the same five steps (per item: single mask, covariance, inverse, apply, attenuation mask):

* the **f64 form** does what the reference does, ``numpy.linalg.pinv(..., hermitian=True)`` included;
* the **truth form** builds the covariance in long double, inverts the unflagged block by a long-double Cholesky
  factorisation and applies it in long double.  ``1 / weight`` is taken in the container's dtype in both forms, as the
  reference's ``invert_no_zero`` on the dataset does; the caller rounds the truth to the container's dtype.

The reference's own result is about 1e-3 (relative) away from the truth at ``epsilon = 1e-12`` (condition number
1e13); the tests measure every implementation by its distance to the truth.
"""

import numpy as np

LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288")
C_LIGHT = 299792458.0


def inz(x):
    x = np.asarray(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0, 0, 1 / np.where(x == 0, 1, x)).astype(x.dtype)


def get_cut(feedpositions, prod, za_cut, orientation, tauw):
    """``DayenuDelayFilter._get_cut`` (``dayenu.py:177-192``)."""
    b = feedpositions[prod["input_a"], :] - feedpositions[prod["input_b"], :]
    if orientation == "NS":
        b = abs(b[:, 1])
    elif orientation == "EW":
        b = abs(b[:, 0])
    else:
        b = np.sqrt(np.sum(b**2, axis=-1))
    return 1e6 * za_cut * b / C_LIGHT + tauw


def _bands(tau_width, epsilon):
    tw = np.atleast_1d(np.asarray(tau_width, dtype=np.float64))
    ep = np.atleast_1d(np.asarray(epsilon, dtype=np.float64))
    n = max(tw.size, ep.size)
    return np.broadcast_to(tw, (n,)), np.broadcast_to(ep, (n,))


def covariance(freq, tau_width, epsilon):
    dfreq = freq[:, np.newaxis] - freq[np.newaxis, :]
    cov = np.eye(freq.size, dtype=np.float64)
    for tw, eps in zip(*_bands(tau_width, epsilon)):
        cov += np.sinc(2.0 * tw * dfreq) / eps
    return cov


def delay_filter_f64(freq, flag, tau_width, epsilon=1e-12):
    """``delay_filter`` with ``tau_centre = 0`` (``dayenu.py:1125-1202``): ``(pinv [nuniq, nfreq, nfreq], index)``."""
    nfreq = freq.size
    cov = covariance(freq, tau_width, epsilon)
    uflag, uindex = np.unique(flag.reshape(nfreq, -1), return_inverse=True, axis=-1)
    uindex = np.asarray(uindex).reshape(-1)
    uflag = uflag.T
    uflag = uflag[:, np.newaxis, :] & uflag[:, :, np.newaxis]
    ucov = uflag * cov[np.newaxis, :, :]
    pinv = np.linalg.pinv(ucov, hermitian=True) * uflag
    index = [np.flatnonzero(uindex == uu) for uu in range(pinv.shape[0])]
    return pinv, index


def _sinc_ld(x):
    x = np.asarray(x, dtype=LD)
    y = PI_LD * np.where(x == 0, LD(1), x)
    return np.where(x == 0, LD(1), np.sin(y) / y)


def cholesky_inverse_ld(a):
    """Inverse of a symmetric positive definite matrix through its long-double Cholesky factor."""
    n = a.shape[0]
    a = np.array(a, dtype=LD)
    low = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = a[j, j] - np.dot(low[j, :j], low[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError("matrix is not positive definite")
        low[j, j] = np.sqrt(d)
        low[j + 1 :, j] = (a[j + 1 :, j] - low[j + 1 :, :j] @ low[j, :j]) / low[j, j]
    y = np.zeros((n, n), dtype=LD)  # L y = I
    for i in range(n):
        rhs = -(low[i, :i] @ y[:i, :])
        rhs[i] += 1
        y[i, :] = rhs / low[i, i]
    return y.T @ y


def filter_truth(freq, flag, tau_width, epsilon=1e-12):
    """The filter of one mask ``flag [nfreq]``: the long-double inverse of the unflagged block, zeros elsewhere."""
    flag = np.asarray(flag, dtype=bool).reshape(-1)
    f = np.asarray(freq, dtype=LD)
    dfreq = f[:, np.newaxis] - f[np.newaxis, :]
    cov = np.eye(f.size, dtype=LD)
    for tw, eps in zip(*_bands(tau_width, epsilon)):
        cov = cov + _sinc_ld(2 * LD(tw) * dfreq) / LD(eps)
    out = np.zeros((f.size, f.size), dtype=LD)
    sel = np.flatnonzero(flag)
    if sel.size:
        out[np.ix_(sel, sel)] = cholesky_inverse_ld(cov[np.ix_(sel, sel)])
    return out


def delay_filter_truth(freq, flag, tau_width, epsilon=1e-12):
    nfreq = freq.size
    uflag, uindex = np.unique(flag.reshape(nfreq, -1), return_inverse=True, axis=-1)
    uindex = np.asarray(uindex).reshape(-1)
    pinv = np.stack([filter_truth(freq, uflag[:, u], tau_width, epsilon) for u in range(uflag.shape[1])])
    return pinv, [np.flatnonzero(uindex == uu) for uu in range(pinv.shape[0])]


def atten_flag(diag, atten_threshold):
    diag = np.asarray(diag)
    return diag > (atten_threshold * np.median(diag[diag > 0.0]))


def filter_item(freq, cut, vis, weight, epsilon=1e-12, atten_threshold=0.0, truth=False):
    """One item, ``vis`` / ``weight [nfreq, ncol]``: ``(vis, weight, flag_low)``, or ``None`` if it is skipped.  f64 form:
    arrays of the container's dtypes, assigned as the reference does.  Truth form: long double, not rounded."""
    flag = np.all(weight > 0.0, axis=-1, keepdims=True)
    weight = weight * flag.astype(weight.dtype)
    if not np.any(flag):
        return None
    bvar = inz(weight)
    if truth:
        nf = filter_truth(freq, flag, cut, epsilon)
        cplx = np.iscomplexobj(vis)
        ov = nf @ vis.real.astype(LD) + (1j * (nf @ vis.imag.astype(LD)) if cplx else 0)
        ow = inz((nf * nf) @ bvar.astype(LD))
    else:
        nf = delay_filter_f64(freq, flag, cut, epsilon)[0][0]
        ov = np.matmul(nf, vis).astype(vis.dtype)
        ow = inz(np.matmul(nf**2, bvar)).astype(weight.dtype)
    low = None
    if atten_threshold > 0.0:
        low = atten_flag(np.diag(nf).astype(np.float64) if not truth else np.diag(nf), atten_threshold)
        ow = ow * low[:, np.newaxis].astype(ow.dtype)
    return ov, ow, low


def filter_stream(freq, cutoff, vis, weight, epsilon=1e-12, atten_threshold=0.0, truth=False):
    """``DayenuDelayFilter.process`` on ``vis`` / ``weight [nfreq, nstack, nra]``; the truth comes back rounded to the
    container's dtypes."""
    ov, ow = vis.copy(), weight.copy()
    for bb, cut in enumerate(cutoff):
        ow[:, bb] *= np.all(weight[:, bb] > 0.0, axis=-1, keepdims=True).astype(weight.dtype)
        r = filter_item(freq, cut, vis[:, bb], weight[:, bb], epsilon, atten_threshold, truth)
        if r is not None:
            ov[:, bb], ow[:, bb] = r[0].astype(vis.dtype), r[1].astype(weight.dtype)
    return ov, ow


def filter_ringmap(freq, cut, rmap, weight, epsilon=1e-12, atten_threshold=0.0, truth=False):
    """``DayenuDelayFilterMap.process`` on ``map [beam, pol, freq, ra, el]`` / ``weight [pol, freq, ra, el]``, one
    beam."""
    assert rmap.shape[0] == 1
    om, ow = rmap.copy(), weight.copy()
    for pp in range(rmap.shape[1]):
        for ee in range(rmap.shape[-1]):
            w = weight[pp, :, :, ee]
            ow[pp, :, :, ee] *= np.all(w > 0.0, axis=-1, keepdims=True).astype(weight.dtype)
            r = filter_item(freq, cut, rmap[0, pp, :, :, ee], w, epsilon, atten_threshold, truth)
            if r is not None:
                om[0, pp, :, :, ee], ow[pp, :, :, ee] = r[0].astype(rmap.dtype), r[1].astype(weight.dtype)
    return om, ow


def rel_err(a, b):
    """max |a - b| / max |b|."""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())
