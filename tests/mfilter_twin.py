"""Plain NumPy restatement of the DAYENU m-mode filter (``draco/analysis/dayenu.py:977-1122, 1235-1427``).

Two forms of the same steps (per frequency: RA mask, cuts, covariance of each kind, inverse, mixer, apply):

* the **f64 form** does what the reference does, ``numpy.linalg.pinv(..., hermitian=True)`` included;
* the **truth form** builds the covariance in long double from the float64 cuts, inverts the unflagged block by a
  long-double Cholesky factorisation (``dayenu_twin.cholesky_inverse_ld``), takes the mixer in long double and applies
  in long double; the caller gets it rounded to complex64.

The covariance kinds are ``"lowpass"``, ``"bandpass"`` and ``"highpass"``.
"""

import numpy as np

from dayenu_twin import C_LIGHT, LD, PI_LD, _sinc_ld, cholesky_inverse_ld, rel_err  # noqa: F401

CLD = np.clongdouble


def instantaneous_m(ha, lat, dec, u, v, w=0.0):
    d = u * (-np.cos(dec) * np.cos(ha)) + v * (np.sin(lat) * np.cos(dec) * np.sin(ha)) + w * (-np.cos(lat) * np.cos(dec) * np.sin(ha))
    return 2.0 * np.pi * d


def get_cut(freq, xsep, latitude, dec):
    """``DayenuMFilter._get_cut``: ``freq`` in MHz, ``xsep`` in metres, ``latitude`` and ``dec`` in degrees."""
    return instantaneous_m(0.0, np.radians(latitude), np.radians(dec), xsep / (C_LIGHT / (freq * 1e6)), 0.0)


def covariance(ra, kind, m_cut, m_center, epsilon, truth=False):
    T = LD if truth else np.float64
    pi = PI_LD if truth else np.pi
    r = np.asarray(ra, dtype=T)
    dra = r[:, np.newaxis] - r[np.newaxis, :]
    x = T(m_cut) * dra / pi
    sinc = _sinc_ld(x) if truth else np.sinc(x)
    eye = np.eye(r.size, dtype=T)
    if kind == "highpass":
        return eye + sinc / T(epsilon)
    a = T(np.median(np.abs(np.diff(np.asarray(ra, dtype=np.float64))))) * T(m_cut) / pi
    aeps = a * T(epsilon)
    if kind == "lowpass":
        return eye / aeps + a * (1 - 1 / aeps) * sinc
    assert kind == "bandpass"
    return eye / aeps + 2 * a * (1 - 1 / aeps) * sinc * np.cos(T(m_center) * dra)


def _index(flag, nra):
    uflag, uindex = np.unique(flag.reshape(-1, nra), return_inverse=True, axis=0)
    uindex = np.asarray(uindex).reshape(-1)
    return uflag, [np.unravel_index(np.flatnonzero(uindex == uu), flag.shape[:-1]) for uu in range(uflag.shape[0])]


def mmode_filter_f64(ra, kind, m_cut, m_center, flag, epsilon=1e-10):
    """The three builder functions: ``(pinv [nuniq, nra, nra], index)``."""
    cov = covariance(ra, kind, m_cut, m_center, epsilon)
    uflag, index = _index(np.asarray(flag, dtype=bool), ra.size)
    uflag = (uflag[:, np.newaxis, :] & uflag[:, :, np.newaxis]).astype(np.float64)
    return np.linalg.pinv(uflag * cov[np.newaxis], hermitian=True) * uflag, index


def filter_truth(ra, kind, m_cut, m_center, flag, epsilon=1e-10):
    """The filter of one mask ``flag [nra]``: the long-double inverse of the unflagged block, zeros elsewhere."""
    flag = np.asarray(flag, dtype=bool).reshape(-1)
    cov = covariance(ra, kind, m_cut, m_center, epsilon, truth=True)
    out = np.zeros(cov.shape, dtype=LD)
    sel = np.flatnonzero(flag)
    if sel.size:
        out[np.ix_(sel, sel)] = cholesky_inverse_ld(cov[np.ix_(sel, sel)])
    return out


def mmode_filter_truth(ra, kind, m_cut, m_center, flag, epsilon=1e-10):
    uflag, index = _index(np.asarray(flag, dtype=bool), ra.size)
    return np.stack([filter_truth(ra, kind, m_cut, m_center, u, epsilon) for u in uflag]), index


def ew_separation(feedpos, prod, spacing):
    b = feedpos[prod["input_a"], 0] - feedpos[prod["input_b"], 0]
    return np.round(b / spacing) * spacing


def ra_mask(weight_f):
    """``(gb, flag [nra])`` of one frequency's ``weight [nstack, nra]``; ``flag`` is ``None`` where ``gb`` is empty."""
    good = weight_f > 0.0
    gb = np.flatnonzero(np.any(good, axis=-1))
    if gb.size == 0:
        return gb, None
    return gb, np.sum(good[gb, :], axis=0) > (0.90 * float(gb.size))


def filter_stream(freq, ra_deg, feedpos, prod, spacing, latitude, vis, weight, dec=40.0, epsilon=1e-10, fkeep_intra=0.75, fkeep_inter=0.75, truth=False):
    """``DayenuMFilter.process`` on ``vis`` / ``weight [nfreq, nstack, nra]``: ``(vis, weight)`` of the containers'
    dtypes (the truth rounded to them)."""
    ra = np.radians(np.asarray(ra_deg, dtype=np.float64))
    sep = ew_separation(feedpos, prod, spacing)
    db = 0.5 * spacing
    ov, ow = vis.copy(), weight.copy()
    for ff, nu in enumerate(freq):
        gb, flag = ra_mask(weight[ff])
        if flag is None:
            continue
        ow[ff] *= flag[np.newaxis, :].astype(weight.dtype)
        if not np.any(flag):
            continue
        m_cut = np.abs(get_cut(nu, db, latitude, dec))
        kinds = {True: ("bandpass", 0.5 * fkeep_intra * m_cut, 0.5 * (2.0 - fkeep_intra) * m_cut), False: ("lowpass", fkeep_inter * m_cut, 0.0)}
        filt = {}
        for ss, ub in enumerate(sep):
            intra = bool(np.abs(ub) < db)
            if intra not in filt:
                kind, mc, m0 = kinds[intra]
                filt[intra] = filter_truth(ra, kind, mc, m0, flag, epsilon) if truth else mmode_filter_f64(ra, kind, mc, m0, flag[np.newaxis, :], epsilon)[0][0]
            v = vis[ff, ss].astype(CLD if truth else np.complex128)
            if intra:
                out = filt[intra] @ v.real + 1j * (filt[intra] @ v.imag) if truth else filt[intra] @ v
            else:
                arg = (LD(get_cut(nu, ub, latitude, dec)) * ra.astype(LD)) if truth else get_cut(nu, ub, latitude, dec) * ra
                mixer = np.cos(arg) - 1j * np.sin(arg)
                vm = v * mixer
                out = (filt[intra] @ vm.real + 1j * (filt[intra] @ vm.imag) if truth else filt[intra] @ vm) * mixer.conj()
            ov[ff, ss] = out.astype(vis.dtype)
    return ov, ow
