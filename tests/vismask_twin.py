"""An independent NumPy twin of the transient RFI mask from visibilities (``draco_amd/analysis/flagging.py``,
``RFITransientVisMask``, and the kernels of ``csrc/vismask.hip``): the Stokes-I sum, the weighted FIR filter as direct
sums in a chosen precision (long double for the truth, float64 for the error a float64 sum has anyway), a direct DFT in
long double, the hysteresis threshold by connected-component labelling, and the whole task as a replay.  SIR and the
medians are those of ``rfi_twin.py``.  It shares no code with the library; the argument handling (the design of the
taps, the order of the task's steps) necessarily says what the reference says, since that is what is being pinned.
Plain loops, meant for small cubes.
"""

import numpy as np
from scipy import ndimage, signal

import rfi_twin

LD = np.longdouble
CLD = np.clongdouble
SPEED_OF_LIGHT = 299792458.0


def stokes_i(vis, weight, ptr, rows):
    """Per baseline the sum of its rows in table order, in the arrays' own precision, from a zero."""
    nf, _, nt = vis.shape
    nbase = len(ptr) - 1
    vi, wi = np.zeros((nf, nbase, nt), dtype=vis.dtype), np.zeros((nf, nbase, nt), dtype=weight.dtype)
    for b in range(nbase):
        for r in rows[ptr[b] : ptr[b + 1]]:
            vi[:, b] += vis[:, r]
            wi[:, b] += weight[:, r]
    return vi, wi


def design(samples, cutoff):
    fs = 1 / np.median(abs(np.diff(samples)))
    order = int(np.ceil(fs / cutoff) // 2 * 2 + 1)
    return signal.firwin(order, cutoff, window="flattop", fs=fs)


def wconv(data, weight, taps, highpass=False, real=LD):
    """Rows of ``data [..., n]``: ``vw[t] = sum_j taps[j] (d w)[t + c - j]``, ``ww`` likewise, ``lp = vw inz(ww)``, all
    in the precision ``real`` in ascending ``j``; returns ``lp`` or ``d - lp`` in that precision."""
    data, weight = np.asarray(data), np.asarray(weight)
    cplx = np.iscomplexobj(data)
    ctype = (CLD if real is LD else np.complex128) if cplx else real
    d = data.astype(ctype)
    w = np.broadcast_to(weight, data.shape).astype(real)
    h = np.asarray(taps).astype(real)
    n, ntap = d.shape[-1], len(h)
    c = (ntap - 1) // 2
    dw = d * w
    pad = [(0, 0)] * (d.ndim - 1) + [(2 * c, 2 * c)]
    dwp, wp = np.pad(dw, pad), np.pad(w, pad)
    vw, ww = np.zeros(d.shape, dtype=ctype), np.zeros(d.shape, dtype=real)
    for j in range(ntap):  # sample t + c - j sits at t + 3 c - j of the padded row
        s = slice(3 * c - j, 3 * c - j + n)
        vw = vw + h[j] * dwp[..., s]
        ww = ww + h[j] * wp[..., s]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(ww == 0, real(0), real(1) / np.where(ww == 0, real(1), ww))
    lp = vw * inv
    return d - lp if highpass else lp


def beam_dft(x):
    """``|sum_s x[..., s, t] exp(-2 pi i k s / n)|`` over the axis before the last, a direct sum in long double."""
    x = np.asarray(x).astype(CLD)
    n = x.shape[-2]
    ks = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n  # exact phase reduction
    ang = -2 * (LD(4) * np.arctan(LD(1))) * ks.astype(LD) / LD(n)  # (np.pi is a double: pi in long double is 4 atan 1)
    W = np.cos(ang) + 1j * np.sin(ang)
    out = np.einsum("ks,...st->...kt", W.astype(CLD), x)
    return np.abs(out)


def hysteresis(x, low, high):
    """True above ``low`` where the 4-connected region above ``low`` holds a sample above ``high`` (planes one by one)."""
    x = np.asarray(x, dtype=np.float64)
    low = min(low, high)
    if x.ndim > 2:
        return np.stack([hysteresis(p, low, high) for p in x])
    with np.errstate(invalid="ignore"):
        lo, hi = x > low, x > high
    labels, n = ndimage.label(lo)  # the default structure: a cross
    if n == 0:
        return np.zeros(x.shape, dtype=bool)
    sums = ndimage.sum_labels(hi, labels, index=np.arange(n + 1))
    connected = sums > 0
    connected[0] = False
    return connected[labels]


def transient_mask(vis, weight, mask, freq, baselines, times, unix_to_lsa, latitude, mad_base_size=(1, 101), mad_dev_size=(1, 51), sigma_high=8.0, sigma_low=2.0,
                   frac_samples=0.01, hp=None, trace=None, stages=None):
    """The replay of ``RFITransientVisMask.generate_mask`` on ``[nfreq, nbeam, ntime]`` arrays.  ``hp``: a function
    ``(ii, vis, weight, ra, cutoff) -> filtered plane`` that replaces the long-double high-pass; ``trace``: a list that
    receives the MAD ratio of every processed frequency; ``stages``: a dict that receives ``hyst`` (the flag cube after
    the hysteresis), ``high`` (the samples above ``sigma_high``), ``final`` (the cube after SIR) and ``count``."""
    ra = np.unwrap(unix_to_lsa(times), period=360.0) * np.pi / 180.0
    cut = np.min(freq) * 1e6 / SPEED_OF_LIGHT * np.asarray(baselines)[:, 0].max() / np.cos(np.deg2rad(latitude))
    taps = design(ra, cut)
    mask = np.asarray(mask, dtype=bool)
    fl = np.zeros(vis.shape, dtype=bool) | mask[:, None, :]
    high = np.zeros(vis.shape, dtype=bool)
    for ii in range(vis.shape[0]):
        if mask[ii].all():
            continue
        v = wconv(vis[ii], weight[ii], taps, highpass=True) if hp is None else hp(ii, vis[ii], weight[ii], ra, cut)
        beams = np.asarray(beam_dft(v), dtype=np.float64)
        ratio = rfi_twin.mad(beams, fl[ii], mad_base_size, mad_dev_size)
        if trace is not None:
            trace.append(ratio)
        with np.errstate(invalid="ignore"):
            high[ii] = ratio > sigma_high
        fl[ii] |= hysteresis(ratio, sigma_low, sigma_high)
    if stages is not None:
        stages["hyst"], stages["high"] = fl.copy(), high
    seed = fl & ~mask[:, None, :]
    fl |= rfi_twin.scale_invariant_rank(seed, eta=(0.1, 0.2), axis=(0, -1))
    count = fl.sum(axis=1)
    if stages is not None:
        stages["count"], stages["final"] = count, fl
    return count / fl.shape[1] > frac_samples
