"""An independent NumPy twin of the RFI flagging path (``draco_amd/util/filters.py``, ``util/rfi.py`` and the mask
tasks of ``analysis/flagging.py``): sort-based medians under the conventions of DESIGN.md section 7i, SumThreshold with
explicit index windows, a sequential SIR, and the two task iterations.  It shares no code with the library.  The
numerical cores (window sums, sorted medians, the sequential sums of SIR) are written from the algorithms' definitions;
the argument handling around them (defaults, the median and percentile taken before SumThreshold, the order of the
task's steps) necessarily says what the reference says, since that is what is being pinned.  Everything is a plain
loop: the twin is a Python brute force, meant for small planes.
"""

import numpy as np

MAD_TO_RMS = 1.4826


def _mid(v):
    """0.5 (v[(n-1)//2] + v[n//2]) of the sorted samples ``v``, NaN for none."""
    n = len(v)
    if n == 0:
        return np.nan
    return 0.5 * (v[(n - 1) // 2] + v[n // 2])


def moving_weighted_median(x, w, size):
    """Masked moving median with 0/1 weights: window centred, clipped at the edge, NaN where it holds no sample."""
    x = np.asarray(x, dtype=np.float64)
    keep = np.asarray(w) != 0
    if x.ndim == 1:
        sz = (int(size) if np.ndim(size) == 0 else int(size[0]), 1)
        return moving_weighted_median(x[:, None], keep[:, None], sz)[:, 0]
    size = (int(size),) * 2 if np.ndim(size) == 0 else tuple(int(s) for s in size)
    if any(s % 2 == 0 for s in size):
        raise ValueError(f"window sizes must be odd, got {size}")
    hf, ht = size[0] // 2, size[1] // 2
    nf, nt = x.shape
    out = np.empty((nf, nt))
    for f in range(nf):
        f0, f1 = max(f - hf, 0), min(f + hf, nf - 1) + 1
        for t in range(nt):
            t0, t1 = max(t - ht, 0), min(t + ht, nt - 1) + 1
            out[f, t] = _mid(np.sort(x[f0:f1, t0:t1][keep[f0:f1, t0:t1]]))
    return out


def quantile(y, w, q):
    """The "split" quantile of the samples with non-zero weight along the last axis."""
    y = np.asarray(y, dtype=np.float64)
    keep = np.asarray(w) != 0
    lead = y.shape[:-1]
    out = np.empty(lead)
    for ix in np.ndindex(*lead):
        v = np.sort(y[ix][keep[ix]])
        n = len(v)
        if n == 0:
            out[ix] = np.nan
            continue
        t = np.float64(q) * np.float64(n)
        lo = min(max(int(np.ceil(t)) - 1, 0), n - 1)
        hi = min(max(int(np.floor(t)), 0), n - 1)
        out[ix] = 0.5 * (v[lo] + v[hi])
    return out


def weighted_median(y, w):
    return quantile(y, w, 0.5)


def medfilt(x, mask, size):
    keep = ~np.asarray(mask, dtype=bool)
    x = np.asarray(x)
    if x.dtype.kind == "c":  # part by part
        return moving_weighted_median(x.real, keep, size) + 1j * moving_weighted_median(x.imag, keep, size)
    return moving_weighted_median(x, keep, size)


def sumthreshold(data, max_m=16, start_flag=None, threshold1=None, remove_median=True, correct_for_missing=True, variance=None, rho=None, axes=None,
                 only_positive=False, margins=None):
    """SumThreshold on a 2-D plane.  ``margins``: a list that receives the relative margin of every comparison."""
    data = np.array(data, dtype=np.float64)
    rooted = correct_for_missing or variance is not None
    correct_for_missing = rooted
    rho = {True: 0.9428, False: 1.5}[bool(rooted)] if rho is None else rho
    axes = tuple(range(data.ndim - 1, -1, -1)) if axes is None else tuple(np.atleast_1d(axes))
    flag = np.isnan(data) | np.isinf(data)
    if start_flag is not None:
        flag = flag | np.asarray(start_flag, dtype=bool)
    good = data[np.logical_not(flag)]
    if remove_median:
        centre = np.median(good)
        data = data - centre
        good = good - centre
    if threshold1 is None:
        if variance is not None:
            raise RuntimeError("a variance needs a starting threshold")
        threshold1 = np.percentile(good, 95.0)
    m = 1
    while m <= max_m:
        threshold = threshold1 / rho ** (np.log2(m))
        for axis in axes:
            d = np.moveaxis(np.where(flag, 0.0, data), axis, -1)
            with np.errstate(invalid="ignore"):
                c = (~flag).astype(np.float64) if variance is None else (~flag) * np.asarray(variance, dtype=np.float64)
            c = np.moveaxis(c, axis, -1)
            n = d.shape[-1]
            hit = np.zeros(d.shape, dtype=bool)
            for j in range(n):
                idx = np.maximum(np.arange(j - m + 1, j + 1), 0)
                ds = np.zeros(d.shape[:-1])
                cs = np.zeros(d.shape[:-1])
                for i in idx:  # ascending sample order
                    ds = ds + d[..., i]
                    cs = cs + c[..., i]
                with np.errstate(invalid="ignore"):
                    if correct_for_missing:
                        cs = np.sqrt(cs)
                    lhs = ds if only_positive else np.abs(ds)
                    rhs = cs * threshold
                    hit[..., j] = lhs > rhs
                    if margins is not None:
                        big = np.maximum(np.abs(lhs), np.abs(rhs))
                        ok = np.isfinite(lhs) & np.isfinite(rhs) & (big > 0)
                        if ok.any():
                            margins.append(float((np.abs(lhs - rhs)[ok] / big[ok]).min()))
            new = np.zeros(d.shape, dtype=bool)
            for j in range(n):  # a hit at j flags j - m + 1 ... j
                new[..., max(j - m + 1, 0) : j + 1] |= hit[..., j : j + 1]
            flag = flag | np.moveaxis(new, -1, axis)
        m *= 2
    return flag


def sir_line(flag, eta):
    """The SIR operator on one line, every sum strictly sequential."""
    n = len(flag)
    S = np.zeros(n + 1)
    s = np.float64(0.0)
    em1 = np.float64(eta) - np.float64(1.0)
    for i in range(n):
        s = s + (np.float64(1.0 if flag[i] else 0.0) + em1)
        S[i + 1] = s
    out = np.array(flag, dtype=bool)
    for i in range(n):
        before = S[: i + 1].min()
        after = S[n] if i == n - 1 else S[i + 1 : n].max()  # the reference's maximum leaves the last sum out
        out[i] |= after >= before
    return out


def sir1d(basemask, eta=0.2, axis=-1):
    b = np.moveaxis(np.asarray(basemask, dtype=bool), axis, -1)
    out = np.empty(b.shape, dtype=bool)
    for ix in np.ndindex(*b.shape[:-1]):
        out[ix] = sir_line(b[ix], eta)
    return np.moveaxis(out, -1, axis)


def scale_invariant_rank(basemask, eta=0.2, axis=-1):
    axis = tuple(np.atleast_1d(axis))
    eta = tuple(np.broadcast_to(eta, len(axis)))
    out = np.zeros(np.shape(basemask), dtype=bool)
    for ax, et in zip(axis, eta):
        out |= sir1d(basemask, et, ax)
    return out


def invert_no_zero(x):
    x = np.asarray(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0, 0, 1.0 / np.where(x == 0, 1, x)).astype(x.dtype)


def mad(x, mask, base_size=(11, 3), mad_size=(21, 21), sigma=True):
    xs = medfilt(x, mask, base_size)
    dev = np.abs(x - xs)
    m = medfilt(dev, mask, mad_size)
    if sigma:
        m = m * 1.4826
    with np.errstate(divide="ignore", invalid="ignore"):
        return dev / m


def tv_thresholds(freq, sigma, f):
    """(rows, threshold) of every TV channel the frequencies touch, in channel order."""
    import scipy.special as sp
    import scipy.stats as ss

    p_false = 2 * ss.norm.sf(sigma)
    df = np.median(np.abs(np.diff(freq)))
    out = []
    for i in range(67):
        fs = 398 + 6 * i
        rows = np.flatnonzero((freq + 0.5 * df >= fs) & (freq - 0.5 * df <= fs + 6))
        if len(rows) == 0:
            continue
        N = len(rows)
        k = int(f * N)
        out.append((rows, float(ss.norm.isf(sp.betaincinv(k + 1, N - k, 1 - (1 - p_false)) / 2))))
    return out


def tv_channels_flag(x, freq, sigma=5, f=0.5, margins=None):
    frac = np.ones(x.shape, dtype=np.float32)
    for rows, t in tv_thresholds(np.asarray(freq, dtype=np.float64), sigma, f):
        with np.errstate(invalid="ignore"):
            over = x[rows] > t
        if margins is not None:
            _margin(margins, x[rows], t)
        frac[rows] = (over.sum(axis=0).astype(np.float64) / np.float64(len(rows))).astype(np.float32)[None, :]
    if margins is not None:
        _margin(margins, frac.astype(np.float64), float(np.float32(f)))
    return frac > np.float32(f)


def _margin(margins, a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    big = np.maximum(np.abs(a), np.abs(b))
    ok = np.isfinite(a) & np.isfinite(b) & (big > 0)
    if ok.any():
        margins.append(float((np.abs(a - b)[ok] / big[ok]).min()))


def mask_1d(rad, mask, quantile_1d=0.15, win_f_1d=191, nsigma_1d=5.0, margins=None):
    y = np.asarray(rad, dtype=np.float64)
    w = ~np.asarray(mask, dtype=bool)
    medt = quantile(y, w, quantile_1d)
    wt = w.any(axis=-1)
    if win_f_1d is None:
        base = weighted_median(medt, wt)
    else:
        base = moving_weighted_median(medt, wt, win_f_1d)
    absd = np.abs(medt - base)
    if win_f_1d is None:
        m1 = MAD_TO_RMS * weighted_median(absd, wt)
    else:
        m1 = MAD_TO_RMS * moving_weighted_median(absd, wt, win_f_1d)
    if margins is not None:
        _margin(margins, absd, nsigma_1d * m1)
    with np.errstate(invalid="ignore"):
        return absd > nsigma_1d * m1, medt


def sensitivity_mask(measured, radiometer, weight, freq, mask_type="combine", include=None, static=None, madtimes=None, nsigma_1d=5.0, quantile_1d=0.15,
                     win_f_1d=191, nsigma=5.0, niter=5, rho=1.5, base_size=(37, 181), mad_size=(101, 31), tv_fraction=0.5, max_m=64, sir=False, eta=0.2,
                     only_time=False, margins=None):
    """The iteration of RFISensitivityMask on ``[freq, pol, time]`` float32 inputs; ``include``: which pols to process,
    ``static``: frequencies the static mask removes, ``madtimes``: the mixing array of "combine"."""
    measured = np.asarray(measured, dtype=np.float32)
    radiometer = np.asarray(radiometer, dtype=np.float32)
    rad = measured * invert_no_zero(radiometer)  # float32
    flag = np.asarray(weight) == 0.0
    nf, npol, nt = rad.shape
    static = np.zeros(nf, dtype=bool) if static is None else np.asarray(static, dtype=bool)
    if madtimes is None:
        madtimes = np.ones((nf, nt), dtype=bool)
    thresholds = nsigma * rho ** np.arange(niter)[::-1]
    final = np.zeros((npol, nf, nt), dtype=bool)
    for p in range(npol):
        if include is not None and not include[p]:
            continue
        y = rad[:, p, :].astype(np.float64)
        cur = flag[:, p, :] | static[:, None]
        if nsigma_1d is not None:
            f1, ystat = mask_1d(y, cur, quantile_1d, win_f_1d, nsigma_1d, margins)
            cur = cur | f1[:, None]
            y = y - ystat[:, None]
        for ns in thresholds:
            med = medfilt(y, cur, base_size)
            dy = y - med
            ady = np.abs(dy)
            med_ady = MAD_TO_RMS * medfilt(ady, cur, mad_size)
            ratio = ady * invert_no_zero(med_ady)
            if margins is not None:
                _margin(margins, ratio, ns)
            with np.errstate(invalid="ignore"):
                madmask = ratio > ns
            tv = tv_channels_flag(ratio, freq, sigma=ns, f=tv_fraction, margins=margins)
            madmask = madmask | tv
            if mask_type == "mad":
                cur = cur | madmask
                continue
            st = sumthreshold(dy, max_m, start_flag=cur | tv, threshold1=ns, remove_median=False, correct_for_missing=True, rho=1.0, variance=med_ady**2,
                              margins=margins)
            if mask_type == "sumthreshold":
                cur = cur | st
            else:
                temp = np.where(madtimes, madmask, st)
                if not sir:
                    temp = np.where(madtimes, scale_invariant_rank(temp, eta=0.2, axis=-1), temp)
                cur = cur | temp
        final[p] = cur
    out = final.any(axis=0)
    if sir:
        nobase = out.copy()
        nobase[static] = False
        out = scale_invariant_rank(nobase, eta=eta, axis=(-1,) if only_time else (0, -1)) | out
    return out


def rfi_mask(vis, weight, freq, sigma=5.0, tv_fraction=0.5, margins=None):
    """The mask of RFIMask from one stack's ``vis [freq, time]`` and ``weight``."""
    weight = np.asarray(weight)
    wm = weight < 1e-4 * weight.mean()
    dev = mad(vis, wm)
    dev = np.where(np.isnan(dev), 2 * sigma, dev)
    if margins is not None:
        _margin(margins, dev, sigma)
    return tv_channels_flag(dev, freq, sigma=sigma, f=tv_fraction, margins=margins) | (dev > sigma)
