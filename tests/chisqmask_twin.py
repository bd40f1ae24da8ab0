"""An independent NumPy twin of the chi-squared mask path: the weighted moving median of DESIGN.md section 7s (sort
based, weight sums in long double), the three reductions of ``dmm_axis_reduce`` in long double, and the steps of
``RFIMaskChisqHighDelay``.  It shares no code with the library.  The
numerical cores are written from the definitions; the order of the task's steps says what the reference says, since
that is what is being pinned.  A brute force, meant for small planes.
"""

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
MAD_TO_RMS = 1.48625


def weighted_median_1(v, w, detail=False):
    """0.5 (lo + hi) of the samples ``v`` with weight ``w > 0``: with ``W`` the total weight and ``c(x)`` the weight of
    the samples ``<= x``, ``lo`` is the smallest sample with ``c >= W/2`` and ``hi`` the smallest with ``c > W/2``.  NaN
    for no sample.  ``detail``: also whether the split was exact (``c(lo) == W/2``) and whether ``lo != hi``."""
    v = np.asarray(v, dtype=np.float64).ravel()
    w = np.asarray(w).ravel()
    keep = w > 0
    v, w = v[keep], w[keep].astype(LD)
    if v.size == 0:
        return (np.nan, False, False) if detail else np.nan
    order = np.argsort(v, kind="stable")  # NaN samples sort last
    v, w = v[order], w[order]
    c = np.cumsum(w)
    half = c[-1] / LD(2)
    same = (v[1:] == v[:-1]) | (np.isnan(v[1:]) & np.isnan(v[:-1]))
    ends = np.flatnonzero(np.append(~same, True))  # the last sample of every run of equal values
    ce, ve = c[ends], v[ends]
    i = int(np.argmax(ce >= half))
    j = int(np.argmax(ce > half))
    with np.errstate(invalid="ignore"):
        out = 0.5 * (ve[i] + ve[j])
    return (out, bool(ce[i] == half), i != j) if detail else out


def moving_weighted_median(x, w, size, detail=None):
    """The weighted moving median: window centred on the sample, ``size // 2`` to each side, clipped at the edge.
    ``detail``: a dict that receives the Boolean planes ``exact`` (the window split exactly between two different
    samples) and ``empty``."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w)
    if x.ndim == 1:
        sz = int(size) if np.ndim(size) == 0 else int(size[0])
        return moving_weighted_median(x[:, None], w[:, None], (sz, 1), detail)[:, 0]
    size = (int(size),) * 2 if np.ndim(size) == 0 else tuple(int(s) for s in size)
    if any(s < 1 or s % 2 == 0 for s in size):
        raise ValueError(f"window sizes must be odd and positive, got {size}")
    hf, ht = size[0] // 2, size[1] // 2
    nf, nt = x.shape
    out = np.empty((nf, nt))
    exact = np.zeros((nf, nt), dtype=bool)
    empty = np.zeros((nf, nt), dtype=bool)
    for f in range(nf):
        f0, f1 = max(f - hf, 0), min(f + hf, nf - 1) + 1
        for t in range(nt):
            t0, t1 = max(t - ht, 0), min(t + ht, nt - 1) + 1
            out[f, t], ex, two = weighted_median_1(x[f0:f1, t0:t1], w[f0:f1, t0:t1], detail=True)
            exact[f, t] = ex and two
            empty[f, t] = not (w[f0:f1, t0:t1] > 0).any()
    if detail is not None:
        detail["exact"], detail["empty"] = exact, empty
    return out


def weighted_median(y, w):
    """The weighted median along the last axis; an empty row gives 0.0 (the convention of the mask task)."""
    y = np.asarray(y, dtype=np.float64)
    w = np.asarray(w)
    out = np.empty(y.shape[:-1])
    for ix in np.ndindex(*y.shape[:-1]):
        m = weighted_median_1(y[ix], w[ix])
        out[ix] = 0.0 if not (w[ix] > 0).any() else m
    return out


def inz(v):
    v = np.asarray(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(v == 0, 0, 1 / np.where(v == 0, 1, v))


def _ld(x):
    x = np.asarray(x)
    return x.astype(CLD if x.dtype.kind == "c" else LD)


def reduce_chisq(x, w, axis):
    """``(v, num)`` in long double, the reduced axes kept with length one."""
    x, w = _ld(x), np.broadcast_to(np.asarray(w), np.shape(x)).astype(LD)
    num = np.maximum((w > 0).sum(axis=axis, keepdims=True) - 1, 0)
    mu = (w * x).sum(axis=axis, keepdims=True) * inz(w.sum(axis=axis, keepdims=True))
    v = (w * np.abs(x - mu) ** 2).sum(axis=axis, keepdims=True) * inz(num.astype(LD))
    return v, num


def reduce_var(x, w, axis, weighting):
    """``(v, ws)`` in long double for the weightings "none", "masked" and "weighted"."""
    x = _ld(x)
    if weighting == "none":
        mu = x.mean(axis=axis, keepdims=True)
        v = (np.abs(x - mu) ** 2).mean(axis=axis, keepdims=True)
        return v, np.ones(v.shape)
    w = np.broadcast_to(np.asarray(w), x.shape).astype(LD)
    if weighting == "masked":
        w = (w > 0).astype(LD)
    ws = w.sum(axis=axis, keepdims=True)
    mu = (w * x).sum(axis=axis, keepdims=True) * inz(ws)
    return (w * (x - mu) ** 2).sum(axis=axis, keepdims=True) * inz(ws), ws


def reduce_wmean(x, w, axis, factor=1.0):
    """``(y, s)``: ``s = factor sum w``, ``y = sum(w Re x) / s`` (0 where ``s`` is 0), in long double, the reduced
    axes dropped."""
    xr = np.asarray(x).real.astype(LD)
    w = np.broadcast_to(np.asarray(w), xr.shape).astype(LD)
    s = LD(factor) * w.sum(axis=axis)
    return (w * xr).sum(axis=axis) * inz(s), s


def arpls(y, mask, lam, epsilon=1e-2, max_iter=100):
    """Asymmetrically reweighted penalised least squares with a dense solve (Baek et al. 2015)."""
    y = np.asarray(y, dtype=np.float64)
    mask = np.asarray(mask, dtype=bool)
    n = len(y)
    if mask.all():
        return np.zeros(n)
    D = np.zeros((n, max(n - 2, 0)))
    for j in range(max(n - 2, 0)):
        D[j : j + 3, j] = (1.0, -2.0, 1.0)
    H = lam * (D @ D.T)
    w = np.where(mask, 0.0, 1.0)
    big = np.log(np.finfo(np.float64).max)
    z = np.zeros(n)
    for _ in range(max_iter):
        z = np.linalg.solve(H + np.diag(w), w * y)
        d = y - z
        neg = (d < 0) & ~mask
        mu, sigma = d[neg].mean(), d[neg].std()
        arg = np.clip(2 * (d - (2 * sigma - mu)) * (0.0 if sigma == 0 else 1.0 / sigma), -big, big)
        wn = 1.0 / (np.exp(arg) + 1.0)
        if np.linalg.norm(w - wn) / np.linalg.norm(w) < epsilon:
            break
        w = np.where(mask, 0.0, wn)
    return z


def _note(trace, lhs, rhs):
    """Record the two sides of a threshold comparison (``trace``: a list, or None)."""
    if trace is not None:
        a, b = np.broadcast_arrays(np.asarray(lhs, dtype=np.float64), np.asarray(rhs, dtype=np.float64))
        trace.append((a.copy(), b.copy()))


def trace_margin(trace):
    """The smallest relative margin ``|lhs - rhs| / max(|lhs|, |rhs|)`` over the comparisons of a trace whose sides
    are finite and not both zero (the others come out the same under any rounding)."""
    best = np.inf
    for a, b in trace:
        big = np.maximum(np.abs(a), np.abs(b))
        ok = np.isfinite(a) & np.isfinite(b) & (big > 0)
        if ok.any():
            best = min(best, float((np.abs(a - b)[ok] / big[ok]).min()))
    return best


def sumthreshold(dy, max_m, start_flag, threshold1, variance, only_positive=False, trace=None):
    """SumThreshold as the mask task calls it: no median removed, thresholds constant over the window lengths (rho =
    1), the summed variance under the root, time axis first.  Explicit index windows; the windows that reach below
    sample 0 repeat sample 0, as the reference's convolution does."""
    data = np.asarray(dy, dtype=np.float64)
    flag = ~np.isfinite(data) | np.asarray(start_flag, dtype=bool)
    m = 1
    while m <= max_m:
        for axis in (1, 0):
            d = np.moveaxis(np.where(flag, 0.0, data), axis, -1)
            with np.errstate(invalid="ignore"):
                c = np.moveaxis((~flag) * np.asarray(variance, dtype=np.float64), axis, -1)
            n = d.shape[-1]
            ds, cs = np.zeros(d.shape), np.zeros(d.shape)
            for j in range(n):
                for i in range(j - m + 1, j + 1):  # ascending sample order
                    ds[..., j] = ds[..., j] + d[..., max(i, 0)]
                    cs[..., j] = cs[..., j] + c[..., max(i, 0)]
            with np.errstate(invalid="ignore"):
                lhs = ds if only_positive else np.abs(ds)
                rhs = np.sqrt(cs) * threshold1
                hit = lhs > rhs
            _note(trace, lhs, rhs)
            new = np.zeros(d.shape, dtype=bool)
            for j in range(n):  # a hit at j flags j - m + 1 ... j
                new[..., max(j - m + 1, 0) : j + 1] |= hit[..., j : j + 1]
            flag = flag | np.moveaxis(new, -1, axis)
        m *= 2
    return flag


def mask_1d(y, m, reg_arpls=1e5, nsigma_1d=5.0, trace=None, baseline=None):
    y = np.asarray(y, dtype=np.float64)
    m = np.asarray(m, dtype=bool)
    med_y = weighted_median(y, (~m).astype(np.float64))
    med_m = m.all(axis=-1)
    base = arpls(med_y, med_m, reg_arpls) if baseline is None else baseline(med_y, med_m)
    abs_dev = np.where(med_m, 0.0, np.abs(med_y - base))
    mad = MAD_TO_RMS * weighted_median(abs_dev, (~med_m).astype(np.float64))
    _note(trace, abs_dev, nsigma_1d * mad)
    return abs_dev > nsigma_1d * mad


def mask_2d(y, w, win=(1, 601), nsigma_2d=5.0, estimate_var=False, only_positive=False, trace=None, detail=None):
    y = np.asarray(y, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        dy = (y - moving_weighted_median(y, w, win, detail)) * np.sqrt(w)
        if estimate_var:
            mad_y = MAD_TO_RMS * moving_weighted_median(np.abs(dy), (w > 0).astype(np.float64), win)
            dy = dy * inz(mad_y)
        if not only_positive:
            dy = np.abs(dy)
        _note(trace, dy, nsigma_2d)
        return dy > nsigma_2d


def mask_2d_sumthreshold(y, w, win=(1, 601), nsigma_2d=5.0, niter=5, rho=1.5, max_m=32, estimate_var=False, only_positive=False, trace=None, detail=None):
    y = np.asarray(y, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    mad_y = np.ones_like(y)
    mask = w == 0.0
    for nsigma in nsigma_2d * rho ** np.arange(niter)[::-1]:
        f = (~mask) * w
        with np.errstate(invalid="ignore"):
            dy = (y - moving_weighted_median(y, f, win, detail)) * np.sqrt(w)
            if estimate_var:
                mad_y = MAD_TO_RMS * moving_weighted_median(np.abs(dy), (f > 0).astype(np.float64), win)
        mask = mask | sumthreshold(dy, max_m, mask, nsigma, mad_y**2, only_positive, trace)
        detail = None  # the fixtures are counted on the first pass
    return mask


def chisq_mask(chisq, wsum, mask_sources=None, mask_daytime=None, mask_type="mad", nsigma_1d=5.0, reg_arpls=1e5, win=(1, 601), nsigma_2d=5.0, estimate_var=False,
               only_positive=False, niter=5, rho=1.5, max_m=32, trace=None, detail=None, baseline=None):
    """The mask of one ``[freq, time]`` plane from the collapsed statistic and its summed weight."""
    chisq = np.asarray(chisq, dtype=np.float64)
    wsum = np.asarray(wsum, dtype=np.float64)
    nf, nt = chisq.shape
    day = np.zeros(nt, dtype=bool) if mask_daytime is None else np.asarray(mask_daytime, dtype=bool)
    mask = (wsum == 0.0) | (np.zeros((nf, nt), dtype=bool) if mask_sources is None else np.asarray(mask_sources, dtype=bool))
    out = np.zeros((nf, nt), dtype=bool)
    if nsigma_1d > 0.0:
        rows = mask_1d(chisq, mask | day, reg_arpls, nsigma_1d, trace, baseline)[:, None]
        mask = mask | rows
        out |= rows
    if nsigma_2d > 0.0:
        w = ~mask * wsum / 2.0
        if mask_type == "mad":
            m2 = mask_2d(chisq, w, win, nsigma_2d, estimate_var, only_positive, trace, detail)
        else:
            m2 = mask_2d_sumthreshold(chisq, w, win, nsigma_2d, niter, rho, max_m, estimate_var, only_positive, trace, detail)
        out |= m2 & ~day
    return out
