"""Plain NumPy restatement of ``DayenuDelayFilterHybridVis.process`` (``draco/analysis/dayenu.py:463-572``) and
``RADependentWeights.process`` (``draco/analysis/ringmapmaker.py:1227-1315``).

Two forms, as in ``dayenu_twin.py``:

* the **f64 form** does what the reference does, dtype by dtype (``numpy.linalg.pinv``, float32 variances, the float32
  time average of the inverse-variance scheme);
* the **truth form** builds every filter by ``dayenu_twin.filter_truth`` (long-double covariance and Cholesky inverse)
  and carries every product and sum in long double.  ``inz`` of the float32 weights is taken in float32 in both forms,
  as the reference's ``invert_no_zero`` on the dataset does; the caller rounds the truth to each dataset's dtype.

Datasets: ``vis [pol, freq, ew, el, ra]`` c64, ``weight [pol, freq, ew, ra]`` f32, ``filter`` / ``freq_cov [pol, freq,
freq_sum, ew, ra]`` f64; ring map ``weight [pol, freq, ra, el]``, ``filter`` / ``freq_cov [pol, freq, freq_sum, ra]``
f64.
"""

import numpy as np

import dayenu_twin as dt

LD = np.longdouble
rel_err = dt.rel_err


def inz(x):
    """``invert_no_zero``: in the dtype of a floating-point ``x``, in float64 for integers."""
    x = np.asarray(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0, 0, 1 / np.where(x == 0, 1, x)).astype(x.dtype if x.dtype.kind in "fc" else np.float64)


def sample_mask(weight):
    """``flag [freq, ew, ra]``: the channels whose weight is positive in every polarisation."""
    return np.all(weight > 0.0, axis=0)


def filter_hybrid(freq, vis, weight, tauw=0.4, epsilon=1e-12, atten_threshold=0.0, apply_filter=True, save_filter=False, calculate_cov=False, truth=False):
    """``(vis, weight, filter, freq_cov)`` (the last two ``None`` unless asked for).  f64 form: arrays of the
    containers' dtypes, assigned as the reference does.  Truth form: long double, not rounded."""
    npol, nfreq, new, nel, ntime = vis.shape
    flag = sample_mask(weight)
    if truth:
        ovis, oweight = vis.astype(np.clongdouble), weight.astype(LD)
    else:
        ovis, oweight = vis.copy(), weight.copy()
    ft = LD if truth else np.float64
    filt = np.zeros((npol, nfreq, nfreq, new, ntime), dtype=ft) if save_filter else None
    cov = np.zeros((npol, nfreq, nfreq, new, ntime), dtype=ft) if calculate_cov else None
    cache = {}
    for tt in range(ntime):
        for xx in range(new):
            flagx = flag[:, xx, tt]
            if not np.any(flagx):
                continue
            key = flagx.tobytes()
            if key not in cache:
                cache[key] = dt.filter_truth(freq, flagx, tauw, epsilon) if truth else dt.delay_filter_f64(freq, flagx[:, np.newaxis], tauw, epsilon)[0][0]
            nf = cache[key]
            for pp in range(npol):
                if save_filter:
                    filt[pp, :, :, xx, tt] = nf
                tvar = inz(weight[pp, :, xx, tt])  # (float32)
                if not apply_filter:  # (the reference skips the rest, the covariance included)
                    continue
                if truth:
                    tv = vis[pp, :, xx, :, tt]
                    ovis[pp, :, xx, :, tt] = nf @ tv.real.astype(LD) + 1j * (nf @ tv.imag.astype(LD))
                    w = inz(np.matmul(nf * nf, tvar.astype(LD)))
                else:
                    ovis[pp, :, xx, :, tt] = np.matmul(nf, np.ascontiguousarray(vis[pp, :, xx, :, tt]))
                    w = inz(np.matmul(np.abs(nf) ** 2, tvar))
                if calculate_cov:
                    cov[pp, :, :, xx, tt] = np.matmul(nf * tvar.astype(ft) if truth else nf * tvar, nf.T)
                if atten_threshold > 0.0:
                    diag = np.abs(np.diag(nf))
                    w = w * (diag > (atten_threshold * np.median(diag[diag > 0.0]))).astype(w.dtype)
                oweight[pp, :, xx, tt] = w
    return ovis, oweight, filt, cov


def ew_weights(var_time_avg, scheme, exclude_cyl, new, truth=False):
    """``weight_ew`` broadcastable against ``var [pol, freq, ew, ra]`` (``ringmapmaker.py:1267-1284``)."""
    if scheme == "inverse_variance":
        w = inz(var_time_avg)
    else:
        w = np.ones(new) if scheme == "uniform" else new - np.arange(new)
        w = w[np.newaxis, np.newaxis, :, np.newaxis]
        if truth:
            w = w.astype(LD)
    w = np.array(w)
    for cyl in exclude_cyl:
        w[..., cyl, :] = 0.0
    return w


def ra_dependent_weights(hweight, rweight, scheme, exclude_cyl, filt=None, cov=None, truth=False):
    """``(ringmap weight, filter, freq_cov)``; ``filter`` / ``freq_cov`` are ``None`` where the hybrid stream has none
    (and ``freq_cov`` for ``inverse_variance``).  Truth form: long double, not rounded."""
    var = inz(hweight)  # (float32)
    new = var.shape[-2]
    if truth:
        var = var.astype(LD)
    var_time_avg = np.mean(var, axis=-1, keepdims=True)
    w = ew_weights(var_time_avg, scheme, exclude_cyl, new, truth)
    ra_dep = np.sum(w**2 * var_time_avg, axis=-2) * inz(np.sum(w**2 * var, axis=-2))
    oweight = (rweight.astype(LD) if truth else rweight.copy()) * ra_dep[..., np.newaxis]
    ofilt = ocov = None
    if filt is not None:
        sum_w = np.sum(w, axis=-2, keepdims=True)
        wew = (w * inz(sum_w))[:, :, np.newaxis]
        ofilt = np.sum(wew * (filt.astype(LD) if truth else filt), axis=-2)
    if cov is not None and scheme != "inverse_variance":
        ws = np.squeeze(w)
        wew2 = ws[:, np.newaxis] ** 2 * inz(np.sum(ws) ** 2)
        ocov = np.sum(wew2 * (cov.astype(LD) if truth else cov), axis=-2)
    return oweight, ofilt, ocov


# ---- the cases of tests/golden/dayenu_hybrid.npz (tests/gen_golden_dayenu_hybrid.py)
HYBRID_CASES = ("H33", "H70", "H6", "H20")
SCHEMES = ("natural", "uniform", "inverse_variance")
R_CASES = tuple(f"R_{s}_{x}" for s in SCHEMES for x in ("none", "1"))


def case(g, name):
    """Inputs and configuration of a hybrid case: ``vis`` complex64 from the stored multiples of 1/8."""
    q = g[f"{name}/vis_q"]
    atten, apply_filter, save_filter, calculate_cov = (float(x) for x in g[f"{name}/cfg"])
    tauw, eps = g[f"{name}/tauw"], g[f"{name}/epsilon"]
    cfg = dict(tauw=tauw if tauw.size > 1 else float(tauw[0]), epsilon=eps if eps.size > 1 else float(eps[0]), atten_threshold=atten,
               apply_filter=bool(apply_filter), save_filter=bool(save_filter), calculate_cov=bool(calculate_cov))
    return dict(freq=g[f"{name}/freq"], vis=((q[..., 0] + 1j * q[..., 1]) / 8.0).astype(np.complex64), weight=g[f"{name}/weight"], cfg=cfg, pos=g[f"{name}/pos"])


def truth_of(c):
    """The truth of a hybrid case, rounded to the datasets' dtypes (``None`` for the datasets it does not keep)."""
    tv, tw, tf, tc = filter_hybrid(c["freq"], c["vis"], c["weight"], truth=True, **c["cfg"])
    f64 = lambda a: None if a is None else a.astype(np.float64)  # noqa: E731
    return dict(vis=tv.astype(np.complex64), weight=tw.astype(np.float32), filter=f64(tf), freq_cov=f64(tc))


def r_case(name):
    """``(scheme, exclude_cyl)`` of an R case name."""
    scheme, excl = name[2:].rsplit("_", 1)
    return scheme, ([] if excl == "none" else [int(x) for x in excl.split("x")])


def at_positions(name, arr, pos):
    """The stored sample of a hybrid dataset: ``vis [npos, pol, freq, el]``, ``filter [freq, freq_sum, npos]`` (pol 0),
    ``freq_cov [pol, freq, freq_sum, npos]``."""
    px, pt = pos[:, 0], pos[:, 1]
    if name == "vis":
        return arr[:, :, px, :, pt]
    if name == "filter":
        return arr[0][:, :, px, pt]
    return arr[:, :, :, px, pt]
