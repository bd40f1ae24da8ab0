"""Plain NumPy restatement of the stored-filter apply (``draco/analysis/dayenu.py:575-739``) and of the HyFoReS bandpass
estimate and clean (``draco/analysis/hyforesbandpass.py``), in the arithmetic of ``csrc/hyfores.hip``.

Two forms:

* the **f64 form** mirrors the device: the difference ``vis - post`` and every sum in float64 from the complex64
  inputs, ``inz`` of the float32 weight in float32, ``vis`` rounded to complex64 and ``vis_weight`` to float32 at the end;
* the **truth form** (``truth=True``) carries every product and sum in ``numpy.longdouble`` and does not round; for the
  sums of the estimate it also returns ``allow``, an absolute bound of what float64 summation *in any order* can be off
  by: ``(n + 4) u S_abs`` for a sum of ``n`` complex products, ``u = 2**-53``, ``S_abs`` the sum of the moduli of the
  terms (long double), carried through the division as ``allow_y = allow_yN inz(D) + |y| (n + 6) u``.

Datasets: ``vis`` / ``post [pol, freq, ew, el, ra]`` c64, ``weight [pol, freq, ew, ra]`` f32, ``filt`` / ``freq_cov
[pol, freq, freq_sum, ew, ra]`` f64, pixel masks ``[pol, freq, ra, el]`` bool (a ring map's axes).
"""

import numpy as np
import scipy.linalg as la

LD = np.longdouble
CLD = np.clongdouble
U = 2.0**-53
C_LIGHT = 299792458.0
OK, SKIPPED, ZERO_FILTER, MISSING_FREQ = 0, 1, 2, 3


def inz(x):
    """``invert_no_zero`` in the dtype of ``x``."""
    x = np.asarray(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0, 0, 1 / np.where(x == 0, 1, x)).astype(x.dtype)


def rel_err(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def sample_status(weight, filt):
    """``status [pol, ew, ra]`` of the reference's three early exits (``dayenu.py:671-700``), flags per polarisation."""
    flag = weight > 0.0  # [p, k, x, t]
    colnz = (filt != 0.0).any(axis=1)  # [p, k, x, t]
    st = np.full(flag.shape[:1] + flag.shape[2:], OK, dtype=np.uint8)
    st[(colnz & ~flag).any(axis=1)] = MISSING_FREQ
    st[~colnz.any(axis=1)] = ZERO_FILTER
    st[~flag.any(axis=1)] = SKIPPED
    return st


def atten_flags(filt, atten_threshold):
    """``[pol, freq, ew, ra]`` bool: ``|F[f, f]| > atten_threshold x median(non-zero |F[f, f]|)`` (all True for a sample
    whose diagonal is zero)."""
    npol, nfreq, _, new, nra = filt.shape
    out = np.ones((npol, nfreq, new, nra), dtype=bool)
    for p in range(npol):
        for x in range(new):
            for t in range(nra):
                diag = np.abs(np.diag(filt[p, :, :, x, t]))
                if np.any(diag > 0.0):
                    out[p, :, x, t] = diag > (atten_threshold * np.median(diag[diag > 0.0]))
    return out


def apply_filter(vis, weight, filt, gain=None, atten_threshold=0.0, atten_vis=False, keep_input=True, calculate_cov=False, truth=False):
    """``(vis, weight, freq_cov, status)`` of the stored-filter apply; ``gain [pol, ew, freq]`` complex128 takes
    ``d = 1 - gain`` out of the data first.  f64 form: complex64 / float32 / float64; truth form: long double."""
    ft, ct = (LD, CLD) if truth else (np.float64, np.complex128)
    st = sample_status(weight, filt)
    ok = st == OK
    fl = filt.astype(ft)
    v = vis.astype(ct)
    var = inz(weight).astype(ft)  # (inz in float32)
    if gain is not None:
        d = (1 - np.asarray(gain).astype(ct)).transpose(0, 2, 1)  # [p, k, x]
        v = v * d[:, :, :, None, None]
        var = var * (d.real**2 + d.imag**2)[:, :, :, None]
    out = np.einsum("pfkxt,pkxlt->pfxlt", fl, v.real) + 1j * np.einsum("pfkxt,pkxlt->pfxlt", fl, v.imag)
    w = inz(np.einsum("pfkxt,pkxt->pfxt", fl * fl, var))
    at = atten_flags(filt, atten_threshold) if atten_threshold > 0.0 else None
    if at is not None:
        w = w * at
        if atten_vis:
            out = out * at[:, :, :, None, :]
    okv, okw = ok[:, None, :, None, :], ok[:, None, :, :]
    out = np.where(okv, out, vis.astype(ct) if keep_input else 0)
    w = np.where(okw, w, np.where((st == SKIPPED)[:, None], weight.astype(ft), 0))
    cov = None
    if calculate_cov:
        cov = np.einsum("pfkxt,pgkxt,pkxt->pfgxt", fl, fl, var) * ok[:, None, None]
    if not truth:
        out, w = out.astype(np.complex64), w.astype(np.float32)
    return out, w, cov, st


def el_mask(el, freq, min_ysep):
    return np.abs(el) < (C_LIGHT / (np.max(freq) * 1e6 * min_ysep) - 1.0)


def pixel_mask(mask, masks=None):
    """``[pol, freq, el, ra]`` from ring-map masks ``[pol, freq, ra, el]``; with ``masks``: ``mask & ~masks``."""
    m = np.asarray(mask, dtype=bool)
    if masks is not None:
        m = m & ~np.asarray(masks, dtype=bool)
    return np.swapaxes(m, -1, -2)


def estimate(vis, post, weight, filt, elm, pix=None, truth=False):
    """``dict(yN, D, N, y, W)``, ``[pol, ew, freq(, freq)]``, from complex64 ``vis`` and ``post``; the truth form adds
    ``allow_yN`` ... ``allow_W``."""
    ft, ct = (LD, CLD) if truth else (np.float64, np.complex128)
    npol, nfreq, new, nel, nra = vis.shape
    m = (weight > 0.0)[:, :, :, None, :] & np.asarray(elm, dtype=bool)[None, None, None, :, None]
    if pix is not None:
        m = m & ~np.asarray(pix, dtype=bool)[:, :, None, :, :]
    g = (vis.astype(ct) - post.astype(ct)) * m
    s = post.astype(ct) * m
    fl = filt.astype(ft)
    yn = np.einsum("pfxlt,pfxlt->pxf", np.conj(g), s)
    d = np.einsum("pfxlt->pxf", g.real**2 + g.imag**2)
    gram = np.einsum("pfxlt,pgxlt->pfgxt", np.conj(g), g)
    n = np.einsum("pfgxt,pfgxt->pxfg", fl, gram.real) + 1j * np.einsum("pfgxt,pfgxt->pxfg", fl, gram.imag)
    out = dict(yN=yn, D=d, N=n, y=yn * inz(d), W=n * inz(d)[..., None])
    if truth:
        cnt = nel * nra
        ag, as_ = np.abs(g), np.abs(s)
        out["allow_yN"] = (cnt + 4) * U * np.einsum("pfxlt,pfxlt->pxf", ag, as_)
        out["allow_D"] = (cnt + 4) * U * d
        out["allow_N"] = (cnt + 4) * U * np.einsum("pfgxt,pfgxt->pxfg", np.abs(fl), np.einsum("pfxlt,pgxlt->pfgxt", ag, ag))
        out["allow_y"] = out["allow_yN"] * inz(d) + np.abs(out["y"]) * (cnt + 6) * U
        out["allow_W"] = out["allow_N"] * inz(d)[..., None] + np.abs(out["W"]) * (cnt + 6) * U
    return out


def filtered_for_estimate(vis, weight, filt, atten_threshold=0.0, truth=False):
    """``(post complex64, weight float32)`` as the ``DelayFilter...`` estimators form them: the filtered visibilities
    **rounded to complex64** (zero where a sample is not filtered, and under the attenuation flag) and the copy of the
    weight, zeroed where a sample is not filtered and under the attenuation flag."""
    post, _, _, st = apply_filter(vis, weight, filt, atten_threshold=atten_threshold, atten_vis=True, keep_input=False, truth=truth)
    w = weight * (st == OK)[:, None]
    if atten_threshold > 0.0:
        w = w * atten_flags(filt, atten_threshold)
    return post.astype(np.complex64), w.astype(np.float32)


KINDS = ("DelayFilterHyFoReSBandpassHybridVis", "DelayFilterHyFoReSBandpassHybridVisMask", "HyFoReSBandpassHybridVis", "HyFoReSBandpassHybridVisMask",
         "HyFoReSBandpassHybridVisMaskKeepSource")


def estimator(kind, c, truth=False, post=None):
    """The estimate of task ``kind`` on the inputs of case ``c`` (:func:`case`).  ``post``: use these complex64
    filtered visibilities in place of the twin's own for the ``DelayFilter...`` kinds."""
    elm = el_mask(c["el"], c["freq"], c["min_ysep"])
    pix = None
    if "Mask" in kind:
        pix = pixel_mask(c["mask"], c["masks"] if kind.endswith("KeepSource") else None)
    if kind.startswith("DelayFilter"):
        p, w = filtered_for_estimate(c["vis"], c["weight"], c["filter"], c["atten_threshold"], truth=truth)
        if post is not None:
            p = post
        return estimate(c["vis"], p, w, c["filter"], elm, pix, truth=truth)
    return estimate(c["vis"], c["pf_vis"], c["pf_weight"], c["filter"], elm, pix, truth=truth)


def compensate_window(W, y, cutoff):
    """``(g, sval, rank)`` as ``hyforesbandpass.py:1177-1199``."""
    npol, new, nfreq = y.shape
    sval, rank = np.zeros((npol, new, nfreq)), np.zeros((npol, new))
    if cutoff == 0.0:
        return y, sval, rank
    g = np.zeros_like(y)
    for p in range(npol):
        for x in range(new):
            sval[p, x] = la.svd(W[p, x], compute_uv=False)
            wp, rank[p, x] = la.pinv(W[p, x], atol=cutoff, return_rank=True)
            g[p, x] = np.dot(wp, y[p, x])
    return g, sval, rank


# ---- the cases of tests/golden/hyfores.npz (tests/gen_golden_hyfores.py)
CASES = ("Y33", "Y70", "Y6")


def expand_filter(mats, index):
    """``filter [pol, freq, freq, ew, ra]`` from one matrix per distinct mask ``mats [nmat, freq, freq]`` and ``index
    [pol, ew, ra]`` (negative: a zero filter)."""
    nmat, nfreq, _ = mats.shape
    full = np.concatenate([mats, np.zeros((1, nfreq, nfreq))], axis=0)[np.where(index < 0, nmat, index)]  # [p, x, t, f, k]
    return np.ascontiguousarray(full.transpose(0, 3, 4, 1, 2))


def case(g, name):
    """The inputs of a case: ``vis`` / ``pf_vis`` complex64 from the stored multiples of 1/8."""
    k = lambda s: g[f"{name}/{s}"]  # noqa: E731
    q = k("vis_q")
    c = dict(freq=k("freq"), el=k("el"), min_ysep=float(k("min_ysep")), atten_threshold=float(k("atten_threshold")),
             vis=((q[..., 0] + 1j * q[..., 1]) / 8.0).astype(np.complex64), weight=k("weight"), filter=expand_filter(k("filter_mats"), k("filter_index")), pos=k("pos"))
    if f"{name}/pf_vis_q" in g:
        pq = k("pf_vis_q").astype(np.float64)
        c["pf_vis"], c["pf_weight"] = ((pq[..., 0] + 1j * pq[..., 1]) / 8.0).astype(np.complex64), k("pf_weight")
    if f"{name}/mask" in g:
        c["mask"], c["masks"] = k("mask"), k("masks")
    if f"{name}/src_weight" in g:
        c["src_weight"] = k("src_weight")
    return c


def at_positions(name, arr, pos):
    """The stored sample of a dataset: ``vis [npos, pol, freq, el]``, ``freq_cov [pol, freq, freq_sum, npos]``."""
    px, pt = pos[:, 0], pos[:, 1]
    if name == "vis":
        return arr[:, :, px, :, pt]
    return arr[:, :, :, px, pt]
