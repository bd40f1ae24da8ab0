"""Long-double twins of the rebinner, its gradient correction and the direct interpolators (dense restatements, CPU
only): exact products, no float32 intermediates except the two that are part of the contract -- the variance
``invert_no_zero(weight)`` of the interpolators and of the rebinner's uniform mode, which the reference holds in float32.
"""

import numpy as np

LD = np.longdouble


def inz(x):
    x = np.asarray(x)
    return np.where(x == 0, 0, 1 / np.where(x == 0, 1, x))


def fvar(weight):
    """The reference's float32 variance ``invert_no_zero(weight)``."""
    w = np.asarray(weight, dtype=np.float32)
    with np.errstate(divide="ignore"):
        return np.where(w == 0, np.float32(0), np.float32(1) / np.where(w == 0, np.float32(1), w)).astype(np.float32)


def rebin_matrix(tra, ra, width_t=0.0):
    """Dense ``R [len(ra), len(tra)]`` float64, one sample at a time: the overlap of the sample's extent with the bin
    at or above it and with the bin below."""
    nra, nt = len(ra), len(tra)
    R = np.zeros((nra, nt))
    width_ra = np.median(np.abs(np.diff(ra)))
    lowest, highest = ra[0] - width_ra / 2, ra[-1] + width_ra / 2
    if width_t == 0:
        width_t = 1e-10
    for i in range(nt):
        j = int(np.searchsorted(ra, tra[i]))
        lo, hi = tra[i] - width_t / 2.0, tra[i] + width_t / 2.0
        if hi > lowest and j < nra:
            R[j, i] = min(max((hi - (ra[j] - width_ra / 2)) / width_t, 0.0), 1.0)
        if lo < highest and j > 0:
            R[j - 1, i] = min(max(((ra[j - 1] + width_ra / 2) - lo) / width_t, 0.0), 1.0)
    return R


def rebin_twin(vis, weight, lsd, samples, start, mode):
    """``vis [nrow, nt]``, ``weight [nrow / fold, nt]`` -> ``(vis [nrow, samples] c128, weight, nsample, effective_ra
    [nrow / fold, samples] f64)``; ``mode``: ``"uniform"`` or ``"inverse_variance"``."""
    lsd = np.asarray(lsd, dtype=np.float64)
    target = np.linspace(start, start + 1, samples, endpoint=False)
    ra = np.linspace(0.0, 360.0, samples, endpoint=False)
    R = rebin_matrix(lsd, target, np.median(np.abs(np.diff(lsd)))).astype(LD)
    nrow, nw = vis.shape[0], weight.shape[0]
    fold = nrow // nw
    wt = np.asarray(weight, dtype=np.float32)
    m = (wt > 0).astype(LD)
    if mode == "uniform":
        w, v = m, fvar(wt).astype(LD)
    else:
        w = v = wt.astype(LD)
    norm = inz(w @ R.T)  # [nw, samples]
    wv_re = (np.repeat(w, fold, axis=0) * vis.real.astype(LD)) @ R.T
    wv_im = (np.repeat(w, fold, axis=0) * vis.imag.astype(LD)) @ R.T
    nf = np.repeat(norm, fold, axis=0)
    out = (nf * wv_re).astype(np.float64) + 1j * (nf * wv_im).astype(np.float64)
    nsample = (m @ R.T).astype(np.float64)
    wout = inz(norm**2 * (v @ (R.T**2)))
    era = 360 * (norm * ((w * lsd.astype(LD)[None, :]) @ R.T) - LD(start))
    era = np.where(wout.astype(np.float32) == 0, ra[None, :].astype(LD), era)
    return out, wout.astype(np.float64), nsample, era.astype(np.float64)


def grad_twin(x, si, mask):
    """``(gradient c128-as-two-longdoubles, mask)`` of one row wrapped with period 360: second-order differences on
    uneven positions; flagged where a neighbour is flagged or the result is not finite."""
    n = len(x)
    si = np.asarray(si).astype(LD)
    shift = np.ceil(si[-1] / 360) * 360
    s = np.concatenate(([si[-1] - shift], si, [si[0] + shift]))
    xr = np.concatenate(([x[-1]], x, [x[0]]))
    mk = np.concatenate(([mask[-1]], mask, [mask[0]])).astype(bool)
    gr, gi, out_mask = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n):
            k = i + 1
            hd, hs = s[k] - s[k - 1], s[k + 1] - s[k]
            a, b, c = -hs / (hd * (hd + hs)), (hs - hd) / (hd * hs), hd / (hs * (hd + hs))
            r = a * LD(xr[k - 1].real) + b * LD(xr[k].real) + c * LD(xr[k + 1].real)
            q = a * LD(xr[k - 1].imag) + b * LD(xr[k].imag) + c * LD(xr[k + 1].imag)
            bad = mk[k - 1] or mk[k] or mk[k + 1] or hd == 0 or hs == 0 or not (np.isfinite(r) and np.isfinite(q))
            out_mask[i] = bad
            if not bad:
                gr[i], gi[i] = r, q
    return gr, gi, out_mask


def gradient_twin(vis, weight, era, ra, ref_vis, ref_weight, ref_pos):
    """``vis, weight, era [nrow, nra]``; ``ref_pos [nrow, nra]`` or ``[nra]`` -> corrected ``(vis c128, weight f64)``."""
    out = np.array(vis, dtype=np.complex128)
    wout = np.array(weight, dtype=np.float64)
    ra = np.asarray(ra, dtype=np.float64).astype(LD)
    for k in range(vis.shape[0]):
        if not np.any(weight[k]):
            continue
        pos = ref_pos[k] if np.ndim(ref_pos) > 1 else ref_pos
        gr, gi, mask = grad_twin(ref_vis[k], pos, ref_weight[k] == 0)
        d = (np.asarray(era[k]).astype(LD) - ra) * (weight[k] > 0)
        out[k] = (vis[k].real.astype(LD) - gr * d).astype(np.float64) + 1j * (vis[k].imag.astype(LD) - gi * d).astype(np.float64)
        wout[k] = weight[k] * ~mask
    return out, wout


def interp_taps(kind, lsd, grid):
    """Per grid point: the samples read, their float64 coefficients and whether the point is flagged."""
    n, delta = len(lsd), np.median(np.abs(np.diff(lsd)))
    taps, coeffs, bad = [], [], []
    for x in grid:
        j = int(np.searchsorted(lsd, x, side="left"))
        if kind == "nearest":
            p, q = max(0, j - 1), min(n - 1, j)
            i = p if abs(x - lsd[p]) < abs(x - lsd[q]) else q
            taps.append([i])
            coeffs.append([1.0])
            bad.append(abs(lsd[i] - x) > delta)
        elif kind == "linear":
            i1, i2, out = j - 1, j, False
            if i1 == -1:
                i1, i2, out = 0, 1, True
            if i2 == n:
                i1, i2, out = n - 2, n - 1, True
            dx1, dx2 = x - lsd[i1], lsd[i2] - x
            nrm = 0.0 if dx1 + dx2 == 0 else 1.0 / (dx1 + dx2)
            taps.append([i1, i2])
            coeffs.append([dx2 * nrm, dx1 * nrm])
            bad.append(out or abs(lsd[i1] - x) > delta or abs(lsd[i2] - x) > delta)
        else:
            raw = [j - 2, j - 1, j, j + 1]
            ii = [min(max(i, 0), n - 1) for i in raw]
            h = lsd[ii[2]] - lsd[ii[1]]
            u = (x - lsd[ii[1]]) * (0.0 if h == 0 else 1.0 / h)
            taps.append(ii)
            coeffs.append([0.5 * (u * ((2 - u) * u - 1)), 0.5 * (u**2 * (3 * u - 5) + 2), 0.5 * (u * ((4 - 3 * u) * u + 1)), 0.5 * (u**2 * (u - 1))])
            bad.append(any(i != r for i, r in zip(ii, raw)) or any(abs(x - lsd[i]) > 2.0 * delta for i in ii))
    return np.array(taps).T, np.array(coeffs).T, np.array(bad)


def interp_twin(kind, vis, weight, lsd, samples, start, end, phase_in=None, phase_out=None):
    """``vis, weight [nrow, nt]`` -> ``(vis [nrow, samples] c128, weight f64)``.  ``phase_in [nrow, nt]`` /
    ``phase_out [nrow, samples]`` complex: the mix-down factor and the factor whose conjugate mixes back up."""
    lsd = np.asarray(lsd, dtype=np.float64)
    grid = np.arange(0, samples, dtype=np.float64) / samples * (end - start) + start
    tap, coeff, bad = interp_taps(kind, lsd, grid)
    y = np.asarray(vis, dtype=np.complex128)
    if phase_in is not None:
        y = y * phase_in
    c = coeff.astype(LD)
    re = sum(c[k][None, :] * y.real.astype(LD)[:, tap[k]] for k in range(len(tap)))
    im = sum(c[k][None, :] * y.imag.astype(LD)[:, tap[k]] for k in range(len(tap)))
    out = re.astype(np.float64) + 1j * im.astype(np.float64)
    if kind == "nearest":
        wout = np.asarray(weight, dtype=np.float64)[:, tap[0]].copy()
    else:
        var = sum(c[k][None, :] ** 2 * fvar(weight).astype(LD)[:, tap[k]] for k in range(len(tap)))
        ok = np.all([weight[:, tap[k]] > 0 for k in range(len(tap))], axis=0)
        wout = (inz(var) * ok).astype(np.float64)
    wout[:, bad] = 0.0
    if phase_out is not None:
        out = out * np.conj(phase_out)
        wout = wout * (np.abs(phase_out) > 0)
    return out, wout
