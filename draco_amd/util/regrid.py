"""Host half of the Lanczos / Wiener regridder (``draco/util/regrid.py``).

The Lanczos matrix depends on the times only: it is evaluated here in float64 with the reference's expressions
(``np.sinc``) and handed to ``libdraco_amd.so`` in compact form -- per grid point the span of time samples in reach and
the kernel values on it.  The solve itself (``band_wiener``, ``regrid.py:14-89``) is ``csrc/regrid.hip``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from ..device import ptr


def lanczos_kernel(x, a):
    """Lanczos interpolation kernel (``regrid.py:92-106``)."""
    return np.where(np.abs(x) < a, np.sinc(x) * np.sinc(x / a), np.zeros_like(x))


def lanczos_forward_matrix(x, y, a=5, periodic=False):
    """Lanczos interpolation matrix ``[len(y), len(x)]`` from the regular points ``x`` onto ``y`` (``regrid.py:109-135``)."""
    if periodic:
        raise NotImplementedError("periodic Lanczos matrices are not supported")
    dx = x[1] - x[0]
    sep = (x[np.newaxis, :] - y[:, np.newaxis]) / dx
    return lanczos_kernel(sep, a)


def compact_rows(R):
    """``(start, end, values)`` of a matrix whose rows are zero outside one span each: ``values`` concatenates
    ``R[g, start[g]:end[g]]`` (``band_wiener`` finds the same spans, ``regrid.py:64-66``)."""
    nz = R != 0
    start = nz.argmax(axis=-1).astype(np.int32)
    end = (R.shape[-1] - nz[..., ::-1].argmax(axis=-1)).astype(np.int32)
    empty = ~nz.any(axis=-1)
    start[empty] = 0
    end[empty] = 0
    vals = np.concatenate([R[g, start[g] : end[g]] for g in range(R.shape[0])]) if R.shape[0] else np.zeros(0)
    return start, end, np.ascontiguousarray(vals, dtype=np.float64)


class RegridPlan:
    """The device tables of one time grid (``dmm_regrid_plan``): build once per day, use for every row."""

    def __init__(self, ctx, grid, times, kernel_width):
        # in blocks of grid points: the dense [ngrid, nt] matrix of a long day is tens of MB of zeros.  Element for
        # element the expression of lanczos_forward_matrix(grid, times, a).T
        grid = np.asarray(grid, dtype=np.float64)
        times = np.asarray(times, dtype=np.float64)
        dx = grid[1] - grid[0]
        parts = [compact_rows(lanczos_kernel((grid[g0 : g0 + 256, np.newaxis] - times[np.newaxis, :]) / dx, kernel_width)) for g0 in range(0, len(grid), 256)]
        start = np.concatenate([p[0] for p in parts])
        end = np.concatenate([p[1] for p in parts])
        vals = np.concatenate([p[2] for p in parts])
        self.ctx, self.ngrid, self.nt, self.kernel_width = ctx, len(grid), len(times), int(kernel_width)
        self.handle = C.c_void_p()
        vals = vals if len(vals) else np.zeros(1)
        _lib.check(
            _lib.lib.dmm_regrid_plan_create(ctx.handle, self.nt, self.ngrid, self.kernel_width, C.c_void_p(start.ctypes.data), C.c_void_p(end.ctypes.data), C.c_void_p(vals.ctypes.data), C.byref(self.handle))
        )

    def close(self):
        if getattr(self, "handle", None):
            _lib.lib.dmm_regrid_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def band_wiener(ctx, plan, vis_d, weight_d, eps, pad, samples, mask_zero_weight=False, mix=None):
    """``[nrow, nt]`` device tensors -> ``(x [nrow, samples] complex64, nw [nrow, samples] float32)`` on the device.

    ``mix``: ``None`` or ``(omega [nrow] f64, feed_mask [nrow] f32, dphi_in [nt] f64, dphi_out [samples] f64)`` device
    tensors: the mix-down and mix-up of ``SiderealRegridder`` fused into the kernel's load and store.
    """
    nrow = int(vis_d.shape[0])
    assert tuple(vis_d.shape) == tuple(weight_d.shape) == (nrow, plan.nt)
    out_vis = ctx.empty((nrow, samples), np.complex64)
    out_w = ctx.empty((nrow, samples), np.float32)
    om, fm, di, do = mix if mix is not None else (None, None, None, None)
    _lib.check(
        _lib.lib.dmm_regrid_band_wiener(
            ctx.handle, plan.handle, ptr(vis_d), ptr(weight_d), nrow, float(eps), int(pad), int(samples), int(bool(mask_zero_weight)), ptr(om), ptr(fm), ptr(di), ptr(do), ptr(out_vis), ptr(out_w)
        )
    )
    return out_vis, out_w


# ---------------------------------------------------------------- rebinning and direct interpolation (csrc/rebin.hip)
def _rebin_fractions(tra, ra, width_t):
    """Per time sample: the bin above it, and whether / how much of it lands in that bin and in the one below
    (``regrid.py:178-209``, vectorised with the scalar loop's expressions in the loop's order)."""
    tra = np.asarray(tra, dtype=np.float64)
    ra = np.asarray(ra, dtype=np.float64)
    inds = np.searchsorted(ra, tra)
    # the typical width of an RA bin
    width_ra = np.median(np.abs(np.diff(ra)))
    lowest_ra = ra[0] - width_ra / 2
    highest_ra = ra[-1] + width_ra / 2
    if width_t == 0:  # nearest-bin assignment: 1 if the sample is inside a bin, 0 otherwise
        width_t = 1e-10
    lower_edge = tra - width_t / 2.0
    upper_edge = tra + width_t / 2.0
    up = (upper_edge > lowest_ra) & (inds < len(ra))
    lo = (lower_edge < highest_ra) & (inds > 0)
    wh = np.clip((upper_edge[up] - (ra[inds[up]] - width_ra / 2)) / width_t, 0.0, 1.0)
    wl = np.clip(((ra[inds[lo] - 1] + width_ra / 2) - lower_edge[lo]) / width_t, 0.0, 1.0)
    return inds, up, wh, lo, wl


def rebin_matrix(tra, ra, width_t=0):
    """The matrix ``[len(ra), len(tra)]`` that rebins time samples onto RA bins: each sample gives every bin the
    fraction of its width ``width_t`` that overlaps the bin (``regrid.py:161-211``)."""
    inds, up, wh, lo, wl = _rebin_fractions(tra, ra, width_t)
    R = np.zeros((np.shape(ra)[0], np.shape(tra)[0]))
    ii = np.arange(R.shape[1])
    R[inds[up], ii[up]] = wh
    R[inds[lo] - 1, ii[lo]] = wl
    return R


def grad_1d(x, si, mask, period=None):
    """``(gradient, mask)`` of ``x`` over the positions ``si``; with ``period`` the two boundary samples are wrapped.
    The gradient is zero, and flagged, wherever it reads a flagged sample or is not finite (``regrid.py:214-270``)."""
    x, si, mask = np.asarray(x), np.asarray(si), np.asarray(mask, dtype=bool)
    if period is not None:
        shift = np.ceil(si[-1] / period) * period  # (the positions may span several periods)
        x = np.concatenate(([x[-1]], x, [x[0]]))
        mask = np.concatenate(([mask[-1]], mask, [mask[0]]))
        si = np.concatenate(([si[-1] - shift], si, [si[0] + shift]))
        sel = slice(1, -1)
    else:
        mask = mask.copy()
        sel = slice(None)
    # a gradient that includes a flagged sample is dropped: spread the flags to both neighbours
    mask = mask | np.concatenate(([False], mask[:-1])) | np.concatenate((mask[1:], [False]))
    with np.errstate(divide="ignore", invalid="ignore"):  # two equal adjacent positions give NaN / inf
        grad = np.gradient(x, si)
    mask |= ~np.isfinite(grad)
    grad[mask] = 0.0
    return grad[sel], mask[sel]


class RebinPlan:
    """The rebinning matrix of one day in CSR form by output bin, on the device (``dmm_rebin``): row pointer, sample
    index and float64 value, the span of samples of every tile of 64 bins, the samples' LSDs and the bin centres.
    Build once per day, use for every row.  The time stamps must not decrease: a bin's samples are then one
    contiguous span, which the kernel stages; anything else raises ``NotImplementedError``."""

    TILE = 64

    def __init__(self, ctx, lsd, target, width_t, start, ra):
        lsd = np.asarray(lsd, dtype=np.float64)
        target = np.asarray(target, dtype=np.float64)
        if np.any(np.diff(lsd) < 0):
            raise NotImplementedError("The rebinner needs non-decreasing time stamps.")
        inds, up, wh, lo, wl = _rebin_fractions(lsd, target, width_t)
        ii = np.arange(len(lsd))
        bins = np.concatenate([inds[up], inds[lo] - 1])
        samp = np.concatenate([ii[up], ii[lo]])
        vals = np.concatenate([wh, wl])
        keep = vals != 0
        bins, samp, vals = bins[keep], samp[keep], vals[keep]
        order = np.lexsort((samp, bins))
        self.nt, self.nra = len(lsd), len(target)
        self.sample_index = samp[order].astype(np.int32)
        self.value = np.ascontiguousarray(vals[order], dtype=np.float64)
        self.row_ptr = np.searchsorted(bins[order], np.arange(self.nra + 1)).astype(np.int32)
        ntile = -(-self.nra // self.TILE)
        span = np.zeros((ntile, 2), dtype=np.int32)
        for t in range(ntile):
            a, b = self.row_ptr[t * self.TILE], self.row_ptr[min((t + 1) * self.TILE, self.nra)]
            if b > a:
                span[t] = self.sample_index[a:b].min(), self.sample_index[a:b].max() + 1
        self.tile_span = span
        self.lsd, self.ra, self.start = lsd, np.asarray(ra, dtype=np.float64), float(start)
        self.ctx = ctx
        if ctx is not None:
            self.row_ptr_d = ctx.to_device(self.row_ptr)
            self.sample_index_d = ctx.to_device(self.sample_index if len(self.sample_index) else np.zeros(1, np.int32))
            self.value_d = ctx.to_device(self.value if len(self.value) else np.zeros(1))
            self.tile_span_d = ctx.to_device(span)
            self.lsd_d = ctx.to_device(lsd)
            self.ra_d = ctx.to_device(self.ra)


def rebin(ctx, plan, vis_d, weight_d, mode, nsample_f32=False):
    """``vis_d [nrow, nt]`` complex64, ``weight_d [nrow / fold, nt]`` float32 device tensors ->
    ``(vis [nrow, nra], weight, nsample, effective_ra [nrow / fold, nra])`` on the device (``dmm_rebin``)."""
    nrow, nwrow = int(vis_d.shape[0]), int(weight_d.shape[0])
    assert tuple(vis_d.shape) == (nrow, plan.nt) and tuple(weight_d.shape) == (nwrow, plan.nt) and nwrow and nrow % nwrow == 0
    out_vis = ctx.empty((nrow, plan.nra), np.complex64)
    out_w = ctx.empty((nwrow, plan.nra), np.float32)
    out_ns = ctx.empty((nwrow, plan.nra), np.float32 if nsample_f32 else np.uint16)
    out_era = ctx.empty((nwrow, plan.nra), np.float32)
    _lib.check(
        _lib.lib.dmm_rebin(
            ctx.handle, int(mode), int(bool(nsample_f32)), ptr(vis_d), ptr(weight_d), nrow, nrow // nwrow, plan.nt, plan.nra, ptr(plan.row_ptr_d), ptr(plan.sample_index_d),
            ptr(plan.value_d), len(plan.value), ptr(plan.tile_span_d), ptr(plan.lsd_d), plan.start, ptr(plan.ra_d), ptr(out_vis), ptr(out_w), ptr(out_ns), ptr(out_era)
        )
    )
    return out_vis, out_w, out_ns, out_era


def rebin_gradient(ctx, vis_d, weight_d, era_d, ra_d, ref_vis_d, ref_weight_d, ref_era_d=None, ref_ra_d=None):
    """In place on ``vis_d`` / ``weight_d [nrow, nra]``: the gradient correction of ``dmm_rebin_gradient``."""
    nrow, nra = (int(s) for s in vis_d.shape)
    assert tuple(weight_d.shape) == tuple(era_d.shape) == tuple(ref_vis_d.shape) == tuple(ref_weight_d.shape) == (nrow, nra)
    _lib.check(_lib.lib.dmm_rebin_gradient(ctx.handle, ptr(vis_d), ptr(weight_d), ptr(era_d), ptr(ra_d), ptr(ref_vis_d), ptr(ref_weight_d), ptr(ref_era_d), ptr(ref_ra_d), nrow, nra))


def regrid_interp(ctx, vis_d, weight_d, tap, coeff, bad, mix=None):
    """``[nrow, nt]`` device tensors -> ``(vis, weight) [nrow, nout]`` on the device: the gather of ``dmm_regrid_interp``
    with the host's ``tap`` / ``coeff [ntap, nout]`` and ``bad [nout]``.  ``mix`` as for :func:`band_wiener`."""
    nrow, nt = (int(s) for s in vis_d.shape)
    ntap, nout = tap.shape
    assert tuple(weight_d.shape) == (nrow, nt) and coeff.shape == (ntap, nout) and bad.shape == (nout,)
    tap_d, coeff_d, bad_d = ctx.to_device(tap, np.int32), ctx.to_device(coeff, np.float64), ctx.to_device(bad, np.uint8)
    out_vis = ctx.empty((nrow, nout), np.complex64)
    out_w = ctx.empty((nrow, nout), np.float32)
    om, fm, di, do = mix if mix is not None else (None, None, None, None)
    _lib.check(_lib.lib.dmm_regrid_interp(ctx.handle, int(ntap), ptr(vis_d), ptr(weight_d), nrow, nt, nout, ptr(tap_d), ptr(coeff_d), ptr(bad_d), ptr(om), ptr(fm), ptr(di), ptr(do), ptr(out_vis), ptr(out_w)))
    ctx.uses(tap_d, coeff_d, bad_d)
    return out_vis, out_w
