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
