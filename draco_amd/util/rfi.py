"""Routines for RFI excision on the GPU (``draco/util/rfi.py``): SumThreshold and the scale-invariant rank operator.

Signatures, defaults and errors are the reference's.  NumPy arrays go in and come out, or device tensors do; the work
is ``dmm_rfi_sumthreshold`` / ``dmm_rfi_sir`` (``csrc/rfi.hip``) either way.  The planes are two-dimensional
``[freq, time]`` (a one-dimensional array is one line); the deprecated ``sir`` is not carried.

``apply_hysteresis_threshold`` is scikit-image's function of that name [3P], which ``RFITransientVisMask`` calls: here
``dmm_rfi_hysteresis`` (``csrc/vismask.hip``).
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..device import Context, ptr


def _flags(ctx, mask):
    """A fresh uint8 device plane, 1 where ``mask`` is set."""
    if isinstance(mask, torch.Tensor):
        return mask.to(ctx.device).ne(0).to(torch.uint8).contiguous()
    return ctx.to_device(np.ascontiguousarray(np.asarray(mask) != 0).view(np.uint8))


def _norm_axes(axes, ndim):
    out = []
    for ax in axes:
        ax = int(ax)
        if ax < -ndim or ax >= ndim:
            raise ValueError(f"axis {ax} is out of bounds for an array of dimension {ndim}")
        out.append(ax % ndim)
    return out


def sumthreshold_steps(max_m, threshold1, rho, axes):
    """The (window, axis, threshold) of every step of the reference's loop, the thresholds by its own expression."""
    window, axis, thr = [], [], []
    m = 1
    while m <= max_m:
        threshold = threshold1 / rho ** (np.log2(m))
        for ax in axes:
            window.append(m)
            axis.append(ax)
            thr.append(float(threshold))
        m *= 2
    return np.array(window, dtype=np.int32), np.array(axis, dtype=np.int32), np.array(thr, dtype=np.float64)


def sumthreshold_device(ctx, data, flag, max_m, threshold1, rho, axes, variance=None, correct_for_missing=True, only_positive=False):
    """SumThreshold on a float64 ``[nf, nt]`` device plane; ``flag`` (uint8) is updated in place and returned."""
    nf, nt = int(data.shape[0]), int(data.shape[1])
    window, axis, thr = sumthreshold_steps(max_m, threshold1, rho, axes)
    if len(window) and int(window.max()) > _lib.DMM_RFI_MAX_ST_WINDOW:
        raise ValueError(f"max_m {max_m}: windows of at most {_lib.DMM_RFI_MAX_ST_WINDOW} samples are supported")
    hit = torch.empty_like(flag)
    _lib.check(
        _lib.lib.dmm_rfi_sumthreshold(
            ctx.handle, ptr(data), ptr(variance), ptr(flag), ptr(hit), nf, nt, len(window), C.c_void_p(window.ctypes.data), C.c_void_p(axis.ctypes.data),
            C.c_void_p(thr.ctypes.data), int(bool(correct_for_missing)), int(bool(only_positive)),
        )
    )
    return flag


def sumthreshold_py(
    data,
    max_m=16,
    start_flag=None,
    threshold1=None,
    remove_median=True,
    correct_for_missing=True,
    variance=None,
    rho=None,
    axes=None,
    only_positive=False,
):
    """SumThreshold outlier detection algorithm (``rfi.py:8-140``).

    Parameters are the reference's: ``data [freq, time]``, ``max_m`` the largest window, ``start_flag`` the initially
    flagged data, ``threshold1`` the first threshold (by default the 95th percentile), ``remove_median``,
    ``correct_for_missing``, ``variance`` (then ``threshold1`` is in units of sigma and must be given), ``rho`` (by
    default 0.9428 with ``correct_for_missing`` and 1.5 without), ``axes`` in flagging order (by default all, last
    first) and ``only_positive``.  Returns the Boolean mask, True marking outliers.  The median and the percentile are
    taken on the host.
    """
    is_tensor = isinstance(data, torch.Tensor)
    ndim = data.dim() if is_tensor else np.ndim(data)
    if ndim not in (1, 2):
        raise ValueError(f"sumthreshold takes [freq, time] planes (or one line), got {ndim} dimensions")
    if variance is not None and threshold1 is None:
        raise RuntimeError("If variance is provided, then must also provide starting threshold in units of sigma.")
    correct_for_missing = bool(correct_for_missing) or variance is not None  # variances are summed, then rooted
    if rho is None:  # the two historical defaults
        rho = 0.9428 if correct_for_missing else 1.5
    axes = _norm_axes(range(ndim - 1, -1, -1) if axes is None else np.atleast_1d(axes).tolist(), ndim)

    ctx = Context.get()
    d = ctx.to_device(data if is_tensor else np.asarray(data), np.float64)
    if d is data:
        d = d.clone()
    flag = _flags(ctx, start_flag) if start_flag is not None else torch.zeros(d.shape, dtype=torch.uint8, device=ctx.device)
    var = None if variance is None else ctx.to_device(variance if isinstance(variance, torch.Tensor) else np.asarray(variance), np.float64)
    if ndim == 1:  # one line along time
        d, flag = d.reshape(1, -1), flag.reshape(1, -1)
        var = None if var is None else var.reshape(1, -1)
        axes = [1 for _ in axes]
    if tuple(flag.shape) != tuple(d.shape) or (var is not None and tuple(var.shape) != tuple(d.shape)):
        raise ValueError("data, start_flag and variance must have one shape")

    if remove_median or threshold1 is None:
        h = d.cpu().numpy()
        keep = np.isfinite(h) & ~(flag.cpu().numpy() != 0)
        if remove_median:
            med = np.median(h[keep])
            h = h - med
            d = ctx.to_device(h)
        if threshold1 is None:
            threshold1 = np.percentile(h[keep], 95.0)

    sumthreshold_device(ctx, d, flag, max_m, threshold1, rho, axes, variance=var, correct_for_missing=correct_for_missing, only_positive=only_positive)
    out = flag.ne(0)
    if ndim == 1:
        out = out.reshape(-1)
    return out if is_tensor else out.cpu().numpy()


sumthreshold = sumthreshold_py  # the reference exports the routine under both names


def hysteresis_device(ctx, x, low, high, out=None, info=None):
    """The hysteresis threshold of float64 ``[..., nf, nt]`` device planes (``dmm_rfi_hysteresis``): a new uint8 tensor,
    or OR-ed into ``out``.  ``info``: a dict that receives ``sweeps``."""
    nf, nt = int(x.shape[-2]), int(x.shape[-1])
    nplane = x.numel() // (nf * nt) if nf * nt else 0
    accumulate = out is not None
    if out is None:
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    sweeps = C.c_int32(0)
    if x.numel():
        state = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        changed = torch.empty(1, dtype=torch.int32, device=x.device)
        # planes beyond the grid's 65535 go in runs
        xf, of, sf = x.reshape(nplane, nf, nt), out.reshape(nplane, nf, nt), state.reshape(nplane, nf, nt)
        total = 0
        for p0 in range(0, nplane, 65535):
            p1 = min(nplane, p0 + 65535)
            _lib.check(_lib.lib.dmm_rfi_hysteresis(ctx.handle, ptr(xf[p0:p1]), p1 - p0, nf, nt, float(low), float(high), int(accumulate), ptr(sf[p0:p1]), ptr(changed),
                                                   ptr(of[p0:p1]), C.byref(sweeps)))
            total = max(total, sweeps.value)
        sweeps = C.c_int32(total)
    if info is not None:
        info["sweeps"] = int(sweeps.value)
    return out


def apply_hysteresis_threshold(image, low, high):
    """Hysteresis threshold (scikit-image's ``filters.apply_hysteresis_threshold``, as ``flagging.py:1262`` calls it).

    True at every sample above ``low`` whose connected region of samples above ``low`` -- neighbours along the last two
    axes, no diagonals -- holds a sample above ``high``.  Comparisons are strict; a NaN is in neither set; ``low`` is
    ``min(low, high)``.  ``image``: one line, one ``[nf, nt]`` plane, or planes ``[..., nf, nt]`` that are treated one
    by one.  NumPy in, NumPy out; a device tensor in, a device tensor out.
    """
    is_tensor = isinstance(image, torch.Tensor)
    ndim = image.dim() if is_tensor else np.ndim(image)
    if ndim < 1:
        raise ValueError("apply_hysteresis_threshold needs at least one dimension")
    if np.isnan(low) or np.isnan(high):
        raise ValueError("apply_hysteresis_threshold: a threshold is NaN")
    if (image.is_complex() if is_tensor else np.iscomplexobj(image)):
        raise ValueError("apply_hysteresis_threshold takes real data")
    ctx = Context.get()
    x = ctx.to_device(image if is_tensor else np.asarray(image), np.float64).contiguous()
    if ndim == 1:
        x = x.reshape(1, -1)
    out = hysteresis_device(ctx, x, low, high).ne(0)
    if ndim == 1:
        out = out.reshape(-1)
    return out if is_tensor else out.cpu().numpy()


_SIR_WORK = {}


def sir_device(ctx, flag, eta, axis, out=None):
    """``flag | SIR(flag)`` along ``axis`` (0 or 1) of a uint8 ``[nf, nt]`` device plane; with ``out`` the result is
    OR-ed into it."""
    nf, nt = int(flag.shape[0]), int(flag.shape[1])
    work = _SIR_WORK.get(flag.device)  # one grow-only scratch per device: the task calls this once per pass
    if work is None or work.numel() < 2 * nf * nt:
        work = _SIR_WORK[flag.device] = torch.empty(2 * nf * nt, dtype=torch.float64, device=flag.device)
    accumulate = out is not None
    if out is None:
        out = torch.empty_like(flag)
    _lib.check(_lib.lib.dmm_rfi_sir(ctx.handle, ptr(flag), nf, nt, int(axis), float(eta), int(accumulate), ptr(work), ptr(out)))
    return out


def _sir_planes(basemask, etas, axes):
    is_tensor = isinstance(basemask, torch.Tensor)
    ndim = basemask.dim() if is_tensor else np.ndim(basemask)
    if ndim not in (1, 2):
        raise ValueError(f"the SIR operator takes [freq, time] planes (or one line), got {ndim} dimensions")
    axes = _norm_axes(axes, ndim)
    ctx = Context.get()
    flag = _flags(ctx, basemask)
    if ndim == 1:
        flag = flag.reshape(1, -1)
        axes = [1 for _ in axes]
    out = None
    for ax, et in zip(axes, etas):
        out = sir_device(ctx, flag, et, ax, out=out)
    out = out.ne(0)
    if ndim == 1:
        out = out.reshape(-1)
    return out if is_tensor else out.cpu().numpy()


def _sir_lastaxis(basemask, eta=0.2, axis=-1):
    """The scale-invariant rank (SIR) operator along one axis (``rfi.py:147-198``, arXiv:1201.3364v2).

    ``basemask``: True for flagged points; ``eta``: aggressiveness, 0 returns ``basemask`` and 1 flags everything.
    Returns the mask after the operator, same shape.
    """
    return _sir_planes(basemask, (eta,), (axis,))


sir1d = _sir_lastaxis  # the public name of the single-axis form


def scale_invariant_rank(basemask, eta=0.2, axis=-1):
    """Apply the SIR operator along one or more axes and return the logical OR of the masks (``rfi.py:205-257``).

    ``eta`` may be a tuple of the length of ``axis``.
    """
    if (basemask.dim() if isinstance(basemask, torch.Tensor) else np.ndim(basemask)) < 1:
        raise ValueError("basemask must have at least one dimension.")
    axis = tuple(np.atleast_1d(axis).tolist())
    eta = (eta,) * len(axis) if np.ndim(eta) == 0 else tuple(eta)
    if len(eta) != len(axis):
        raise ValueError(f"If eta is a tuple, it must have the same length as axis.Got len(eta)={len(eta)} and len(axis)={len(axis)}.")
    return _sir_planes(basemask, eta, axis)
