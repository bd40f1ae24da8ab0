"""Masked moving median (``draco/util/filters.py:99-130``), the weighted moving median of the chi-squared mask, and the
delay null-space filter (``draco/util/filters.py:133-212``) on the GPU.

``medfilt`` wraps caput's ``moving_weighted_median`` [3P] in the reference; here it is ``dmm_rfi_medfilt``
(``csrc/rfi.hip``) under the conventions of DESIGN.md section 7i: the window is centred on the sample and clipped at
the array's edge, the result is ``0.5 * (v[(n-1)//2] + v[n//2])`` of the ``n`` unmasked samples ``v`` of the window in
ascending order and NaN for an empty window.  Window sizes are odd.  ``medfilt`` has 0/1 weights only: a sample is masked
or not.  :func:`moving_weighted_median` takes real weights and longer windows (``dmm_rfi_wmedfilt``).

``null_filter`` projects out (or keeps) the span of the Fourier modes ``exp(2 pi i f s)``, ``f = linspace(-cutoff,
cutoff, num_modes)``, on the unmasked samples: ``dmm_nullfilter_build`` (``csrc/nullfilter.hip``)
takes the SVD of the real form of that matrix by a batched one-sided Jacobi in float64.  :func:`build_null_filters` is
the batched form the tasks of ``draco_amd.analysis.delay`` use.

``lowpass_weighted_convolution_filter`` / ``highpass_weighted_convolution_filter`` (``draco/util/filters.py:22-96``): the
taps are designed on the host as the reference designs them, the weighted convolution is ``dmm_wconv_filter``
(``csrc/vismask.hip``), a direct sum in float64.
"""

from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..device import Context, ptr


def _check_window(size, ndim, max_window, max_strip):
    if np.ndim(size) == 0:
        size = (int(size),) * ndim
    size = tuple(int(s) for s in size)
    if len(size) != ndim:
        raise ValueError(f"size {size} does not match a {ndim}-dimensional array")
    if ndim == 1:
        size = (size[0], 1)
    if any(s < 1 or s % 2 == 0 for s in size):
        raise ValueError(f"window sizes must be odd and positive, got {size}")
    if max(size) > max_window or size[0] * size[1] > max_strip:
        raise ValueError(f"window {size} is beyond the supported bound: each size at most {max_window}, their product at most {max_strip}")
    return size


def check_size(size, ndim):
    """The window as ``(size_f, size_t)``; ``ValueError`` for an even size or one beyond the kernel's bound."""
    return _check_window(size, ndim, _lib.DMM_RFI_MAX_WINDOW, _lib.DMM_RFI_MAX_STRIP)


def medfilt_device(ctx, x, flag, size):
    """``x [..., nf, nt]`` float64 and ``flag`` uint8 device tensors -> the filtered planes, a new tensor."""
    nf, nt = int(x.shape[-2]), int(x.shape[-1])
    nplane = int(np.prod(x.shape[:-2])) if x.dim() > 2 else 1
    out = torch.empty_like(x)
    _lib.check(_lib.lib.dmm_rfi_medfilt(ctx.handle, ptr(x), ptr(flag), nplane, nf, nt, int(size[0]), int(size[1]), ptr(out)))
    return out


def quantile_device(ctx, y, flag, q, count=False):
    """The "split" quantile of the unflagged samples of every row of ``y [nrow, n]`` (float64 device tensor); with
    ``count`` also the number of unflagged samples of every row (int32)."""
    nrow, n = int(y.shape[0]), int(y.shape[1])
    if n > _lib.DMM_RFI_MAX_ROW:
        raise ValueError(f"rows of {n} samples: at most {_lib.DMM_RFI_MAX_ROW} are supported")
    out = torch.empty(nrow, dtype=torch.float64, device=y.device)
    cnt = torch.empty(nrow, dtype=torch.int32, device=y.device) if count else None
    _lib.check(_lib.lib.dmm_rfi_quantile(ctx.handle, ptr(y), ptr(flag), nrow, n, float(q), ptr(out), ptr(cnt)))
    return (out, cnt) if count else out


def _flag_tensor(ctx, mask):
    if isinstance(mask, torch.Tensor):
        return mask.to(ctx.device).ne(0).to(torch.uint8).contiguous() if mask.dtype != torch.uint8 else mask.to(ctx.device).contiguous()
    return ctx.to_device(np.ascontiguousarray(np.asarray(mask) != 0).view(np.uint8))


def medfilt(x, mask, size, *args):
    """Masked moving median of ``x``.

    ``x``: a 1-D array or ``[..., freq, time]`` planes, real or complex (complex input is filtered as its real and
    imaginary parts); ``mask``: True where a sample is left out; ``size``: the odd window size in each dimension.
    NumPy in, NumPy out; device tensors in, a device tensor out.  Data within the mask is undefined, as in the reference.
    """
    if args:
        raise NotImplementedError("medfilt takes no further arguments: the moving median has 0/1 weights only")
    is_tensor = isinstance(x, torch.Tensor)
    ndim = x.dim() if is_tensor else np.ndim(x)
    if ndim < 1:
        raise ValueError("medfilt needs at least one dimension")
    size = check_size(size, min(ndim, 2))
    if tuple(x.shape) != tuple(mask.shape):
        raise ValueError(f"data {tuple(x.shape)} and mask {tuple(mask.shape)} differ in shape")
    if (x.is_complex() if is_tensor else np.iscomplexobj(x)):
        return medfilt(x.real, mask, size[: min(ndim, 2)]) + 1.0j * medfilt(x.imag, mask, size[: min(ndim, 2)])
    ctx = Context.get()
    xt = ctx.to_device(x if is_tensor else np.asarray(x), np.float64)
    ft = _flag_tensor(ctx, mask)
    if ndim == 1:
        xt, ft = xt.reshape(-1, 1), ft.reshape(-1, 1)
    out = medfilt_device(ctx, xt, ft, size)
    if ndim == 1:
        out = out.reshape(-1)
    return out if is_tensor else out.cpu().numpy()


# ---- the weighted moving median


def check_weighted_size(size, ndim):
    """The window of the weighted median as ``(size_f, size_t)``; ``ValueError`` for an even size or one beyond the
    kernel's bound (each size at most ``DMM_RFI_WMED_MAX_WINDOW``, their product at most ``DMM_RFI_WMED_MAX_STRIP``)."""
    return _check_window(size, ndim, _lib.DMM_RFI_WMED_MAX_WINDOW, _lib.DMM_RFI_WMED_MAX_STRIP)


def moving_weighted_median_device(ctx, x, w, size):
    """``x [..., nf, nt]`` and ``w`` float64 device tensors of one shape -> the weighted moving median of every plane,
    a new tensor.  ``size``: ``(size_f, size_t)`` as :func:`check_weighted_size` returns it.  Weights that are
    negative or NaN are not looked for here: such a sample is dropped."""
    nf, nt = int(x.shape[-2]), int(x.shape[-1])
    nplane = int(np.prod(x.shape[:-2])) if x.dim() > 2 else 1
    out = torch.empty_like(x)
    _lib.check(_lib.lib.dmm_rfi_wmedfilt(ctx.handle, ptr(x), ptr(w), nplane, nf, nt, int(size[0]), int(size[1]), ptr(out)))
    return out


def moving_weighted_median(x, w, size):
    """Weighted moving median of ``x`` (caput's ``moving_weighted_median`` [3P] as ``flagging.py:1670-1773`` calls it).

    ``x``: a 1-D array or ``[..., freq, time]`` real planes; ``w``: the weights, of the same shape; ``size``: the odd
    window size in each dimension.  NumPy in, NumPy out; device tensors in, a device tensor out.

    The convention: the window is centred on the sample and clipped at the array's edge, without
    padding.  Only samples with a weight > 0 take part.  With the window's samples in ascending order, ``W`` their
    total weight and ``c(v)`` the weight of all samples ``<= v``: ``lo`` is the smallest sample with ``c(lo) >= W/2``,
    ``hi`` the smallest with ``c(hi) > W/2``, and the result is ``0.5 * (lo + hi)``; a window without a sample gives
    NaN.  With 0/1 weights this is :func:`medfilt`'s ``0.5 * (v[(n-1)//2] + v[n//2])``.  Signed zeros and NaN samples
    as there.

    Weight sums are float64.  Where every partial sum is exact (integer or dyadic weights of modest size) the result is
    exactly the stated one, whatever the shape of the plane.  Elsewhere it is the stated one wherever ``c(v)`` misses
    ``W/2`` by more than the rounding of the sums; a window whose split is decided by a rounding error may give
    ``lo`` or ``0.5 * (lo + hi)``.

    ``ValueError``: an even or non-positive size, a window beyond the bound (:func:`check_weighted_size`), shapes that
    differ, complex data, and -- for NumPy input -- a negative or NaN weight.  Device input is not inspected: there a
    negative or NaN weight is undefined.
    """
    is_tensor = isinstance(x, torch.Tensor)
    ndim = x.dim() if is_tensor else np.ndim(x)
    if ndim < 1:
        raise ValueError("moving_weighted_median needs at least one dimension")
    size = check_weighted_size(size, min(ndim, 2))
    if tuple(x.shape) != tuple(w.shape):
        raise ValueError(f"data {tuple(x.shape)} and weight {tuple(w.shape)} differ in shape")
    if (x.is_complex() if is_tensor else np.iscomplexobj(x)):
        raise ValueError("moving_weighted_median takes real data")
    if not is_tensor:
        wh = np.asarray(w, dtype=np.float64)
        if np.isnan(wh).any() or (wh < 0).any():
            raise ValueError("moving_weighted_median: weights must be non-negative numbers")
    ctx = Context.get()
    xt = ctx.to_device(x if is_tensor else np.asarray(x), np.float64)
    wt = ctx.to_device(w if is_tensor else wh, np.float64)
    if ndim == 1:
        xt, wt = xt.reshape(-1, 1), wt.reshape(-1, 1)
    out = moving_weighted_median_device(ctx, xt.contiguous(), wt.contiguous(), size)
    if ndim == 1:
        out = out.reshape(-1)
    return out if is_tensor else out.cpu().numpy()


# ---- the weighted convolution filter


def convolution_taps(samples, cutoff):
    """The FIR taps of the weighted convolution filter, float64 on the host, exactly as the reference designs them: the
    median sampling rate ``fs``, an odd ``order = ceil(fs / cutoff) // 2 * 2 + 1`` and a flat-top windowed
    ``scipy.signal.firwin``.  A ``ValueError`` of firwin (a cutoff at or above ``fs / 2``) propagates."""
    from scipy import signal

    fs = 1 / np.median(abs(np.diff(samples)))
    order = int(np.ceil(fs / cutoff) // 2 * 2 + 1)
    taps = np.ascontiguousarray(signal.firwin(order, cutoff, window="flattop", fs=fs), dtype=np.float64)
    if len(taps) > _lib.DMM_WCONV_MAX_TAPS:
        raise ValueError(f"weighted convolution filter: {len(taps)} taps, at most {_lib.DMM_WCONV_MAX_TAPS} are supported")
    return taps


def wconv_filter_device(ctx, data, weight, taps, highpass=False):
    """``data [..., n]`` (complex64 with a float32 weight, or complex128 / float64 with a float64 weight) and ``weight``
    of the same shape, contiguous device tensors; ``taps`` float64 on the host or the device.  Returns the low-pass
    ``conv(d w) inz(conv(w))`` (or ``d`` minus it) as a new complex128 / float64 tensor."""
    kind = {torch.complex64: (_lib.DMM_REDUCE_C64, torch.float32, torch.complex128), torch.complex128: (_lib.DMM_REDUCE_C128, torch.float64, torch.complex128),
            torch.float64: (_lib.DMM_REDUCE_F64, torch.float64, torch.float64)}.get(data.dtype)
    if kind is None:
        raise TypeError(f"weighted convolution filter: data of type {data.dtype} is not supported")
    if weight.dtype != kind[1] or tuple(weight.shape) != tuple(data.shape):
        raise TypeError(f"weighted convolution filter: {data.dtype} data {tuple(data.shape)} needs a {kind[1]} weight of the same shape, got {weight.dtype} {tuple(weight.shape)}")
    taps_d = taps if isinstance(taps, torch.Tensor) else ctx.to_device(np.ascontiguousarray(taps, dtype=np.float64))
    data, weight = data.contiguous(), weight.contiguous()
    out = torch.empty(data.shape, dtype=kind[2], device=data.device)
    n = int(data.shape[-1])
    if data.numel():
        _lib.check(_lib.lib.dmm_wconv_filter(ctx.handle, kind[0], ptr(data), ptr(weight), data.numel() // n, n, ptr(taps_d), int(taps_d.numel()), int(bool(highpass)), ptr(out)))
    ctx.uses(taps_d)
    return out


def _wconv(data, weight, samples, cutoff, axis, highpass):
    is_tensor = isinstance(data, torch.Tensor)
    taps = convolution_taps(np.asarray(samples.cpu() if isinstance(samples, torch.Tensor) else samples), cutoff)
    ctx = Context.get()
    d = data.to(ctx.device) if is_tensor else ctx.to_device(np.asarray(data))
    w = weight.to(ctx.device) if isinstance(weight, torch.Tensor) else ctx.to_device(np.asarray(weight))
    if d.dtype == torch.float32:
        d = d.to(torch.float64)
    if d.dtype not in (torch.complex64, torch.complex128, torch.float64):
        raise TypeError(f"weighted convolution filter: data of type {d.dtype} is not supported")
    if w.is_complex():
        raise TypeError("weighted convolution filter: the weight must be real")
    w = torch.broadcast_to(w.to(torch.float32 if d.dtype == torch.complex64 else torch.float64), d.shape)
    d, w = torch.movedim(d, axis, -1).contiguous(), torch.movedim(w, axis, -1).contiguous()
    out = torch.movedim(wconv_filter_device(ctx, d, w, taps, highpass), -1, axis)
    return out if is_tensor else out.cpu().numpy()


def lowpass_weighted_convolution_filter(data, weight, samples, cutoff, axis=-1):
    """Apply a low-pass weighted convolution filter along an axis (``filters.py:22-65``).

    ``data``: real or complex; ``weight``: its weights; ``samples``: the sample positions along ``axis``; ``cutoff``:
    the cutoff frequency in their inverse units.  With ``h`` the taps (:func:`convolution_taps`) the result is
    ``(h * (d w)) inz(h * w)``, each convolution the slice of the full one that is centred on the data (SciPy's
    ``mode="same"``), ``inz(v) = 1 / v`` and 0 for 0.  NumPy in, NumPy out; device tensors in, a device tensor out.
    The result is complex128 or float64.

    The sums are direct, in float64: over a window of zero weights ``h * w`` is exactly zero and so is the result.  The
    reference convolves by FFT in the input's precision, where that sum is rounding noise and its inverse a number of
    order one.
    """
    return _wconv(data, weight, samples, cutoff, axis, False)


def highpass_weighted_convolution_filter(data, weight, samples, cutoff, axis=-1):
    """Apply a crude high-pass weighted convolution filter along an axis (``filters.py:68-96``): the data minus
    :func:`lowpass_weighted_convolution_filter` of them."""
    return _wconv(data, weight, samples, cutoff, axis, True)


# ---- the delay null-space filter

NULL_MAX_ORDER = 1024  # samples, and Fourier modes, of one filter


def null_filter_window(samples, window):
    """The window ``null_filter`` applies, ``[n]`` float64 on the host: ``True`` is 'nuttall', a false value is no
    window (``None``)."""
    if isinstance(window, (bool, np.bool_)) or window is None:
        if not window:
            return None
        window = "nuttall"
    from ..analysis.delay import _window_coef

    samples = np.asarray(samples, dtype=np.float64)
    return np.ascontiguousarray(_window_coef((samples - samples.min()) / np.ptp(samples), str(window)))


def _check_null_modes(num_modes):
    num_modes = int(num_modes)
    if num_modes < 1:
        raise ValueError(f"null_filter: num_modes must be positive, got {num_modes} (the cutoff is too small for the bandwidth: 4 x bandwidth x cutoff < 0.5)")
    if num_modes == 1:
        raise NotImplementedError(
            "null_filter: num_modes == 1 leaves the single, unpaired mode exp(2 pi i cutoff s), which makes the filter genuinely complex; "
            "only the real filters of two or more modes (symmetric about zero delay) run on the GPU"
        )
    if num_modes > NULL_MAX_ORDER:
        raise ValueError(f"null_filter: {num_modes} modes, the kernels take 2 ... {NULL_MAX_ORDER}")
    return num_modes


def build_null_filters(ctx, samples_d, cutoffs, num_modes, masks, window=None, tol=1e-8, type_="high", workspace_mib=1024, info=None):
    """Build one filter per ``(cutoffs[m], num_modes[m], masks[m])``.

    ``samples_d [n]``: float64 on the device; ``cutoffs [nmat]``, ``num_modes [nmat]`` (or one integer) and ``masks
    [nmat, n]`` (non-zero: sample kept) on the host; ``window``: the ``[n]`` float64 coefficients on the host
    (:func:`null_filter_window`) or ``None``.  Returns ``(nf, status, nkeep, sig)``: ``nf [nmat, n, n]`` float64 on the
    device, and on the host ``status [nmat]`` (non-zero: the Jacobi sweeps of that matrix did not converge, its filter
    is not to be used), ``nkeep [nmat]`` (singular values above ``tol`` times the largest) and ``sig [nmat, max
    num_modes]`` (the singular values in descending order, zero beyond a matrix's own ``num_modes``).  Matrices with
    different ``num_modes`` go through ``dmm_nullfilter_build`` together (one block per matrix), in chunks whose factors
    fit ``workspace_mib``.
    ``info``: a dict that receives ``sweeps [nmat]``."""
    masks = np.ascontiguousarray(np.asarray(masks) != 0).view(np.uint8)
    nmat, n = masks.shape
    cutoffs = np.asarray(cutoffs, dtype=np.float64).reshape(nmat)
    kk = np.broadcast_to(np.asarray(num_modes, dtype=np.int64), (nmat,))
    for k in np.unique(kk):
        _check_null_modes(k)
    if not 1 <= n <= NULL_MAX_ORDER:
        raise ValueError(f"null_filter: {n} samples, the kernels take 1 ... {NULL_MAX_ORDER}")
    if type_ not in {"high", "low"}:
        raise ValueError(f"Filter type must be one of [high, low]. Got {type_}")
    kmax = int(kk.max()) if nmat else 0
    nf = ctx.empty((nmat, n, n), np.float64)
    status, nkeep, sweeps = (np.zeros(nmat, dtype=np.int32) for _ in range(3))
    sig = np.zeros((nmat, kmax), dtype=np.float64)
    window_d = ctx.to_device(np.ascontiguousarray(window, dtype=np.float64)) if window is not None else None
    per = max(1, min(65535, (int(workspace_mib) << 20) // (8 * max(kmax, 1) * n)))
    for m0 in range(0, nmat, per):
        m1 = min(nmat, m0 + per)
        nm, kp = m1 - m0, int(kk[m0:m1].max())
        modes = np.zeros((nm, kp), dtype=np.float64)
        for r in range(nm):
            modes[r, : kk[m0 + r]] = np.linspace(-cutoffs[m0 + r], cutoffs[m0 + r], int(kk[m0 + r]))
        modes_d, masks_d, kk_d = ctx.to_device(modes), ctx.to_device(np.ascontiguousarray(masks[m0:m1])), ctx.to_device(kk[m0:m1].astype(np.int32))
        sig_d = ctx.empty((nm, kp), np.float64)
        words = ctx.zeros((3, nm), np.int32)
        _lib.check(
            _lib.lib.dmm_nullfilter_build(
                ctx.handle, int(n), int(nm), kp, ptr(kk_d), int(type_ == "low"), float(tol), ptr(samples_d), ptr(modes_d), ptr(masks_d), ptr(window_d), ptr(nf[m0:m1]), ptr(sig_d),
                ptr(words[0]), ptr(words[1]), ptr(words[2]),
            )
        )
        w = words.cpu().numpy()
        nkeep[m0:m1], status[m0:m1], sweeps[m0:m1] = w[0], w[1], w[2]
        sig[m0:m1, :kp] = -np.sort(-sig_d.cpu().numpy(), axis=1)
        ctx.uses(modes_d, masks_d, kk_d, sig_d, words)
    ctx.uses(window_d)
    if info is not None:
        info["sweeps"] = sweeps
    return nf, status, nkeep, sig


def null_filter(samples, cutoff, mask, num_modes=200, tol=1e-8, window=True, type_="high", lapack_driver="gesvd", device=True):
    """Create a high-pass or low-pass filter by nulling Fourier modes (``filters.py:133-212``).

    ``samples [n]``: where there is data (at most 1024); ``cutoff``: the Fourier-inverse cut; ``mask [n]``: non-zero
    where a sample is kept (as in the reference, whose tasks pass ``f_mask``); ``num_modes``: Fourier modes in
    ``[-cutoff, cutoff]``; ``tol``: relative cut on the singular values; ``window``: ``True`` ('nuttall'), a window name,
    or a false value; ``type_``: 'high' or 'low'.  ``lapack_driver`` is accepted and ignored (the SVD is a Jacobi on the
    device).  Returns the ``[n, n]`` filter, a float64 tensor **on the device**, or a NumPy array with
    ``device=False``.

    The filter is real.  The reference returns a complex array, but its modes are symmetric about zero, so ``F F^H`` and
    the projector are real and the imaginary part it carries (2e-9 ... 5e-8 in the cases tried) is the rounding error
    of its complex SVD, not signal.  ``num_modes == 1`` is the exception (one unpaired mode, a genuinely complex
    filter): ``NotImplementedError``.  Mask and window multiply the filter's columns only; the rows of masked samples
    come out zero because the basis is zero there.  ``numpy.linalg.LinAlgError`` if the sweeps do not converge.
    """
    if type_ not in {"high", "low"}:
        raise ValueError(f"Filter type must be one of [high, low]. Got {type_}")
    num_modes = _check_null_modes(num_modes)
    samples = np.ascontiguousarray(samples, dtype=np.float64)
    mask = np.asarray(mask)
    if samples.ndim != 1 or mask.shape != samples.shape:
        raise ValueError(f"null_filter: samples {samples.shape} and mask {mask.shape} must be one-dimensional and alike")
    ctx = Context.get()
    samples_d = ctx.to_device(samples)
    nf, status, _, _ = build_null_filters(ctx, samples_d, [float(cutoff)], num_modes, mask[np.newaxis, :], null_filter_window(samples, window), tol=tol, type_=type_)
    ctx.uses(samples_d)
    if status[0]:
        raise np.linalg.LinAlgError("null_filter: the Jacobi SVD did not converge")
    return nf[0] if device else nf[0].cpu().numpy()
