"""Masked moving median on the GPU (``draco/util/filters.py:99-130``).

``medfilt`` wraps caput's ``moving_weighted_median`` [3P] in the reference; here it is ``dmm_rfi_medfilt``
(``csrc/rfi.hip``) under the conventions of DESIGN.md section 7i: the window is centred on the sample and clipped at
the array's edge, the result is ``0.5 * (v[(n-1)//2] + v[n//2])`` of the ``n`` unmasked samples ``v`` of the window in
ascending order and NaN for an empty window.  Window sizes are odd.  Only 0/1 weights exist: a sample is masked or not.
"""

from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..device import Context, ptr


def check_size(size, ndim):
    """The window as ``(size_f, size_t)``; ``ValueError`` for an even size or one beyond the kernel's bound."""
    if np.ndim(size) == 0:
        size = (int(size),) * ndim
    size = tuple(int(s) for s in size)
    if len(size) != ndim:
        raise ValueError(f"size {size} does not match a {ndim}-dimensional array")
    if ndim == 1:
        size = (size[0], 1)
    if any(s < 1 or s % 2 == 0 for s in size):
        raise ValueError(f"window sizes must be odd and positive, got {size}")
    if max(size) > _lib.DMM_RFI_MAX_WINDOW or size[0] * size[1] > _lib.DMM_RFI_MAX_STRIP:
        raise ValueError(
            f"window {size} is beyond the supported bound: each size at most {_lib.DMM_RFI_MAX_WINDOW}, "
            f"their product at most {_lib.DMM_RFI_MAX_STRIP}"
        )
    return size


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
