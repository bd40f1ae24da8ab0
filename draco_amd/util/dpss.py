"""DPSS (discrete prolate spheroidal sequence) inpainting on the GPU.

Drop-in for ``draco/util/dpss.py``:

* :func:`make_covariance`, :func:`get_basis`   ``dpss.py:9-118``  on the **host**, exactly as the reference (one
  ``scipy.linalg.eigh(driver="evd")`` per distinct cut of a run: setup work, not per-sample work);
* :func:`project`, :func:`solve`, :func:`filter`, :func:`inpaint`, :func:`accumulate_variance`,
  :func:`flag_above_cutoff`   ``dpss.py:121-443``  on the **device** (``csrc/dpss.hip``): they take device tensors
  (NumPy input is uploaded) and return device tensors.  As in the reference the first axis is the interpolation axis,
  the second the independent columns, and the basis ``A [n, k]`` is explicit.

Arithmetic: per column in float64, rounded once to ``complex64`` / ``float32`` (the reference works in float32 from
``Ni.astype(A.dtype)`` on).  The variance diagonal of ``F N F^H`` is formed as ``a_i . y_i - Si |y_i|^2`` with ``y_i =
C^-1 a_i``: ``O(k^2 n)`` per column instead of the reference's ``O(k n^2)`` einsum (``Ni inz(Ni) Ni = Ni``).

A non-zero centre makes the basis complex: the device functions raise ``NotImplementedError`` for it.  The order ``n``
is 1 ... 4096 and the mode count ``k`` 1 ... ``n`` (``ValueError`` otherwise).  A column whose matrix is not positive
definite raises ``numpy.linalg.LinAlgError`` here (the reference's ``cho_factor`` does); the tasks of
``draco_amd.analysis.interpolate`` keep such a column's data, zero its weight and log an error instead.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..device import Context, ptr

MAX_ORDER = 4096
MAX_BATCH = 65535


# ---------------------------------------------------------------------------------------------------------- host side
def make_covariance(samples, halfwidths, centres):
    """Signal covariance of a sum of top-hats in the Fourier inverse of ``samples`` (``dpss.py:9-64``).

    Real if every centre is zero, complex otherwise.
    """
    if np.isscalar(halfwidths):
        halfwidths = [halfwidths]
    if np.isscalar(centres):
        centres = [centres]
    if len(centres) != len(halfwidths):
        raise ValueError(f"`halfwidths` and `centres` must be the same length. Got halfwidths={halfwidths}, centres={centres}")
    ds = np.subtract.outer(samples, samples)
    cov = np.zeros(ds.shape, dtype=np.complex128)
    for ct, hw in zip(centres, halfwidths):
        cov += np.exp(-2.0j * np.pi * ct * ds) * np.sinc(2.0 * hw * ds)
    if np.isreal(cov).all():
        cov = np.ascontiguousarray(cov.real)
    return cov


def get_basis(cov, threshold=1e-12, dtype=np.float32):
    """The eigenvectors of ``cov`` whose eigenvalue exceeds ``threshold`` times the largest, by decreasing eigenvalue,
    cast to ``dtype`` after the cut (``dpss.py:67-118``).  Host LAPACK, as the reference."""
    import scipy.linalg as la

    evals, evecs = la.eigh(cov, check_finite=False, driver="evd")
    idx = np.argsort(evals)[::-1]
    evals = evals[idx]
    evecs = evecs[:, idx]
    nmodes = (evals > threshold * evals.max()).sum()
    real = np.dtype(dtype).type(0).real.dtype
    if np.iscomplexobj(evecs):
        real = np.dtype({"float32": np.complex64, "float64": np.complex128}[real.name])
    return evecs[:, :nmodes].astype(real)


# -------------------------------------------------------------------------------------------------------- device side
class DeviceBasis:
    """``A [n, k]`` and its transpose as float64 device tensors."""

    def __init__(self, ctx, A, who="dpss"):
        if isinstance(A, torch.Tensor):
            if A.is_complex():
                raise NotImplementedError(f"{who}: a complex basis (non-zero centres) is not on the GPU path")
            A = A.to(ctx.device, torch.float64)
        else:
            A = np.asarray(A)
            if np.iscomplexobj(A):
                raise NotImplementedError(f"{who}: a complex basis (non-zero centres) is not on the GPU path")
            A = ctx.to_device(A, np.float64)
        if A.ndim != 2:
            raise ValueError(f"{who}: the basis must be [n, k], got {tuple(A.shape)}")
        self.n, self.k = int(A.shape[0]), int(A.shape[1])
        if not 1 <= self.n <= MAX_ORDER:
            raise ValueError(f"{who}: {self.n} samples, the kernels take 1 ... {MAX_ORDER}")
        if not 1 <= self.k <= self.n:
            raise ValueError(f"{who}: {self.k} modes for {self.n} samples, the kernels take 1 ... n")
        self.A = A.contiguous()
        self.At = self.A.t().contiguous()


def _basis(ctx, A, who):
    return A if isinstance(A, DeviceBasis) else DeviceBasis(ctx, A, who)


def batch_columns(n, k, workspace_mib):
    """Columns per batch: ``C`` takes ``8 k^2`` bytes per column, the variance right-hand sides ``8 k n``, the packed
    rows about ``64 n + 32 k``."""
    per = 8 * k * k + 8 * k * n + 64 * n + 32 * k + 64
    return int(max(1, min(MAX_BATCH, (int(workspace_mib) << 20) // per)))


class _Timer:
    """Accumulates the device time of named stages (``tools/dpss_timing.py``); each stage is synchronised."""

    def __init__(self, ctx, into):
        self.ctx, self.into = ctx, into

    def __call__(self, name, fn):
        if self.into is None:
            return fn()
        self.ctx.timer_start()
        fn()
        self.into[name] = self.into.get(name, 0.0) + self.ctx.timer_stop()


def _layout(ninner, stride_outer, stride_inner, stride_samp):
    return (C.c_int64 * 4)(int(ninner), int(stride_outer), int(stride_inner), int(stride_samp))


def _core(ctx, basis, Si, Ni, W, status, timer, X=None, xhat=None, B=None):
    """Gram, projection, factorisation, solves, synthesis and PCHIP on packed rows; returns ``(F, wout)``.  Either the
    packed data ``X`` with its mean ``xhat`` is given and projected, or the projected data ``B [nb][2][k]`` itself."""
    lib = _lib.lib
    n, k, nb = basis.n, basis.k, int(Ni.shape[0])
    Cm = ctx.empty((nb, k, k), np.float64)
    Z = ctx.empty((nb, n, k), np.float64)
    F = ctx.empty((nb, 2, n), np.float64)
    var = ctx.zeros((nb, n), np.float64)
    wout = ctx.empty((nb, n), np.float64)
    timer("gram", lambda: _lib.check(lib.dmm_dpss_gram(ctx.handle, n, k, nb, ptr(basis.A), ptr(Ni), float(Si), ptr(Cm), ptr(status))))
    if B is None:
        B = ctx.empty((nb, 2, k), np.float64)
        timer("project", lambda: _lib.check(lib.dmm_dpss_project(ctx.handle, n, k, nb, ptr(basis.A), ptr(X), ptr(Ni), ptr(xhat), ptr(B))))
    timer("factor", lambda: _lib.check(lib.dmm_dpss_solve(ctx.handle, k, nb, ptr(Cm), ptr(B), ptr(status))))
    timer("variance", lambda: _lib.check(lib.dmm_dpss_variance(ctx.handle, n, k, nb, ptr(basis.A), ptr(Cm), float(Si), ptr(Z), ptr(var), ptr(status))))
    timer("synth", lambda: _lib.check(lib.dmm_dpss_synth(ctx.handle, n, k, nb, ptr(basis.At), ptr(B), ptr(F))))
    timer("pchip", lambda: _lib.check(lib.dmm_dpss_pchip(ctx.handle, n, nb, ptr(Ni), ptr(W), ptr(var), ptr(status), ptr(wout))))
    ctx.uses(Cm, Z, B, var)
    return F, wout


def run_columns(ctx, basis, Si, layout, cols, vis_in, weight_in, wext, vis_out, weight_out, inpaint, fc=None, workspace_mib=1024, timings=None):
    """Filter the columns ``cols`` (host int64) of a stream through one basis, batch by batch.

    ``layout = (ninner, stride_outer, stride_inner, stride_samp)`` addresses the columns of ``vis_in`` / ``weight_in``
    (complex64 / float32 device tensors) and of the outputs alike, see ``include/draco_amd.h``.  ``wext``: the mask as
    a ``uint8`` tensor of the weights' layout, or ``None`` (``W = weight > 0``).  ``fc``: the gap cutoff in samples, or
    ``None``.  Returns the columns whose matrix was not positive definite (their data is copied through, their weight
    is zero).
    """
    lib = _lib.lib
    n = basis.n
    cols = np.ascontiguousarray(cols, dtype=np.int64)
    lay = _layout(*layout)
    per = batch_columns(n, basis.k, workspace_mib)
    timer = _Timer(ctx, timings)
    failed = []
    for c0 in range(0, cols.size, per):
        sel = cols[c0 : c0 + per]
        nb = int(sel.size)
        cols_d = ctx.to_device(sel)
        X = ctx.empty((nb, 2, n), np.float64)
        Ni = ctx.empty((nb, n), np.float64)
        W = ctx.empty((nb, n), np.uint8)
        xhat = ctx.empty((nb, 2), np.float64)
        status = ctx.empty((nb,), np.int32)
        timer("pack", lambda: _lib.check(lib.dmm_dpss_pack(ctx.handle, n, nb, lay, ptr(cols_d), ptr(vis_in), ptr(weight_in), ptr(wext), ptr(X), ptr(Ni), ptr(W), ptr(xhat), ptr(status))))
        F, wout = _core(ctx, basis, Si, Ni, W, status, timer, X=X, xhat=xhat)
        keep = None
        if fc is not None:
            keep = ctx.empty((nb, n), np.uint8)
            valid = W if wext is None else (Ni > 0).to(torch.uint8)
            timer("gapflag", lambda: _lib.check(lib.dmm_dpss_gapflag(ctx.handle, n, nb, ptr(valid), float(np.float32(fc)), ptr(keep))))
            ctx.uses(valid)
        timer("store", lambda: _lib.check(lib.dmm_dpss_store(ctx.handle, n, nb, lay, ptr(cols_d), ptr(F), ptr(xhat), ptr(X), ptr(Ni), ptr(W), ptr(wout), ptr(keep), ptr(status), int(bool(inpaint)), ptr(vis_out), ptr(weight_out))))
        st = status.cpu().numpy()
        failed.extend(sel[st == _lib.DMM_DPSS_NOT_POSDEF].tolist())
        ctx.uses(cols_d, X, Ni, W, xhat, status, F, wout, keep)
    return np.asarray(failed, dtype=np.int64)


def _as_2d(ctx, x, dtype):
    """Device tensor ``[n, ncol]`` of ``dtype`` and whether the input had one axis."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    one = t.ndim == 1
    if one:
        t = t[:, None]
    if t.ndim != 2:
        raise ValueError(f"dpss: expected [n] or [n, ncol], got {tuple(t.shape)}")
    return t.to(ctx.device).to(dtype).contiguous(), one


def _check_rows(who, basis, *ts):
    for t in ts:
        if int(t.shape[0]) != basis.n:
            raise ValueError(f"Shape mismatch. x: {tuple(t.shape)}, A: {(basis.n, basis.k)}.")


def _raise_failed(who, status):
    bad = np.flatnonzero(status.cpu().numpy() == _lib.DMM_DPSS_NOT_POSDEF)
    if bad.size:
        raise np.linalg.LinAlgError(f"{who}: the matrix of column {int(bad[0])} is not positive definite")


def _chunks(ncol):
    return [(c0, min(ncol, c0 + MAX_BATCH)) for c0 in range(0, ncol, MAX_BATCH)]


def project(x, Ni, A):
    """Noise-weighted data projected into the basis, ``A^T (Ni x)`` (``dpss.py:121-151``): ``[k, ncol]`` complex128 on
    the device."""
    ctx = Context.get()
    basis = _basis(ctx, A, "project")
    xt, one = _as_2d(ctx, x, torch.complex128)
    nt, _ = _as_2d(ctx, Ni, torch.float64)
    _check_rows("project", basis, xt, nt)
    ncol = int(xt.shape[1])
    out = torch.empty((basis.k, ncol), dtype=torch.complex128, device=ctx.device)
    for c0, c1 in _chunks(ncol):
        X = torch.stack([xt[:, c0:c1].real.t(), xt[:, c0:c1].imag.t()], dim=1).contiguous()
        Np = nt[:, c0:c1].t().contiguous()
        B = ctx.empty((c1 - c0, 2, basis.k), np.float64)
        zero = ctx.zeros((c1 - c0, 2), np.float64)
        _lib.check(_lib.lib.dmm_dpss_project(ctx.handle, basis.n, basis.k, c1 - c0, ptr(basis.A), ptr(X), ptr(Np), ptr(zero), ptr(B)))
        out[:, c0:c1] = torch.complex(B[:, 0, :], B[:, 1, :]).t()
        ctx.uses(X, Np, B, zero)
    return out[:, 0] if one else out


def solve(xp, Ni, A, Si=1e-3):
    """Apply the inpainting operator to projected data (``dpss.py:154-251``).

    Returns ``(xinp, winp)``: ``A C^-1 xp`` as complex64 and the inverse of the diagonal of the uncertainty matrix as
    float32, ``[n, ncol]`` on the device.  A column whose ``Ni`` is all zero is not solved: its data is zero and its
    weight stays zero.
    """
    ctx = Context.get()
    basis = _basis(ctx, A, "solve")
    xt, one = _as_2d(ctx, xp, torch.complex128)
    nt, _ = _as_2d(ctx, Ni, torch.float64)
    _check_rows("solve", basis, nt)
    if int(xt.shape[0]) != basis.k:
        raise ValueError(f"Shape mismatch. x: {tuple(xt.shape)}, A: {(basis.k, basis.n)}.")
    ncol = int(nt.shape[1])
    xo = torch.empty((basis.n, ncol), dtype=torch.complex64, device=ctx.device)
    wo = torch.empty((basis.n, ncol), dtype=torch.float32, device=ctx.device)
    timer = _Timer(ctx, None)
    for c0, c1 in _chunks(ncol):
        nb = c1 - c0
        Np = nt[:, c0:c1].t().contiguous()
        B = torch.stack([xt[:, c0:c1].real.t(), xt[:, c0:c1].imag.t()], dim=1).contiguous()
        status = torch.where((Np != 0).any(dim=1), _lib.DMM_DPSS_OK, _lib.DMM_DPSS_SKIPPED).to(torch.int32).contiguous()
        B[status != 0] = 0.0
        W = ctx.zeros((nb, basis.n), np.uint8)  # no knots: the PCHIP stage is inz(var) alone
        F, wout = _core(ctx, basis, Si, Np, W, status, timer, B=B)
        _raise_failed("solve", status)
        xo[:, c0:c1] = torch.complex(F[:, 0, :], F[:, 1, :]).t().to(torch.complex64)
        wo[:, c0:c1] = wout.t().to(torch.float32)
        ctx.uses(Np, B, status, W, F, wout)
    return (xo[:, 0], wo[:, 0]) if one else (xo, wo)


def accumulate_variance(wo, wi, W):
    """PCHIP-interpolate the variance of the non-inpainted weights ``wo`` through the samples where ``W`` is set and
    add it to the variance of the inpainted weights ``wi`` (``dpss.py:254-304``); float32 ``[n, ncol]`` on the device."""
    ctx = Context.get()
    wot, one = _as_2d(ctx, wo, torch.float64)
    wit, _ = _as_2d(ctx, wi, torch.float64)
    Wt, _ = _as_2d(ctx, W, torch.uint8)
    n, ncol = int(wot.shape[0]), int(wot.shape[1])
    if not 1 <= n <= MAX_ORDER:
        raise ValueError(f"accumulate_variance: {n} samples, the kernels take 1 ... {MAX_ORDER}")
    Np, Wp = wot.t().contiguous(), Wt.t().contiguous()
    vi = wit.t().contiguous()
    var = torch.where(vi != 0, 1.0 / torch.where(vi != 0, vi, torch.ones_like(vi)), torch.zeros_like(vi))  # invert_no_zero
    status = ctx.zeros((ncol,), np.int32)
    wout = ctx.empty((ncol, n), np.float64)
    _lib.check(_lib.lib.dmm_dpss_pchip(ctx.handle, n, ncol, ptr(Np), ptr(Wp), ptr(var), ptr(status), ptr(wout)))
    out = wout.t().to(torch.float32).contiguous()
    ctx.uses(Np, Wp, var, status, wout)
    return out[:, 0] if one else out


def flag_above_cutoff(W, fc=None):
    """Mask that is False in the gaps of ``W`` (along the first axis) wider than the cutoff ``fc`` in samples
    (``dpss.py:307-356``), with the reference's edge rules: a gap from ``ri`` to ``fi`` is kept where ``fi - ri < fc``
    (its width minus one); everything before the first valid sample is flagged, and everything from the last valid
    sample on, that sample included.  ``fc=None`` returns ``W``.  Bool ``[n, ncol]`` on the device."""
    ctx = Context.get()
    Wt, one = _as_2d(ctx, W, torch.uint8)
    if fc is None:
        out = Wt.to(torch.bool)
        return out[:, 0] if one else out
    n, ncol = int(Wt.shape[0]), int(Wt.shape[1])
    if not 1 <= n <= MAX_ORDER:
        raise ValueError(f"flag_above_cutoff: {n} samples, the kernels take 1 ... {MAX_ORDER}")
    valid = Wt.t().contiguous()
    keep = ctx.empty((ncol, n), np.uint8)
    _lib.check(_lib.lib.dmm_dpss_gapflag(ctx.handle, n, ncol, ptr(valid), float(np.float32(fc)), ptr(keep)))
    out = keep.t().to(torch.bool).contiguous()
    ctx.uses(valid, keep)
    return out[:, 0] if one else out


def _filter(who, x, Ni, A, W, Si, put_back):
    ctx = Context.get()
    basis = _basis(ctx, A, who)
    xt, one = _as_2d(ctx, x, torch.complex64)
    nt, _ = _as_2d(ctx, Ni, torch.float32)
    Wt, _ = _as_2d(ctx, W, torch.uint8)
    _check_rows(who, basis, xt, nt, Wt)
    ncol = int(xt.shape[1])
    xo, wo = torch.empty_like(xt), torch.empty_like(nt)
    failed = run_columns(ctx, basis, Si, (ncol, 0, 1, ncol), np.arange(ncol), xt, nt, Wt, xo, wo, put_back)
    if failed.size:
        raise np.linalg.LinAlgError(f"{who}: the matrix of column {int(failed[0])} is not positive definite")
    ctx.uses(xt, nt, Wt)
    return (xo[:, 0], wo[:, 0]) if one else (xo, wo)


def filter(x, Ni, A, W, Si=1e-3):  # noqa: A001  (the reference's name)
    """Filter with a DPSS basis over the first axis (``dpss.py:359-404``): ``(xfilt, wfilt)``, complex64 / float32
    ``[n, ncol]`` on the device.  The mean over the samples where ``W`` is set is removed first and added back."""
    return _filter("filter", x, Ni, A, W, Si, False)


def inpaint(x, Ni, A, W, Si=1e-3):
    """Inpaint with a DPSS basis over the first axis (``dpss.py:407-443``): as :func:`filter`, but the samples where
    ``W`` is set keep the input's data and weight, bit for bit."""
    return _filter("inpaint", x, Ni, A, W, Si, True)


__all__ = ["accumulate_variance", "filter", "flag_above_cutoff", "get_basis", "inpaint", "make_covariance", "project", "solve"]
