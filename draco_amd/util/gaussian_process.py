"""Gaussian-process regression onto a new set of sample positions (``draco/util/gaussian_process.py``).

Signatures and defaults are the reference's; the arithmetic runs in ``libdraco_amd.so`` (``csrc/gp.hip``).  Per
frequency the reference selects the input samples that have a positive weight in some stack (``mi``) and the output
rows close enough to them (``mt``), truncates the kernel matrix of the selected samples to a band, solves for the
projection ``A = Kstar K^-1`` and applies it to every stack.  Here the host decides the two selections and the band
height ``M`` in float64 with NumPy, groups the frequencies by ``(mi, mt)`` -- a group shares one factorisation, and a
frequency's result does not depend on the groups beside it -- and the device does the rest:

    fill (``dmm_gp_fill``, or matrices from the caller) -> projection (``dmm_gp_project``, ``dmm_gp_compact``) -> apply
    (``dmm_gp_apply``).

:func:`resample` and :func:`interpolate_unweighted` take ``[freq, time, stack]`` arrays like the reference and return
device tensors ``[freq, nout, stack]``; :func:`resample_device` is the form the regridder task uses, on ``[freq, stack,
time]`` device tensors without a transposed copy.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.linalg as la

from . import kernels

BAND_TOL = 1.0e-8  # of the band of K and of the band edges of A
WORKSPACE_BYTES = 8 << 30  # band and right-hand sides of the groups of one pass


# ------------------------------------------------------------------------------------------------------ kernel specs
def _build_gp_kernels_from_spec(samples, kernel_spec):
    """``(Ki, Ks)`` of one spec dict: ``Ki = k(samples[1], samples[1])`` with ``epsilon`` on its diagonal and ``Ks =
    k(samples[0], samples[1])``.  ``width`` is in units of the spacing of ``samples[0]`` (or of the integer it is)."""
    spec = dict(kernel_spec)
    xo = samples[0]
    if isinstance(xo, np.ndarray):
        dx = np.median(np.abs(np.diff(xo)))
    elif isinstance(xo, int):
        dx = xo
    else:
        raise TypeError(f"Invalid type for `samples`. Expected `int` or `np.ndarray, got {type(xo)}.")
    width = spec.pop("width", 1.0) * dx
    name = spec.pop("name", "gaussian")
    epsilon = spec.pop("epsilon", 0.0)
    Ki = kernels.get_kernel(name=name, N=samples[1], width=width, **spec)
    Ki[np.diag_indices_from(Ki)] += epsilon
    Ks = kernels.get_kernel(name=name, N=samples, width=width, **spec)
    return Ki.astype(np.float64, copy=False), Ks.astype(np.float64, copy=False)


def _split_specs(kernel_params):
    """``(specs without epsilon, the sum of their epsilons)``; the caller's dicts are left as they are."""
    if not isinstance(kernel_params, list | tuple):
        kernel_params = [kernel_params]
    specs, epsilon = [], 0.0
    for kspec in kernel_params:
        spec = dict(kspec)
        epsilon += spec.pop("epsilon", 0.0)
        specs.append(spec)
    return specs, epsilon


def _combine_gp_kernels_from_specs(samples, kernel_params):
    """The element-wise product of the kernels of several specs; their ``epsilon`` are summed and added once to the
    diagonal of ``Ki``."""
    specs, epsilon = _split_specs(kernel_params)
    Ki = Ks = None
    for spec in specs:
        ki, ks = _build_gp_kernels_from_spec(samples, spec)
        if Ki is None:
            Ki, Ks = ki, ks
        else:
            Ki *= ki
            Ks *= ks
    if Ki is not None:
        Ki[np.diag_indices_from(Ki)] += np.zeros(Ki.shape[0], dtype=Ki.dtype) + epsilon
    return Ki, Ks


def _device_specs(specs, dx):
    """``(types int32 [nspec], params float64 [nspec, 3], pair functions)`` of specs the device evaluates."""
    from .. import _lib

    types, params, pairs = [], [], []
    for spec in specs:
        spec = dict(spec)
        name = spec.pop("name", "gaussian").lower()
        width = spec.pop("width", 1.0) * dx
        spec.pop("epsilon", None)
        if name not in kernels.DEVICE_KERNELS:
            if name in ("periodic", "moving_average"):
                raise NotImplementedError(f"the '{name}' kernel is not evaluated on the device; pass matrices to interpolate_unweighted")
            raise ValueError(f"Invalid kernel type: '{name}'.")
        alpha = spec["alpha"]
        if name == "gaussian":
            t, p = _lib.DMM_GP_GAUSSIAN, 0.0
        elif name == "rational":
            t, p = _lib.DMM_GP_RATIONAL, float(spec["a"])
        else:
            if spec["nu"] not in {1.5, 2.5}:
                raise ValueError(f"Invalid value `nu`={spec['nu']}. Only values of (1.5, 2.5) are currently supported.")
            t, p = (_lib.DMM_GP_MATERN15 if spec["nu"] == 1.5 else _lib.DMM_GP_MATERN25), 0.0
        types.append(t)
        params.append((float(width), float(alpha), p))
        pairs.append((name, float(width), alpha, {k: v for k, v in spec.items() if k != "alpha"}))
    return np.array(types, dtype=np.int32), np.array(params, dtype=np.float64).reshape(-1, 3), pairs


def _pair_product(pairs, a, b):
    out = None
    for name, width, alpha, extra in pairs:
        k = kernels.pair_kernel(name, a, b, width, alpha, **extra)
        out = k if out is None else out * k
    return out


def _band_rows_from_positions(x, pairs, epsilon, tol=BAND_TOL):
    """``kernels.band_rows`` of the kernel matrix of the positions ``x`` without forming it.

    The kernels fall with distance, so the entries of row ``i`` above ``tol`` are one run around the diagonal: its two
    ends are bracketed by a sorted search at the distance where the kernel crosses ``tol`` and then settled with the
    kernel values themselves, which are the values the matrix would hold.
    """
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if n == 0:
        return 1
    if np.any(np.diff(x) < 0):  # no order to search in: rows of the matrix in blocks
        count = np.zeros(n, dtype=np.int64)
        for i0 in range(0, n, 256):
            blk = _pair_product(pairs, x[i0 : i0 + 256, None], x[None, :])
            blk[np.arange(blk.shape[0]), np.arange(i0, i0 + blk.shape[0])] += epsilon
            count[i0 : i0 + 256] = np.sum(blk > tol, axis=-1)
        return int(count.max() // 2 + 1)
    span = max(float(x[-1] - x[0]), np.finfo(np.float64).tiny)
    lo_r, hi_r = 0.0, span
    if _pair_product(pairs, np.array([0.0]), np.array([span]))[0] > tol:
        lo_r = span
    else:
        for _ in range(64):
            mid = 0.5 * (lo_r + hi_r)
            if _pair_product(pairs, np.array([0.0]), np.array([mid]))[0] > tol:
                lo_r = mid
            else:
                hi_r = mid
    ii = np.arange(n)
    above = lambda j: _pair_product(pairs, x, x[np.clip(j, 0, n - 1)]) > tol  # noqa: E731
    hi = np.maximum(np.searchsorted(x, x + lo_r, side="right"), ii + 1)  # entries (i, hi) are above tol
    lo = np.minimum(np.searchsorted(x, x - lo_r, side="left"), ii)  # entries [lo, i) are
    for _ in range(n):
        grow = (hi < n) & above(hi)
        shrink = ~grow & (hi - 1 > ii) & ~above(hi - 1)
        if not (grow.any() or shrink.any()):
            break
        hi = hi + grow - shrink
    for _ in range(n):
        grow = (lo > 0) & above(lo - 1)
        shrink = ~grow & (lo < ii) & ~above(lo)
        if not (grow.any() or shrink.any()):
            break
        lo = lo - grow + shrink
    diag = (_pair_product(pairs, x, x) + epsilon) > tol
    count = (ii - lo) + (hi - ii - 1) + diag
    return int(count.max() // 2 + 1)


# --------------------------------------------------------------------------------------------------- row selection
def _select_interp_samples(xi, xo, mask, kwidth, cutoff, partition=0):
    """Which output samples to interpolate onto, ``[mask.shape[0], len(xo)]`` bool.

    Distances are in units of the median input spacing.  An output sample is kept if it has an unflagged input sample
    strictly on either side closer than ``kwidth - 1``, and if its ``partition``-th nearest (counted from 0) unflagged
    input sample is closer than ``cutoff``.  The booleans are those of the full distance table; the nearest samples are
    found by sorted searches, and the distance ``(xo - xi) / spacing`` of a pair is the table's own expression.
    """
    xi = np.asarray(xi)
    xo = np.asarray(xo)
    mask = np.asarray(mask, dtype=bool)
    med = np.median(np.abs(np.diff(xi)))
    kw_cutoff = kwidth - 1
    out = np.empty((mask.shape[0], xo.shape[0]), dtype=bool)
    done = {}
    for ii in range(mask.shape[0]):
        mi = mask[ii]
        if not np.any(mi):
            out[ii] = False
            continue
        key = mi.tobytes()
        if key in done:
            out[ii] = out[done[key]]
            continue
        done[key] = ii
        xm = np.sort(xi[mi])
        nm = len(xm)
        if partition >= nm or partition < -nm:
            raise ValueError(f"kth(={partition}) out of bounds ({nm})")
        dist = lambda idx: (xo - xm[np.clip(idx, 0, nm - 1)]) / med  # noqa: E731
        below = np.searchsorted(xm, xo, side="left")  # samples [0, below) lie strictly below the output sample
        above = np.searchsorted(xm, xo, side="right")  # samples [above, nm) strictly above
        pdist = np.where(below > 0, np.minimum(dist(below - 1), kw_cutoff), kw_cutoff)
        ndist = np.where(above < nm, np.maximum(dist(above), -kw_cutoff), -kw_cutoff)
        keep = np.maximum(pdist, np.abs(ndist)) < kw_cutoff
        # the partition-th smallest |distance|: it is among the partition + 1 samples on either side
        kth = partition % nm
        offs = np.arange(-(kth + 1), kth + 1)
        cand = below[:, None] + offs[None, :]
        dc = np.abs((xo[:, None] - xm[np.clip(cand, 0, nm - 1)]) / med)
        dc[(cand < 0) | (cand >= nm)] = np.inf
        out[ii] = keep & (np.partition(dc, kth, axis=-1)[:, kth] < cutoff)
    return out


# ------------------------------------------------------------------------------------------------------ device chain
def _dev(ctx, a, dtype):
    return ctx.to_device(np.ascontiguousarray(a, dtype=dtype))


def sample_masks(ctx, w_d):
    """``(mi, nz [nfreq, nt] bool on the host, rowflag [nfreq nstack] bytes on the device)`` of the weights ``w_d [nfreq,
    nstack, nt]``: any stack with weight > 0, any with weight != 0, any sample of the row with weight > 0."""
    from .. import _lib
    from ..device import ptr

    nfreq, nstack, nt = (int(s) for s in w_d.shape)
    mi = ctx.zeros((nfreq, nt), np.uint8)
    nz = ctx.zeros((nfreq, nt), np.uint8)
    rowflag = ctx.zeros((max(nfreq * nstack, 1),), np.uint8)
    _lib.check(_lib.lib.dmm_gp_masks(ctx.handle, ptr(w_d), nfreq, nstack, nt, ptr(mi), ptr(nz), ptr(rowflag)))
    return mi.cpu().numpy().astype(bool), nz.cpu().numpy().astype(bool), rowflag


class _Timer:
    def __init__(self, ctx, timings):
        self.ctx, self.t = ctx, timings

    def start(self):
        if self.t is not None:
            self.ctx.timer_start()

    def stop(self, key):
        if self.t is not None:
            self.t[key] = self.t.get(key, 0.0) + self.ctx.timer_stop()


def _interpolate(ctx, vis_d, w_d, mi_all, mt_all, rowflag, pad, samples, source, mix=None, timings=None, info=None):
    """The device chain on ``vis_d`` / ``w_d [nfreq, nstack, nt]``: ``(vis, weight) [nfreq, nstack, samples]``, the output
    rows ``pad ... pad + samples``.  ``source``: ``("spec", xi, xo, types, params, pairs, epsilon)`` or
    ``("matrix", K, Kstar)``."""
    from .. import _lib
    from ..device import ptr

    nfreq, nstack, nt = (int(s) for s in vis_d.shape)
    out_vis = ctx.zeros((nfreq, nstack, samples), np.complex64)
    out_w = ctx.zeros((nfreq, nstack, samples), np.float32)
    # ---- frequencies by (input mask, kept rows)
    groups, members = {}, []
    for ii in range(nfreq):
        if not mt_all[ii].any() or not mi_all[ii].any():
            continue
        key = mi_all[ii].tobytes() + mt_all[ii].tobytes()
        if key not in groups:
            groups[key] = len(members)
            members.append([])
        members[groups[key]].append(ii)
    if info is not None:
        info.update(ngroup=len(members), M=[], n=[], nk=[], span=[], span_sum=[], nfreq_of=[])
    if not members or nstack == 0:
        return out_vis, out_w
    idx = [np.flatnonzero(mi_all[m[0]]).astype(np.int32) for m in members]
    kout = [np.flatnonzero(mt_all[m[0]]).astype(np.int32) for m in members]
    if source[0] == "spec":
        _, xi, xo, types, params, pairs, epsilon = source
        M = [_band_rows_from_positions(xi[j], pairs, epsilon) for j in idx]
    else:
        _, K, Kstar = source
        M = [kernels.band_rows(K[j][:, j], BAND_TOL) for j in idx]
    n = [len(j) for j in idx]
    nk = [len(k) for k in kout]
    per_group = [8 * ng * (Mg + 64 * -(-nkg // 64)) for ng, Mg, nkg in zip(n, M, nk)]
    om, fm, di, do = mix if mix is not None else (None, None, None, None)
    tm = _Timer(ctx, timings)
    g0 = 0
    while g0 < len(members):  # passes of groups whose band and right-hand sides fit the workspace
        g1, used = g0, 0
        while g1 < len(members) and (g1 == g0 or used + per_group[g1] <= WORKSPACE_BYTES) and g1 - g0 < 65535:
            used += per_group[g1]
            g1 += 1
        G = g1 - g0
        nmax, Mmax, nkpad = max(n[g0:g1]), max(M[g0:g1]), 64 * -(-max(nk[g0:g1]) // 64)
        dims = np.zeros((G, 4), dtype=np.int32)
        dims[:, 0], dims[:, 1], dims[:, 2] = n[g0:g1], M[g0:g1], nk[g0:g1]
        dims_p = C.c_void_p(dims.ctypes.data)
        dims_d = ctx.zeros((G, 4), np.int32)
        idx_h = np.zeros((G, nmax), dtype=np.int32)
        kout_h = np.zeros((G, nkpad), dtype=np.int32)
        for g in range(G):
            idx_h[g, : n[g0 + g]] = idx[g0 + g]
            kout_h[g, : nk[g0 + g]] = kout[g0 + g]
        if source[0] == "spec":
            pos_h = np.zeros((G, nmax))
            xok_h = np.zeros((G, nkpad))
            for g in range(G):
                pos_h[g, : n[g0 + g]] = xi[idx[g0 + g]]
                xok_h[g, : nk[g0 + g]] = xo[kout[g0 + g]]
            pos_d, xok_d = _dev(ctx, pos_h, np.float64), _dev(ctx, xok_h, np.float64)
            Kb = ctx.empty((G, nmax, Mmax), np.float64)
            Y = ctx.empty((G, nmax, nkpad), np.float64)
            tm.start()
            _lib.check(
                _lib.lib.dmm_gp_fill(
                    ctx.handle, len(types), C.c_void_p(types.ctypes.data), C.c_void_p(params.ctypes.data), float(epsilon), G, dims_p, ptr(dims_d), nmax, Mmax, nkpad,
                    ptr(pos_d), ptr(xok_d), ptr(Kb), ptr(Y)
                )
            )
        else:
            Kb_h = np.zeros((G, nmax, Mmax))
            Y_h = np.zeros((G, nmax, nkpad))
            for g in range(G):
                j, k = idx[g0 + g], kout[g0 + g]
                Kg = np.asarray(K[j][:, j], dtype=np.float64)
                for d in range(M[g0 + g]):
                    Kb_h[g, d : len(j), d] = Kg.diagonal(-d)
                Y_h[g, : len(j), : len(k)] = np.asarray(Kstar[k][:, j], dtype=np.float64).T
            tm.start()
            Kb, Y = _dev(ctx, Kb_h, np.float64), _dev(ctx, Y_h, np.float64)
        tm.stop("fill_ms")
        status = ctx.zeros((G,), np.int32)
        start = ctx.zeros((G, nkpad), np.int32)
        end = ctx.zeros((G, nkpad), np.int32)
        tm.start()
        _lib.check(_lib.lib.dmm_gp_project(ctx.handle, G, dims_p, ptr(dims_d), nmax, Mmax, nkpad, ptr(Kb), ptr(Y), BAND_TOL, ptr(status), ptr(start), ptr(end)))
        status_h = status.cpu().numpy()
        if np.any(status_h != _lib.DMM_GP_OK):
            ctx.sync()
            bad_g = min(np.flatnonzero(status_h != _lib.DMM_GP_OK), key=lambda g: members[g0 + g][0])
            raise la.LinAlgError(
                f"The band-truncated kernel matrix of frequency index {members[g0 + bad_g][0]} (order {n[g0 + bad_g]}, {M[g0 + bad_g]} band rows) is not positive "
                "definite; a larger `epsilon` on the diagonal of `K` usually resolves this."
            )
        span = (end - start).amax(dim=1).cpu().numpy()
        W = max(int(span.max()), 1)
        Ac = ctx.empty((G, W, nkpad), np.float64)
        _lib.check(_lib.lib.dmm_gp_compact(ctx.handle, G, dims_p, ptr(dims_d), nmax, nkpad, W, ptr(Y), ptr(start), ptr(end), ptr(Ac)))
        tm.stop("project_ms")
        fgroup = np.full(nfreq, -1, dtype=np.int32)
        for g in range(G):
            fgroup[members[g0 + g]] = g
        fgroup_d, idx_d, kout_d = _dev(ctx, fgroup, np.int32), _dev(ctx, idx_h, np.int32), _dev(ctx, kout_h, np.int32)
        tm.start()
        _lib.check(
            _lib.lib.dmm_gp_apply(
                ctx.handle, nfreq, nstack, nt, int(samples), int(pad), G, dims_p, ptr(dims_d), nmax, nkpad, W, ptr(fgroup_d), ptr(idx_d), ptr(kout_d), ptr(start), ptr(end),
                ptr(Ac), ptr(rowflag), ptr(vis_d), ptr(w_d), ptr(om), ptr(fm), ptr(di), ptr(do), ptr(out_vis), ptr(out_w)
            )
        )
        tm.stop("apply_ms")
        ctx.sync()  # the pass's tables go out of scope below
        if info is not None:
            info["M"] += M[g0:g1]
            info["n"] += n[g0:g1]
            info["nk"] += nk[g0:g1]
            info["span"] += [int(s) for s in span]
            info["span_sum"] += [int(s) for s in (end - start).sum(dim=1).cpu().numpy()]
            info["nfreq_of"] += [len(m) for m in members[g0:g1]]
            if info.get("keep_projection"):  # (tests: the compact projection of every group of the pass, on the host)
                info.setdefault("projection", []).append({"members": members[g0:g1], "rows": kout[g0:g1], "n": n[g0:g1], "start": start.cpu().numpy(), "end": end.cpu().numpy(), "A": Ac.cpu().numpy()})
        g0 = g1
    return out_vis, out_w


def resample_device(ctx, vis_d, w_d, xi, xo, cutoff_dist=1.0, cutoff_partition=0, kernel_spec={}, pad=0, samples=None, mix=None, timings=None, info=None):
    """:func:`resample` on ``[nfreq, nstack, nt]`` device tensors (complex64, float32): ``(vis, weight) [nfreq, nstack,
    samples]`` device tensors, the output samples ``pad ... pad + samples`` of ``xo`` (all of them by default).

    ``mix``: ``None`` or ``(omega [nfreq nstack] f64, feed_mask [nfreq nstack] f32, dphi_in [nt] f64, dphi_out [samples]
    f64)`` device tensors, the mix-down and mix-up of ``SiderealRegridder`` fused into the load and the store.
    ``timings``: a dict that receives ``fill_ms`` / ``project_ms`` / ``apply_ms`` (device time; it serialises the stages).
    """
    xi = np.asarray(xi, dtype=np.float64)
    xo = np.asarray(xo, dtype=np.float64)
    samples = len(xo) - 2 * pad if samples is None else int(samples)
    specs, epsilon = _split_specs(kernel_spec)
    types, params, pairs = _device_specs(specs, np.median(np.abs(np.diff(xo))))
    kwidth = 0.0
    for spec in specs:
        kwidth = max(kwidth, spec.get("width", 0.0))
    mi_all, nz_all, rowflag = sample_masks(ctx, w_d)
    mt_all = _select_interp_samples(xi, xo, nz_all, kwidth, cutoff_dist, cutoff_partition)
    return _interpolate(ctx, vis_d, w_d, mi_all, mt_all, rowflag, pad, samples, ("spec", xi, xo, types, params, pairs, epsilon), mix, timings, info)


def _to_device_layout(ctx, data, weight):
    """``[freq, time, stack]`` arrays -> ``[freq, stack, time]`` contiguous complex64 / float32 device tensors."""
    import torch

    data = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.asarray(data))
    weight = weight if isinstance(weight, torch.Tensor) else torch.from_numpy(np.asarray(weight))
    if not data.is_complex():
        data = data.to(torch.complex64)
    weight = torch.broadcast_to(weight, data.shape)
    vis_d = data.to(ctx.device).to(torch.complex64).permute(0, 2, 1).contiguous()
    w_d = weight.to(ctx.device).to(torch.float32).permute(0, 2, 1).contiguous()
    return vis_d, w_d


def resample(data, weight, xi, xo, cutoff_dist=1.0, cutoff_partition=0, kernel_spec={}):
    """Resample a dataset with a GP kernel given as one spec dict or a list of them (their kernels are multiplied).

    ``data [freq, time, stack]`` (complex64; the stacks share ``weight``'s masking), ``weight`` broadcastable to it,
    ``xi`` the positions of the samples and ``xo`` those to interpolate onto.  Output samples further than
    ``cutoff_dist`` input spacings from their ``cutoff_partition``-th nearest unflagged input sample are left zero.
    Returns device tensors ``(xout [freq, len(xo), stack] complex64, wout float32)``.
    """
    from ..device import Context

    ctx = Context.get()
    vis_d, w_d = _to_device_layout(ctx, data, weight)
    xout, wout = resample_device(ctx, vis_d, w_d, xi, xo, cutoff_dist, cutoff_partition, kernel_spec)
    return xout.permute(0, 2, 1), wout.permute(0, 2, 1)


def interpolate_unweighted(data, weight, K, Kstar, interp_samples=None):
    """Interpolate ``data [freq, time, stack]`` with the source kernel ``K [time, time]`` and the projection kernel
    ``Kstar [nout, time]`` (host matrices), assuming the signal is noise free; ``interp_samples [freq, nout]`` bool
    restricts the output rows (the others stay zero).  Returns device tensors ``(xout [freq, nout, stack], wout)``.

    Raises ``scipy.linalg.LinAlgError`` if the band-truncated ``K`` of a frequency's samples is not positive definite.
    """
    from ..device import Context

    ctx = Context.get()
    vis_d, w_d = _to_device_layout(ctx, data, weight)
    K, Kstar = np.asarray(K), np.asarray(Kstar)
    nout = Kstar.shape[0]
    mi_all, _, rowflag = sample_masks(ctx, w_d)
    if interp_samples is None:
        mt_all = np.ones((vis_d.shape[0], nout), dtype=bool)
    else:
        mt_all = np.stack([np.ones(nout, dtype=bool) if isinstance(m, slice) else np.asarray(m, dtype=bool) for m in interp_samples])
    xout, wout = _interpolate(ctx, vis_d, w_d, mi_all, mt_all, rowflag, 0, nout, ("matrix", K, Kstar))
    return xout.permute(0, 2, 1), wout.permute(0, 2, 1)
