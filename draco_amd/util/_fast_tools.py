"""Fringestop and sum over products on the GPU (``draco/util/_fast_tools.pyx:211-290``; ``csrc/srcbeam.hip``).

:func:`beamform` has the reference's argument order and layout and takes one source; :func:`form`, :func:`prepare` and
:func:`collapse` are the chunked stages the tasks of ``draco_amd.analysis.beamform`` drive.  The per-source tables
(``cos`` / ``sin`` of hour angle and declination, which sample every hour-angle slot reads, which frequencies a source
processes) are float64 NumPy on the host, uploaded; every sum is a kernel.  Nothing here waits for the device: the
uploaded tables are torch tensors of the stream the kernels run on (``Context.get()`` follows torch's current stream),
so the allocator hands their memory on only behind the kernels that read them.
"""

from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from ..device import Context, ptr

WEIGHT_MODES = {"inverse_variance": _lib.DMM_SRCBEAM_INVERSE_VARIANCE, "natural": _lib.DMM_SRCBEAM_NATURAL, "uniform": _lib.DMM_SRCBEAM_UNIFORM}


def phase_tables(dec, lat, cosha, sinha):
    """``(ut, vt)`` with the fringestop phase ``2 pi (u ut + v vt)``: ``ut = cos(dec) sin(ha)``,
    ``vt = -(cos(lat) sin(dec) - sin(lat) cos(dec) cos(ha))``; ``dec`` broadcasts against the hour-angle tables."""
    dec = np.asarray(dec, dtype=np.float64)
    cosdec, sindec = np.cos(dec), np.sin(dec)
    coslat, sinlat = np.cos(np.float64(lat)), np.sin(np.float64(lat))
    ut = cosdec * np.asarray(sinha, dtype=np.float64)
    vt = -(coslat * sindec - sinlat * cosdec * np.asarray(cosha, dtype=np.float64))
    return np.ascontiguousarray(ut), np.ascontiguousarray(vt)


def window_pairs(ra_index, nra):
    """Invert the windows ``ra_index [nsrc, nha]`` (sample of every hour-angle slot, negative: no such slot) into the
    list the form kernel walks: ``pair_id`` = ``src * nha + slot`` sorted by sample (sources in one bin keep catalogue
    order) and ``pair_start [nra + 1]``, the first pair of every sample."""
    flat = np.asarray(ra_index, dtype=np.int64).ravel()
    if flat.size and flat.max() >= nra:
        raise ValueError(f"window sample {int(flat.max())} outside an axis of {nra}")
    ids = np.flatnonzero(flat >= 0)
    order = np.argsort(flat[ids], kind="stable")
    pair_id = ids[order].astype(np.int32)
    pair_start = np.searchsorted(flat[pair_id], np.arange(nra + 1)).astype(np.int32)
    return pair_start, pair_id


def prepare(ctx, vis, weight, sel, mode, redundancy=None):
    """One processed polarisation of a dataset: ``vis`` / ``weight [nfreq, nstack, nra]`` device tensors (complex64 /
    float32), ``sel`` the polarisation's stacks, ``redundancy [nstack, nra]`` float32 (array or device tensor) for the natural and uniform modes.
    Returns ``(visT, ws, SW, SW2)``: ``[nfreq, nra, nsel]`` complex64 / float32 and the two float64 sums ``[nfreq, nra]``."""
    nfreq, nstack, nra = (int(s) for s in vis.shape)
    sel = np.ascontiguousarray(sel, dtype=np.int32)
    if sel.size and (sel.min() < 0 or sel.max() >= nstack):
        raise ValueError("stack selection outside the stack axis")
    nsel = int(sel.size)
    sel_d = ctx.to_device(sel) if nsel else None
    red_d = None if redundancy is None else ctx.to_device(redundancy, np.float32)
    if red_d is not None and tuple(red_d.shape) != (nstack, nra):
        raise ValueError(f"redundancy of shape {tuple(red_d.shape)}, expected {(nstack, nra)}")
    visT = ctx.empty((nfreq, nra, nsel), np.complex64)
    ws = ctx.empty((nfreq, nra, nsel), np.float32)
    SW = ctx.empty((nfreq, nra), np.float64)
    SW2 = ctx.empty((nfreq, nra), np.float64)
    _lib.check(_lib.lib.dmm_srcbeam_prepare(ctx.handle, nfreq, nstack, nra, nsel, ptr(sel_d), int(WEIGHT_MODES[mode]), ptr(vis), ptr(weight), ptr(red_d),
                                            ptr(visT) if nsel else None, ptr(ws) if nsel else None, ptr(SW), ptr(SW2)))
    return visT, ws, SW, SW2


def form(ctx, visT, ws, u, v, ut, vt, ra_index, fmask=None, out=None):
    """The hot kernel for a chunk of sources: ``F [nsrc, nfreq, nha]`` float64 on the device.

    ``visT [nfreq, nra, ns]`` complex64 and ``ws`` (float32 or float64) and ``u`` / ``v [nfreq, ns]`` float64 are device
    tensors; ``ut`` / ``vt [nsrc, nha]`` float64, ``ra_index [nsrc, nha]`` int and ``fmask [nsrc, nfreq]`` bool are host
    arrays.  Slots whose ``ra_index`` is negative and frequencies outside ``fmask`` stay zero.  ``out``: a contiguous
    device tensor of that shape to fill instead of a new one."""
    nfreq, nra, ns = (int(s) for s in visT.shape)
    ra_index = np.asarray(ra_index)
    nsrc, nha = (int(s) for s in ra_index.shape)
    if nha > nra:
        raise ValueError(f"a window of {nha} samples is longer than the axis ({nra})")
    F = ctx.empty((nsrc, nfreq, nha), np.float64) if out is None else out
    if tuple(F.shape) != (nsrc, nfreq, nha) or F.dtype != torch.float64 or not F.is_contiguous():
        raise ValueError(f"out of shape {tuple(F.shape)}, expected {(nsrc, nfreq, nha)} float64")
    if nsrc == 0:
        return F
    pair_start, pair_id = window_pairs(ra_index, nra)
    npair = int(pair_id.size)
    ps_d = ctx.to_device(pair_start)
    pi_d = ctx.to_device(pair_id if npair else np.zeros(1, np.int32))
    ut_d, vt_d = ctx.to_device(ut, np.float64), ctx.to_device(vt, np.float64)
    fm_d = None if fmask is None else ctx.to_device(np.asarray(fmask).astype(np.uint8))
    wtype = {torch.float32: _lib.DMM_SRCBEAM_W_F32, torch.float64: _lib.DMM_SRCBEAM_W_F64}[ws.dtype]
    _lib.check(_lib.lib.dmm_srcbeam_form(ctx.handle, nfreq, nra, ns, int(wtype), ptr(visT), ptr(ws), ptr(u), ptr(v), nsrc, nha, ptr(ut_d), ptr(vt_d), ptr(fm_d), npair,
                                         ptr(ps_d), ptr(pi_d), ptr(F)))
    return F


def collapse(ctx, F, pb, SW, SW2, ra_index, fmask, rows, beam, weight, collapse_ha, inverse_variance, stokes_i):
    """Finish a chunk: ``F`` / ``pb [npol, nsrc, nfreq, nha]`` (``pb`` None: ones) and ``SW`` / ``SW2 [npol, nfreq, nra]``
    device tensors, ``ra_index``, ``fmask`` and ``rows`` (output row of every source) host arrays; writes the rows of
    ``beam`` / ``weight`` (``[nobj, npol_out, nfreq]``, with a trailing ``nha`` unless ``collapse_ha``)."""
    npol, nsrc, nfreq, nha = (int(s) for s in F.shape)
    nra = int(SW.shape[-1])
    ri_d = ctx.to_device(np.ascontiguousarray(ra_index, dtype=np.int32))
    fm_d = None if fmask is None else ctx.to_device(np.asarray(fmask).astype(np.uint8))
    rows_d = ctx.to_device(np.ascontiguousarray(rows, dtype=np.int64))
    _lib.check(_lib.lib.dmm_srcbeam_collapse(ctx.handle, nfreq, nra, npol, nsrc, nha, int(bool(collapse_ha)), int(bool(inverse_variance)), int(bool(stokes_i)), ptr(F),
                                             ptr(pb), ptr(SW), ptr(SW2), ptr(ri_d), ptr(fm_d), ptr(rows_d), int(beam.shape[0]), ptr(beam), ptr(weight)))


def beamform(vis, weight, dec, lat, cosha, sinha, u, v, f_index, ra_index):
    """Fringestop visibility data to one source and sum over products (``_fast_tools.pyx:211-290``).

    As in the reference the sum is not normalised.  ``vis [freq, ra, stack]`` complex64, ``weight`` of the same shape
    float64, ``dec`` and ``lat`` in radians, ``cosha`` / ``sinha [ha]``, ``u`` / ``v [freq, stack]`` in wavelengths,
    ``f_index`` the frequencies to process and ``ra_index [ha]`` the sample of every hour angle; arrays or device
    tensors.  Returns a device tensor ``[vis.shape[0], len(ra_index)]`` float64, zero at frequencies not in ``f_index``.
    """
    ctx = Context.get()
    vis_d = ctx.to_device(vis, np.complex64)
    w_d = ctx.to_device(weight, np.float64)
    if vis_d.ndim != 3 or tuple(w_d.shape) != tuple(vis_d.shape):
        raise ValueError(f"vis of shape {tuple(vis_d.shape)} and weight of shape {tuple(w_d.shape)}")
    nfreq, nra, ns = (int(s) for s in vis_d.shape)
    u_d, v_d = ctx.to_device(u, np.float64), ctx.to_device(v, np.float64)
    if tuple(u_d.shape) != (nfreq, ns) or tuple(v_d.shape) != (nfreq, ns):
        raise ValueError(f"u / v of shape {tuple(u_d.shape)} / {tuple(v_d.shape)}, expected {(nfreq, ns)}")
    ra_index = np.asarray(ra_index, dtype=np.int64).reshape(1, -1)
    nha = ra_index.shape[1]
    cosha, sinha = np.asarray(cosha, dtype=np.float64), np.asarray(sinha, dtype=np.float64)
    if cosha.shape != (nha,) or sinha.shape != (nha,):
        raise ValueError("cosha, sinha and ra_index differ in length")
    if nha and (ra_index.min() < 0 or ra_index.max() >= nra):
        raise ValueError("ra_index outside the axis")
    f_index = np.asarray(f_index, dtype=np.int64)
    if f_index.size and (f_index.min() < 0 or f_index.max() >= nfreq):
        raise ValueError("f_index outside the axis")
    if nha == 0:
        return ctx.zeros((nfreq, 0), np.float64)
    fmask = np.zeros((1, nfreq), dtype=bool)
    fmask[0, f_index] = True
    ut, vt = phase_tables(dec, lat, cosha, sinha)
    return form(ctx, vis_d, w_d, u_d, v_d, ut.reshape(1, nha), vt.reshape(1, nha), ra_index, fmask)[0]
