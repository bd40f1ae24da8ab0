"""DAYENU high-pass delay filter on the GPU (https://arxiv.org/abs/2004.11397).

Drop-in for the frequency-axis foreground filter of ``draco/analysis/dayenu.py``:

* :func:`delay_filter`, :func:`highpass_delay_filter`   ``dayenu.py:1125-1232``
* :class:`DayenuDelayFilter`      ``dayenu.py:20-193``   (``SiderealStream`` / ``TimeStream``)
* :class:`DayenuDelayFilterMap`   ``dayenu.py:776-975``  (``RingMap``)

Same names, config attributes, defaults and ``setup`` / ``process`` signatures.  The arithmetic runs in
``libdraco_amd.so`` (``csrc/dayenu.hip``): a per-item mask pass, a batched float64 Cholesky inverse of the masked
covariance, and an in-place apply on the f64 matrix cores; the datasets stay on the device.

The reference takes ``numpy.linalg.pinv`` of the masked covariance.  Its eigenvalue cut, ``1e-15 lambda_max``, keeps
every eigenvalue of these matrices (the smallest is about 1), so the pseudo-inverse is the inverse of the unflagged
block embedded in zeros, which is what the library forms.  Where the cut could reach an eigenvalue an inverse keeps
(``1e-15 x`` an upper bound of ``lambda_max`` at or above 0.5) a ``ValueError`` is raised instead of a silently
different filter.

The filter needs the whole band in one process: frequency sharding does not apply to these two tasks.

Out of scope (``NotImplementedError`` where a parameter asks for it): ``single_mask=False`` (a filter per time
sample), off-centre (complex) stop bands, the ``DelayCutoff`` file of the ring-map task (HDF5), and the reference's
``DayenuDelayFilterFixedCutoff``, hybrid-visibility variants and ``DayenuMFilter``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.constants
import torch

from .. import _lib
from ..core import io
from ..core.task import ContainerTask
from ..device import Context, ptr
from .transform import _dev_dataset

MAX_ORDER = 1024
_GROUP = {_lib.DMM_DAYENU_F32: 32, _lib.DMM_DAYENU_F64: 16}  # adjacent items per block of the items-contiguous layout


def _bands(tau_width, tau_centre, epsilon):
    """The reference's ``_ensure_consistent`` (``dayenu.py:1157-1168``): ``[nband, 2]`` (tw, eps)."""
    args = [np.atleast_1d(np.asarray(p, dtype=np.float64)) for p in (tau_width, tau_centre, epsilon)]
    nband = max(a.size for a in args)
    for a in args:
        assert a.size in (1, nband)
    tw, tc, eps = (np.broadcast_to(a, (nband,)) for a in args)
    if np.any(np.abs(tc) > 0.0):
        raise NotImplementedError("delay_filter: a non-zero tau_centre makes the covariance complex; only stop bands centred on zero delay run on the GPU")
    return np.stack([tw, eps], axis=-1)


def check_eigenvalue_cut(freq, bands):
    """Raise ``ValueError`` if ``numpy.linalg.pinv``'s cut, ``1e-15 lambda_max``, could reach 0.5: ``lambda_max`` is
    bounded from above by the largest absolute row sum of the unmasked covariance."""
    freq = np.asarray(freq, dtype=np.float64)
    dfreq = freq[:, np.newaxis] - freq[np.newaxis, :]
    cov = np.eye(freq.size)
    for tw, eps in np.asarray(bands, dtype=np.float64).reshape(-1, 2):
        cov = cov + np.abs(np.sinc(2.0 * tw * dfreq) / eps)
    bound = float(np.abs(cov).sum(axis=1).max())
    if not 1e-15 * bound < 0.5:
        raise ValueError(
            f"DAYENU filter: 1e-15 x lambda_max may reach {1e-15 * bound:.3g} (row-sum bound), so the reference's pseudo-inverse "
            "could drop modes that the inverse formed here keeps; choose a larger epsilon"
        )


def build_filters(ctx, freq_d, bands, masks, out=None):
    """``nf [nmat, nfreq, nfreq]`` float64 on the device and the per-matrix status words (host) for ``bands
    [nmat, nband, 2]`` and ``masks [nmat, nfreq]`` (host arrays)."""
    bands = np.ascontiguousarray(bands, dtype=np.float64)
    masks = np.ascontiguousarray(masks, dtype=np.uint8)
    nmat, nfreq = masks.shape
    nf = ctx.empty((nmat, nfreq, nfreq), np.float64) if out is None else out
    status = ctx.zeros((nmat,), np.int32)
    bands_d, masks_d = ctx.to_device(bands), ctx.to_device(masks)
    _lib.check(_lib.lib.dmm_dayenu_build(ctx.handle, int(nfreq), int(nmat), int(bands.shape[1]), ptr(freq_d), ptr(bands_d), ptr(masks_d), ptr(nf), ptr(status)))
    ctx.uses(bands_d, masks_d)
    return nf, status.cpu().numpy()


def delay_filter(freq, flag, tau_width, tau_centre=0.0, epsilon=1e-12):
    """Construct a delay filter (``dayenu.py:1125-1202``).

    Returns ``(pinv, index)``: ``pinv [ntime_uniq, nfreq, nfreq]`` float64 **on the device**, one filter per set of
    unique frequency flags (grouped on the host as the reference does), and ``index``, the time samples each applies to.
    ``tau_centre`` must be zero (``NotImplementedError`` otherwise); a matrix that is not positive definite raises
    ``numpy.linalg.LinAlgError``.  The whole band has to be given: the filter cannot be built per frequency shard.
    """
    freq = np.ascontiguousarray(freq, dtype=np.float64)
    flag = np.asarray(flag)
    nfreq = freq.size
    assert flag.shape[0] == nfreq and flag.ndim == 2
    if not 1 <= nfreq <= MAX_ORDER:
        raise ValueError(f"delay_filter: {nfreq} frequencies, the kernels take 1 ... {MAX_ORDER}")
    bands = _bands(tau_width, tau_centre, epsilon)
    check_eigenvalue_cut(freq, bands)
    uflag, uindex = np.unique(flag.reshape(nfreq, -1).astype(bool), return_inverse=True, axis=-1)
    uindex = np.asarray(uindex).reshape(-1)
    masks = np.ascontiguousarray(uflag.T)
    nuniq = masks.shape[0]
    ctx = Context.get()
    freq_d = ctx.to_device(freq)
    pinv = ctx.empty((nuniq, nfreq, nfreq), np.float64)
    per = max(1, min(65535, (1 << 30) // (16 * nfreq * nfreq)))
    for m0 in range(0, nuniq, per):
        m1 = min(nuniq, m0 + per)
        _, status = build_filters(ctx, freq_d, np.broadcast_to(bands, (m1 - m0, *bands.shape)), masks[m0:m1], out=pinv[m0:m1])
        if status.any():
            raise np.linalg.LinAlgError(f"delay_filter: the covariance of mask {m0 + int(np.flatnonzero(status)[0])} is not positive definite")
    return pinv, [np.flatnonzero(uindex == uu) for uu in range(nuniq)]


def highpass_delay_filter(freq, tau_cut, flag, epsilon=1e-12):
    """Construct a high-pass delay filter with the stop band ``[-tau_cut, tau_cut]`` (``dayenu.py:1205-1232``)."""
    return delay_filter(freq, flag, tau_cut, 0.0, epsilon)


def _side(t, ncol, sf, sc, si, so):
    return _lib.dmm_dayenu_side(C.c_void_p(t.data_ptr()), int(ncol), int(sf), int(sc), int(si), int(so))


def apply_filters(ctx, dtype, layout, nfreq, ninner, nouter, nf, item_matrix_d, atten_d, units_d, nunit, data, weight):
    """One ``dmm_dayenu_apply`` launch; ``data`` / ``weight`` are ``dmm_dayenu_side`` or ``None``."""
    _lib.check(
        _lib.lib.dmm_dayenu_apply(
            ctx.handle, dtype, layout, int(nfreq), int(ninner), int(nouter), ptr(nf), int(nf.shape[0]), ptr(item_matrix_d), ptr(atten_d), ptr(units_d), int(nunit),
            C.byref(data) if data is not None else None, C.byref(weight) if weight is not None else None,
        )
    )


class _DayenuTask(ContainerTask):
    """What the two tasks share: mask pass, filter sharing, batched build, apply."""

    _config_names = ("epsilon", "tauw", "single_mask", "atten_threshold", "workspace_mib")
    epsilon = 1e-12
    tauw = 0.100
    single_mask = True
    atten_threshold = 0.0
    workspace_mib = 1024  # device memory the filters of one batch (and their factorisation scratch) may take

    def _check(self):
        if not self.single_mask:
            raise NotImplementedError(f"{type(self).__name__}: single_mask=False (a filter per time sample) is not on the GPU path")

    def _filter(self, ctx, dtype, layout, freq, cutoff, ninner, nouter, datas, weight, what):
        """``cutoff [nouter * ninner]``: delay cut of every item.  ``datas``: one side per beam (the weights are filtered
        once).  Items with no frequency left are skipped; items whose matrix fails keep their data and lose their weight."""
        freq = np.ascontiguousarray(freq, dtype=np.float64)
        nfreq, nitem = freq.size, ninner * nouter
        if not 1 <= nfreq <= MAX_ORDER:
            raise ValueError(f"{type(self).__name__}: {nfreq} frequencies, the kernels take 1 ... {MAX_ORDER}")
        for cut in np.unique(cutoff):
            check_eigenvalue_cut(freq, [[cut, self.epsilon]])
        flag_d = ctx.empty((nouter, ninner, nfreq), np.uint8)
        _lib.check(_lib.lib.dmm_dayenu_mask(ctx.handle, dtype, layout, nfreq, ninner, nouter, C.byref(weight), ptr(flag_d)))
        flags = flag_d.cpu().numpy().reshape(nitem, nfreq)

        # items with the same (cutoff, mask) share one filter
        keys, cuts, masks = {}, [], []
        imat = np.full(nitem, -1, dtype=np.int64)
        for it in np.flatnonzero(flags.any(axis=1)):
            key = (float(cutoff[it]), flags[it].tobytes())
            if key not in keys:
                keys[key] = len(cuts)
                cuts.append(key[0])
                masks.append(flags[it])
            imat[it] = keys[key]
        nuniq = len(cuts)
        self.log.debug(f"{nitem} {what}s, {int((imat >= 0).sum())} to filter, {nuniq} distinct filters.")
        if nuniq == 0:
            return
        freq_d = ctx.to_device(freq)
        group = _GROUP[dtype]
        ngroup = (ninner + group - 1) // group
        per = max(1, min(65535, (int(self.workspace_mib) << 20) // (16 * nfreq * nfreq)))
        for m0 in range(0, nuniq, per):
            m1 = min(nuniq, m0 + per)
            bands = np.stack([np.asarray(cuts[m0:m1]), np.full(m1 - m0, self.epsilon)], axis=-1)[:, np.newaxis, :]
            nf, status = build_filters(ctx, freq_d, bands, np.stack(masks[m0:m1]))
            sel = np.flatnonzero((imat >= m0) & (imat < m1))
            local = np.full(nitem, -1, dtype=np.int32)
            local[sel] = imat[sel] - m0
            for it in sel[status[local[sel]] != 0]:
                self.log.error(
                    f"Failed to factorise the covariance while processing {what} {it} [{cutoff[it]:0.3f} micro-sec]\n"
                    f"Percentage unmasked frequencies:  {100 * flags[it].mean():0.1f}"
                )
                local[it] = -2
            atten_d = None
            if self.atten_threshold > 0.0:
                diag = torch.diagonal(nf, dim1=1, dim2=2).cpu().numpy()
                low = np.zeros(diag.shape, dtype=np.uint8)
                for m in range(m1 - m0):
                    if status[m] == 0:
                        low[m] = diag[m] > (self.atten_threshold * np.median(diag[m][diag[m] > 0.0]))
                atten_d = ctx.to_device(low)
            if layout == _lib.DMM_DAYENU_COLS:
                units = sel.astype(np.int32)
            else:
                units = np.unique((sel // ninner) * ngroup + (sel % ninner) // group).astype(np.int32)
            units_d, local_d = ctx.to_device(units), ctx.to_device(local)
            for b, data in enumerate(datas):
                apply_filters(ctx, dtype, layout, nfreq, ninner, nouter, nf, local_d, atten_d, units_d, len(units), data, weight if b == 0 else None)
            ctx.uses(nf, atten_d, units_d, local_d)
        ctx.uses(freq_d, flag_d)


class DayenuDelayFilter(_DayenuTask):
    """Apply a DAYENU high-pass delay filter to visibility data (``dayenu.py:20-193``).

    Attributes
    ----------
    za_cut : float
        Sine of the maximum zenith angle included in baseline-dependent delay filtering.  Default 1.0 (the horizon);
        zero turns the baseline-dependent cut off.
    telescope_orientation : one of ('NS', 'EW', 'none')
        Whether the baseline-dependent delay cut is based on the north-south component, the east-west component or the
        full baseline length.  Default 'NS'.
    epsilon : float
        The stop-band rejection of the filter.  Default 1e-12.
    tauw : float
        Delay cutoff in micro-seconds.  Default 0.1.
    single_mask : bool
        One frequency mask for all times: only frequencies whose weights are non-zero at all times are kept.  Default
        True; ``False`` raises ``NotImplementedError``.
    atten_threshold : float
        Mask any frequency where the diagonal element of the filter is not above this fraction of the median over the
        unmasked frequencies.  Default 0.0 (off).

    Works in place and returns the input container with device-resident ``vis`` and ``vis_weight``.  Stack entries with
    the same cutoff and mask share one filter.  The whole band must be in this process.
    """

    _config_names = ("za_cut", "telescope_orientation")
    za_cut = 1.0
    telescope_orientation = "NS"

    def read_config(self, params):
        super().read_config(params)
        if self.telescope_orientation not in ("NS", "EW", "none"):
            raise ValueError(f"telescope_orientation must be 'NS', 'EW' or 'none', not {self.telescope_orientation!r}")

    def setup(self, telescope):
        """Set the telescope needed to obtain baselines."""
        self.telescope = io.get_telescope(telescope)
        self.log.info(f"Instrumental delay cut set to {self.tauw:.3f} micro-sec.")
        if self.atten_threshold > 0.0:
            self.log.info(f"Flagging frequencies with attenuation less than {self.atten_threshold:0.2f} of median attenuation.")

    def process(self, stream):
        """Filter out delays from a SiderealStream or TimeStream, in place."""
        self._check()
        stream.redistribute(["input", "prod", "stack"])
        ctx = Context.get()
        cutoff = self._get_cut(stream.prodstack)
        vis = _dev_dataset(stream.vis, ctx, np.complex64)
        weight = _dev_dataset(stream.weight, ctx, np.float32)
        nfreq, nstack, nra = (int(s) for s in vis.shape)
        if len(cutoff) != nstack:
            raise ValueError(f"{len(cutoff)} products for {nstack} stack entries")
        data = _side(vis, 2 * nra, 2 * nstack * nra, 1, 2 * nra, 0)
        wside = _side(weight, nra, nstack * nra, 1, nra, 0)
        self._filter(ctx, _lib.DMM_DAYENU_F32, _lib.DMM_DAYENU_COLS, stream.freq[:], cutoff, nstack, 1, [data], wside, "baseline")
        stream.vis.set_device(vis)
        stream.weight.set_device(weight)
        return stream

    def _get_cut(self, prod):
        baselines = self.telescope.feedpositions[prod["input_a"], :] - self.telescope.feedpositions[prod["input_b"], :]
        if self.telescope_orientation == "NS":
            baselines = abs(baselines[:, 1])  # Y baseline
        elif self.telescope_orientation == "EW":
            baselines = abs(baselines[:, 0])  # X baseline
        else:
            baselines = np.sqrt(np.sum(baselines**2, axis=-1))  # Norm
        baseline_delay_cut = 1e6 * self.za_cut * baselines / scipy.constants.c
        return baseline_delay_cut + self.tauw


class DayenuDelayFilterMap(_DayenuTask):
    """Apply a DAYENU high-pass delay filter to ringmap data (``dayenu.py:776-975``).

    Attributes
    ----------
    epsilon, tauw, single_mask, atten_threshold
        As for :class:`DayenuDelayFilter`; ``tauw`` is the delay cutoff of every el.
    filename : str
        An HDF5 ``DelayCutoff`` container in the reference.  HDF5 is outside this package: anything but ``None`` raises
        ``NotImplementedError``.

    Works in place and returns the input container with device-resident ``map`` and ``weight``.  The ``(pol, el)``
    columns with the same mask share one filter; with several beams the weights are filtered once, from the masks of
    the unfiltered weights.  The whole band must be in this process.
    """

    _config_names = ("filename",)
    filename = None

    def setup(self):
        """Check the configuration (there is no cutoff file to load)."""
        if self.filename is not None:
            raise NotImplementedError("DayenuDelayFilterMap: the DelayCutoff file (HDF5) is not supported; leave filename unset and use tauw")
        if self.atten_threshold > 0.0:
            self.log.info(f"Flagging frequencies with attenuation less than {self.atten_threshold:0.2f} of median attenuation.")

    def process(self, ringmap):
        """Filter out delays from a RingMap, in place."""
        self._check()
        if self.filename is not None:
            raise NotImplementedError("DayenuDelayFilterMap: the DelayCutoff file (HDF5) is not supported; leave filename unset and use tauw")
        ringmap.redistribute("el")
        ctx = Context.get()
        rmap = _dev_dataset(ringmap.map, ctx, np.float64)
        weight = _dev_dataset(ringmap.weight, ctx, np.float64)
        nbeam, npol, nfreq, nra, nel = (int(s) for s in rmap.shape)
        plane = nfreq * nra * nel
        datas = [_side(rmap[b], nra, nra * nel, nel, 1, plane) for b in range(nbeam)]
        wside = _side(weight, nra, nra * nel, nel, 1, plane)
        cutoff = np.full(npol * nel, float(self.tauw))
        self._filter(ctx, _lib.DMM_DAYENU_F64, _lib.DMM_DAYENU_ITEMS, ringmap.freq[:], cutoff, nel, npol, datas, wside, "el")
        ringmap.map.set_device(rmap)
        ringmap.weight.set_device(weight)
        ringmap.redistribute("freq")
        return ringmap


__all__ = ["DayenuDelayFilter", "DayenuDelayFilterMap", "delay_filter", "highpass_delay_filter"]
