"""DAYENU filters on the GPU (https://arxiv.org/abs/2004.11397): the high-pass delay filter along frequency and the
m-mode filter along right ascension.

Drop-in for ``draco/analysis/dayenu.py``:

* :func:`delay_filter`, :func:`highpass_delay_filter`   ``dayenu.py:1125-1232``
* :class:`DayenuDelayFilter`      ``dayenu.py:20-193``   (``SiderealStream`` / ``TimeStream``)
* :class:`DayenuDelayFilterMap`   ``dayenu.py:776-975``  (``RingMap``)
* :class:`DayenuDelayFilterHybridVis`  ``dayenu.py:407-572`` (``HybridVisStream``; keeps ``filter`` and ``freq_cov``)
* :class:`ApplyDelayFilterHybridVis`, :class:`ApplyDelayFilterHybridVisSingleSource`  ``dayenu.py:575-773``
* :class:`DayenuMFilter`          ``dayenu.py:977-1122`` (``SiderealStream``)
* :func:`bandpass_mmode_filter`, :func:`lowpass_mmode_filter`, :func:`highpass_mmode_filter`, :func:`instantaneous_m`
  ``dayenu.py:1235-1427``

Same names, config attributes, defaults and ``setup`` / ``process`` signatures.  The delay filter's arithmetic runs in
``libdraco_amd.so`` (``csrc/dayenu.hip``): a per-item mask pass, a batched float64 Cholesky inverse of the masked
covariance, and an in-place apply on the f64 matrix cores; the datasets stay on the device.

The m-mode filter (``csrc/mfilter.hip``) has one pair of matrices per frequency, of the order of the RA axis (up to
4096), and nothing couples frequencies: it shards by frequency.  Its task never forms a filter matrix: per frequency
and kind the masked covariance is Cholesky-factored in float64 and the real and imaginary rows of the stack entries
are solved as right-hand sides; only the three builder functions return the matrix, from the same solve on a masked
identity.  The eigenvalue argument below holds for it too (eigenvalues in about ``[1, 1 / (a epsilon)]``).

The reference takes ``numpy.linalg.pinv`` of the masked covariance.  Its eigenvalue cut, ``1e-15 lambda_max``, keeps
every eigenvalue of these matrices (the smallest is about 1), so the pseudo-inverse is the inverse of the unflagged
block embedded in zeros, which is what the library forms.  Where the cut could reach an eigenvalue an inverse keeps
(``1e-15 x`` an upper bound of ``lambda_max`` at or above 0.5) a ``ValueError`` is raised instead of a silently
different filter.

The filter needs the whole band in one process: frequency sharding does not apply to these two tasks.

Out of scope (``NotImplementedError`` where a parameter asks for it): ``single_mask=False`` (a filter per time
sample), off-centre (complex) stop bands and stored complex filters, the ``DelayCutoff`` file of the ring-map task
(HDF5), the reference's ``DayenuDelayFilterFixedCutoff`` and, of the hybrid-visibility tasks, ``elevation_vis_weight``
streams and MPI redistribution.

:class:`ApplyDelayFilterHybridVis` and :class:`ApplyDelayFilterHybridVisSingleSource` (``dayenu.py:575-773``) apply a
filter that :class:`DayenuDelayFilterHybridVis` left on a stream to another stream (``csrc/hyfores.hip``); every
sample has a matrix of its own there, so the product is a per-lane one along RA, not the shared-matrix GEMM above.
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
MAX_RA = 4096  # order of the m-mode filter (the RA axis)
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



def _group_rows(flags):
    """``(masks [nuniq, n], index [nrow])`` of the distinct non-empty rows of ``flags [nrow, n]`` (bytes, 0 or 1); the
    index of an empty row is -1.  The rows are packed into 64-bit words and sorted: ``numpy.unique(axis=0)`` on byte
    rows costs tens of milliseconds for the 8192 samples of a stream."""
    index = np.full(flags.shape[0], -1, dtype=np.int64)
    valid = np.flatnonzero(flags.any(axis=1))
    if valid.size == 0:
        return np.zeros((0, flags.shape[1]), dtype=np.uint8), index
    bits = np.packbits(flags[valid], axis=1)
    words = np.zeros((valid.size, -(-bits.shape[1] // 8) * 8), dtype=np.uint8)
    words[:, : bits.shape[1]] = bits
    words = words.view(np.uint64)
    order = np.lexsort(words.T[::-1])
    first = np.ones(valid.size, dtype=bool)
    first[1:] = np.any(words[order[1:]] != words[order[:-1]], axis=1)
    index[valid[order]] = np.cumsum(first) - 1
    return flags[valid[order[first]]], index


class DayenuDelayFilterHybridVis(ContainerTask):
    """Apply a DAYENU high-pass delay filter to hybrid beamformed visibilities (``dayenu.py:407-572``).

    Attributes
    ----------
    tauw : float or array [nstopband]
        The half width of the stop-band region in micro-seconds.  Default 0.4.
    tauc : float or array [nstopband]
        The centre of the stop-band region in micro-seconds.  Default 0; anything else raises ``NotImplementedError``.
    epsilon : float or array [nstopband]
        The stop-band rejection.  Default 1e-12.
    atten_threshold : float
        Mask any frequency where the diagonal element of the filter is not above this fraction of the median over the
        unmasked frequencies.  Default 0.0 (off).
    apply_filter : bool
        Apply the filter that was generated.  If False, ``save_filter`` must be True.  Default True.
    save_filter : bool
        Save the filter to the ``filter`` dataset of the stream.  Default False.
    calculate_cov : bool
        Calculate the frequency-frequency noise covariance due to filtering, ``freq_cov = NF diag(1 / weight) NF^T``
        from the weights before filtering.  Default False.  As in the reference it is left zero without ``apply_filter``.
    workspace_mib : int
        Device memory the filters of one batch (and their factorisation scratch) may take.  Default 1024.

    Works in place and returns the input container; ``vis``, ``vis_weight``, ``filter`` and ``freq_cov`` stay on the
    device.  There is one filter per ``(ew, ra)`` sample, from the channels whose weight is positive in every
    polarisation; all polarisations and elevations of the sample use it, and samples with the same mask share one
    build.  A sample with no such channel is skipped; one whose factorisation fails is logged, loses its weight (with
    ``apply_filter``) and keeps zero ``filter`` and ``freq_cov``.  The whole band must be in this process.
    """

    _config_names = ("tauw", "tauc", "epsilon", "atten_threshold", "apply_filter", "save_filter", "calculate_cov", "workspace_mib")
    tauw = 0.4
    tauc = 0.0
    epsilon = 1e-12
    atten_threshold = 0.0
    apply_filter = True
    save_filter = False
    calculate_cov = False
    workspace_mib = 1024

    def read_config(self, params):
        params = dict(params)
        for k in ("tauw", "tauc", "epsilon"):  # (the reference's proptype is numpy.atleast_1d)
            if k in params:
                setattr(self, k, np.atleast_1d(np.asarray(params.pop(k), dtype=np.float64)))
        super().read_config(params)

    def setup(self):
        """Check that `save_filter` and `apply_filter` are set."""
        if not self.apply_filter and not self.save_filter:
            raise RuntimeError("At least one of `save_filter` and `apply_filter` must be True.")

    def process(self, stream):
        """Filter out delays from a HybridVisStream, in place."""
        bands = _bands(self.tauw, self.tauc, self.epsilon)  # (NotImplementedError for a non-zero tauc)
        stream.redistribute(["ra", "time"])
        ctx = Context.get()
        lib = _lib.lib
        freq = np.ascontiguousarray(stream.freq[:], dtype=np.float64)
        vis = _dev_dataset(stream.vis, ctx, np.complex64)
        weight = _dev_dataset(stream.weight, ctx, np.float32)
        npol, nfreq, new, nel, nra = (int(s) for s in vis.shape)
        if tuple(weight.shape) != (npol, nfreq, new, nra) or freq.size != nfreq:
            raise ValueError(f"vis {tuple(vis.shape)}, vis_weight {tuple(weight.shape)} and {freq.size} frequencies do not match")
        if not 1 <= nfreq <= MAX_ORDER:
            raise ValueError(f"{type(self).__name__}: {nfreq} frequencies, the kernels take 1 ... {MAX_ORDER}")
        check_eigenvalue_cut(freq, bands)
        if not self.apply_filter:
            self.log.debug("Filter will be generated but not applied.")
        nitem = new * nra
        kept = {}
        for name, on in (("filter", self.save_filter), ("freq_cov", self.calculate_cov)):
            if on:
                if name not in stream.datasets:
                    stream.add_dataset(name)
                kept[name] = ctx.empty((npol, nfreq, nfreq, new, nra), np.float64)

        # flag[f] = all_pol(weight > 0) per (ew, ra) sample; samples with the same mask share one filter
        flag_d = ctx.empty((nfreq, new, nra), np.uint8)
        _lib.check(lib.dmm_dayenu_hybrid_mask(ctx.handle, npol, nfreq, new, nra, ptr(weight), ptr(flag_d)))
        flags = np.ascontiguousarray(flag_d.cpu().numpy().reshape(nfreq, nitem).T)
        ctx.uses(flag_d)
        masks, imat = _group_rows(flags)
        valid = np.flatnonzero(imat >= 0)
        nuniq = masks.shape[0]
        self.log.debug(f"{nitem} (ew, ra) samples, {valid.size} to filter, {nuniq} distinct filters.")
        if nuniq == 0 or not self.apply_filter:
            for name, t in kept.items():
                if nuniq == 0 or name == "freq_cov":
                    t.zero_()

        freq_d = ctx.to_device(freq)
        group = _GROUP[_lib.DMM_DAYENU_F32]
        wide = 2 * nra  # the real and imaginary parts of a sample are two adjacent items with the same filter
        per = max(1, min(65535, (int(self.workspace_mib) << 20) // (16 * nfreq * nfreq)))
        for m0 in range(0, nuniq, per):
            m1 = min(nuniq, m0 + per)
            nf, status = build_filters(ctx, freq_d, np.repeat(bands[np.newaxis], m1 - m0, axis=0), masks[m0:m1])
            sel = np.flatnonzero((imat >= m0) & (imat < m1))
            local = np.full(nitem, -1, dtype=np.int32)
            local[sel] = imat[sel] - m0
            for it in sel[status[local[sel]] != 0]:
                self.log.error(
                    f"Failed to factorise the covariance while processing ew {it // nra}, ra {it % nra}\n"
                    f"Percentage unmasked frequencies:  {100 * flags[it].mean():0.1f}"
                )
                local[it] = -2
            local_d = ctx.to_device(local)
            skip = 0 if m0 == 0 else 1  # the first batch also zeroes the samples that have no filter
            if self.save_filter:
                _lib.check(lib.dmm_dayenu_hybrid_save(ctx.handle, npol, nfreq, new, nra, ptr(nf), m1 - m0, ptr(local_d), skip, ptr(kept["filter"])))
            if self.calculate_cov and self.apply_filter:
                _lib.check(lib.dmm_dayenu_hybrid_cov(ctx.handle, npol, nfreq, new, nra, ptr(nf), m1 - m0, ptr(local_d), ptr(weight), skip, ptr(kept["freq_cov"])))
            if self.apply_filter:
                atten_d = None
                if self.atten_threshold > 0.0:
                    diag = torch.diagonal(nf, dim1=1, dim2=2).cpu().numpy()
                    low = np.zeros(diag.shape, dtype=np.uint8)
                    for m in range(m1 - m0):
                        if status[m] == 0:
                            low[m] = diag[m] > (self.atten_threshold * np.median(diag[m][diag[m] > 0.0]))
                    atten_d = ctx.to_device(low)
                ngw, ngd = (nra + group - 1) // group, (wide + group - 1) // group
                uw = np.unique((sel // nra) * ngw + (sel % nra) // group).astype(np.int32)
                ud = np.unique((sel // nra) * ngd + (2 * (sel % nra)) // group).astype(np.int32)
                wide_d = ctx.to_device(np.repeat(local, 2))
                uw_d, ud_d = ctx.to_device(uw), ctx.to_device(ud)
                vr = torch.view_as_real(vis)
                for pp in range(npol):
                    data = _side(vr[pp], nel, 2 * new * nel * nra, 2 * nra, 1, 2 * nel * nra)
                    wside = _side(weight[pp], 1, new * nra, 0, 1, nra)
                    apply_filters(ctx, _lib.DMM_DAYENU_F32, _lib.DMM_DAYENU_ITEMS, nfreq, wide, new, nf, wide_d, None, ud_d, len(ud), data, None)
                    apply_filters(ctx, _lib.DMM_DAYENU_F32, _lib.DMM_DAYENU_ITEMS, nfreq, nra, new, nf, local_d, atten_d, uw_d, len(uw), None, wside)
                ctx.uses(atten_d, wide_d, uw_d, ud_d)
            ctx.uses(nf, local_d)
        ctx.uses(freq_d)
        stream.vis.set_device(vis)
        stream.weight.set_device(weight)
        for name, t in kept.items():
            stream.attach(name, t)
        stream.redistribute("freq")
        return stream


_MISMATCH = (
    ("freq", "Frequencies do not match for hybrid visibilities."),
    ("el", "Elevations do not match for hybrid visibilities."),
    ("ew", "EW baselines do not match for hybrid visibilities."),
    ("pol", "Polarisations do not match for hybrid visibilities."),
    ("ra", "Right Ascension do not match for hybrid visibilities."),
)


def check_hybrid_match(source, hv):
    """The reference's five ``ValueError`` s (``dayenu.py:621-635``)."""
    for ax, msg in _MISMATCH:
        a, b = (s.freq if ax == "freq" else s.index_map[ax] for s in (source, hv))
        if not np.array_equal(a, b):
            raise ValueError(msg)


def check_real_filter(source):
    """``NotImplementedError`` for a stored complex filter, ``KeyError`` where there is none."""
    if "complex_filter" in source.datasets:
        raise NotImplementedError("stored complex filters (off-centre stop bands) are not supported")
    if "filter" not in source.datasets:
        raise KeyError("Dataset 'filter' not initialised.")
    if np.dtype(source.datasets["filter"].dtype).kind == "c":
        raise NotImplementedError("stored complex filters (off-centre stop bands) are not supported")


def stored_filter(source, ctx, shape):
    """The real ``filter`` dataset of ``source`` on the device; ``shape`` is that of the visibilities it is applied to."""
    check_real_filter(source)
    filt = _dev_dataset(source.datasets["filter"], ctx, np.float64)
    npol, nfreq, new, nel, nra = shape
    if tuple(filt.shape) != (npol, nfreq, nfreq, new, nra):
        raise ValueError(f"filter {tuple(filt.shape)} does not match visibilities {tuple(shape)}")
    if not 1 <= nfreq <= MAX_ORDER:
        raise ValueError(f"{nfreq} frequencies, the kernels take 1 ... {MAX_ORDER}")
    return filt


def attenuation_flags(ctx, filt, atten_threshold):
    """``[pol, freq, ew, ra]`` bytes on the device: ``|F[f, f]| > atten_threshold x median`` over the non-zero
    ``|F[f, f]|`` of the sample (1 everywhere for a sample whose diagonal is zero).  The diagonal, 1 / nfreq of the
    filter, is gathered on the device; the median is ``numpy.median`` on the host, as the reference's."""
    diag = torch.diagonal(filt, dim1=1, dim2=2).abs().cpu().numpy()  # [pol, ew, ra, freq]
    nonzero = diag > 0.0
    some = nonzero.any(axis=-1, keepdims=True)
    # (the median of the non-zero entries of a row: NaN marks the others; a row without any gets a 1 in their place)
    med = np.nanmedian(np.where(nonzero | ~some, np.where(some, diag, 1.0), np.nan), axis=-1, keepdims=True)
    low = np.where(some, diag > atten_threshold * med, True)
    return ctx.to_device(np.ascontiguousarray(np.moveaxis(low, -1, 1)).astype(np.uint8))


def apply_stored_filter(ctx, vis, weight, filt, gain=None, atten_threshold=0.0, atten_vis=False, keep_input=True, want_weight=True, want_cov=False):
    """``(vis_out, weight_out, freq_cov, status, atten)`` of ``dmm_hybrid_filter_apply`` (``include/draco_amd.h``):
    device tensors, ``None`` for what was not asked for; ``status [pol, ew, ra]`` bytes.  ``gain [pol, ew, freq]``
    complex128 (host) takes ``1 - gain`` out of the data first."""
    npol, nfreq, new, nel, nra = (int(s) for s in vis.shape)
    atten = attenuation_flags(ctx, filt, atten_threshold) if atten_threshold > 0.0 else None
    gain_d = None if gain is None else ctx.to_device(np.ascontiguousarray(gain, dtype=np.complex128))
    vis_out = ctx.empty(vis.shape, np.complex64)
    weight_out = ctx.empty(weight.shape, np.float32) if want_weight else None
    cov = ctx.empty(filt.shape, np.float64) if want_cov else None
    bits = ctx.empty((npol, new, nra), np.int32)
    status = ctx.empty((npol, new, nra), np.uint8)
    _lib.check(
        _lib.lib.dmm_hybrid_filter_apply(ctx.handle, npol, nfreq, new, nel, nra, ptr(filt), ptr(vis), ptr(weight), ptr(gain_d), ptr(atten), int(bool(atten_vis)), int(bool(keep_input)),
                                         ptr(vis_out), ptr(weight_out), ptr(cov), ptr(bits), ptr(status))
    )
    ctx.uses(gain_d, bits)
    return vis_out, weight_out, cov, status, atten


def log_filter_status(log, ctx, status, weight, filt):
    """The reference's warning for every missing-frequency sample (``dayenu.py:692-698``), from the status bytes."""
    st = status.cpu().numpy()
    for p, x, t in np.argwhere(st == _lib.DMM_HFA_MISSING_FREQ):
        flag = weight[p, :, x, t].cpu().numpy() > 0.0
        valid = (filt[p, :, :, x, t] != 0.0).any(dim=0).cpu().numpy()
        log.warning(f"Missing the following frequencies that were assumed valid during filter generation: {np.flatnonzero(valid & ~flag)}")
    return st


class ApplyDelayFilterHybridVis(ContainerTask):
    """Apply a previously saved filter to hybrid beamformed visibilities (``dayenu.py:575-739``): how the 21-cm
    simulation gets the data's foreground filter.

    Attributes
    ----------
    atten_threshold : float
        Mask any frequency where the diagonal element of the filter is not above this fraction of the median over the
        non-zero diagonal elements.  Default 0.0 (off).
    calculate_cov : bool
        Calculate the frequency-frequency noise covariance due to filtering.  Default False.
    copy_weight : bool
        Do not propagate the weights through the filter; copy ``vis_weight`` (and ``freq_cov``) from the container the
        filter came from.  Default False.
    copy_tag : bool
        Copy the tag from the container the filter came from.  Default False.

    Works in place and returns ``hv``; ``vis``, ``vis_weight`` and ``freq_cov`` stay on the device, and ``source.filter``
    is read where it is.  The flag of a sample is per polarisation (``weight[p, :, x, t] > 0``).  A sample with no flag
    set is skipped; one whose filter is entirely zero loses its weight; one with a column of the filter non-zero where
    its flag is not set loses its weight, keeps its data and is logged.  Complex filters raise ``NotImplementedError``.
    """

    _config_names = ("atten_threshold", "calculate_cov", "copy_weight", "copy_tag")
    atten_threshold = 0.0
    calculate_cov = False
    copy_weight = False
    copy_tag = False

    def process(self, hv, source):
        """Apply the stored DAYENU filter of ``source`` to ``hv``."""
        check_hybrid_match(source, hv)
        check_real_filter(source)
        if self.copy_tag:
            hv.attrs["tag"] = source.attrs["tag"]
        ctx = Context.get()
        vis = _dev_dataset(hv.vis, ctx, np.complex64)
        weight = _dev_dataset(hv.weight, ctx, np.float32)
        filt = stored_filter(source, ctx, vis.shape)
        if self.calculate_cov and "freq_cov" not in hv.datasets:
            hv.add_dataset("freq_cov")
        own = not self.copy_weight
        vis_out, weight_out, cov, status, _ = apply_stored_filter(ctx, vis, weight, filt, atten_threshold=self.atten_threshold if own else 0.0, want_weight=own,
                                                                  want_cov=self.calculate_cov and own)
        log_filter_status(self.log, ctx, status, weight, filt)
        if self.copy_weight:
            weight_out = _dev_dataset(source.weight, ctx, np.float32).clone()
            if self.calculate_cov:
                cov = _dev_dataset(source.freq_cov, ctx, np.float64).clone()
        hv.vis.set_device(vis_out)
        hv.weight.set_device(weight_out)
        if self.calculate_cov:
            hv.attach("freq_cov", cov)
        return hv


class ApplyDelayFilterHybridVisSingleSource(ApplyDelayFilterHybridVis):
    """:class:`ApplyDelayFilterHybridVis` with one filter, given to ``setup``, for every stream (``dayenu.py:742-773``)."""

    def setup(self, source):
        """Set the stream whose DAYENU filter is applied."""
        self.source = source

    def process(self, hv):
        """Apply the stored DAYENU filter to ``hv``."""
        return super().process(hv, self.source)


class DayenuDelayFilterFixedCutoff(ContainerTask):
    """Not provided (``dayenu.py:196-404``)."""

    def __init__(self, **params):
        raise NotImplementedError("DayenuDelayFilterFixedCutoff is not provided")


def instantaneous_m(ha, lat, dec, u, v, w=0.0):
    """The instantaneous fringe rate (``dayenu.py:1399-1427``), on the host.

    ``ha``, ``lat`` and ``dec`` in radians; ``u``, ``v``, ``w`` the east-west, north-south and vertical baseline in
    wavelengths.  Returns ``2 pi d(u . s)/d(ha)`` of the direction ``s`` at that hour angle and declination.
    """
    cos_dec, sin_ha = np.cos(dec), np.sin(ha)
    rate = u * (-1 * cos_dec * np.cos(ha))
    rate = rate + v * (np.sin(lat) * cos_dec * sin_ha)
    rate = rate + w * (-1 * np.cos(lat) * cos_dec * sin_ha)
    return 2.0 * np.pi * rate


def _mmode_params(ra, kind, m_cut, m_center, epsilon):
    """``(diag, coef, m_cut, m_center)`` of ``C = diag I + coef sinc(m_cut dra / pi) cos(m_center dra)`` for the
    reference's three covariances (``dayenu.py:1267-1279, 1326-1332, 1381-1382``)."""
    if kind == "highpass":
        return (1.0, 1.0 / epsilon, float(m_cut), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.median(np.abs(np.diff(ra))) * m_cut / np.pi
        aeps = a * epsilon
        coef = a * (1.0 - 1.0 / aeps)
        diag = 1.0 / aeps
    if kind == "bandpass":
        return (float(diag), float(2 * coef), float(m_cut), float(m_center))
    return (float(diag), float(coef), float(m_cut), 0.0)


def check_mmode_eigenvalue_cut(ra, params):
    """Raise ``ValueError`` if ``numpy.linalg.pinv``'s cut, ``1e-15 lambda_max``, could reach 0.5, for ``params
    [..., 4]`` as :func:`_mmode_params` gives them.

    ``lambda_max`` is bounded by the largest absolute row sum, and that by ``|diag| + |coef| (1 + 2 sum_k min(1, 1 /
    (m_cut k delta)))``, ``k = 1 ... nra - 1``: ``|sinc(x)| <= min(1, 1 / (pi |x|))``, ``|cos| <= 1``, and two RAs ``k``
    places apart in sorted order are at least ``k delta`` apart, ``delta`` the smallest spacing.  O(nra) per matrix.
    """
    ra = np.sort(np.asarray(ra, dtype=np.float64).reshape(-1))
    par = np.asarray(params, dtype=np.float64).reshape(-1, 4)
    k = np.arange(1, ra.size, dtype=np.float64)
    delta = float(np.min(np.diff(ra))) if ra.size > 1 else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        env = np.minimum(1.0, 1.0 / (np.abs(par[:, 2, np.newaxis]) * k[np.newaxis, :] * delta))
    bound = np.abs(par[:, 0]) + np.abs(par[:, 1]) * (1.0 + 2.0 * env.sum(axis=1))
    worst = float(bound.max()) if np.all(np.isfinite(bound)) else np.inf
    if not 1e-15 * worst < 0.5:
        raise ValueError(
            f"DAYENU m-mode filter: 1e-15 x lambda_max may reach {1e-15 * worst:.3g} (row-sum bound), so the reference's "
            "pseudo-inverse could drop modes that the inverse formed here keeps; choose a larger epsilon"
        )


def _check_nra(who, nra):
    if not 1 <= nra <= MAX_RA:
        raise ValueError(f"{who}: {nra} right ascensions, the kernels take 1 ... {MAX_RA}")


def _mmode_filter(who, ra, flag, par):
    """``(pinv, index)`` of the covariance ``par`` for every unique mask of ``flag [..., nra]``."""
    ra = np.ascontiguousarray(ra, dtype=np.float64).reshape(-1)
    flag = np.asarray(flag)
    nra = ra.size
    assert flag.ndim >= 2 and flag.shape[-1] == nra
    _check_nra(who, nra)
    check_mmode_eigenvalue_cut(ra, par)
    uflag, uindex = np.unique(flag.reshape(-1, nra).astype(bool), return_inverse=True, axis=0)
    uindex = np.asarray(uindex).reshape(-1)
    nuniq = uflag.shape[0]
    ctx = Context.get()
    lib = _lib.lib
    ra_d = ctx.to_device(ra)
    pinv = ctx.empty((nuniq, nra, nra), np.float64)
    per = max(1, min(65535, (1 << 30) // (8 * nra * nra)))
    for m0 in range(0, nuniq, per):
        m1 = min(nuniq, m0 + per)
        nmat = m1 - m0
        G = ctx.empty((nmat, nra, nra), np.float64)
        status = ctx.empty((nmat,), np.int32)
        mask_d = ctx.to_device(np.ascontiguousarray(uflag[m0:m1], dtype=np.uint8))
        par_d = ctx.to_device(np.ascontiguousarray(np.broadcast_to(np.asarray(par, dtype=np.float64), (nmat, 4))))
        out = pinv[m0:m1]
        _lib.check(lib.dmm_mfilter_cov(ctx.handle, nra, nmat, ptr(ra_d), ptr(par_d), ptr(mask_d), ptr(G), ptr(status)))
        _lib.check(lib.dmm_mfilter_eye(ctx.handle, nra, nmat, 0, ptr(mask_d), ptr(out), ptr(status)))
        _lib.check(lib.dmm_mfilter_solve(ctx.handle, nra, nra, nmat, ptr(G), ptr(out), ptr(status)))
        _lib.check(lib.dmm_mfilter_eye(ctx.handle, nra, nmat, 1, ptr(mask_d), ptr(out), ptr(status)))
        bad = status.cpu().numpy()
        ctx.uses(G, mask_d, par_d)
        if bad.any():
            raise np.linalg.LinAlgError(f"{who}: the covariance of mask {m0 + int(np.flatnonzero(bad)[0])} is not positive definite")
    ctx.uses(ra_d)
    index = [np.unravel_index(np.flatnonzero(uindex == uu), flag.shape[:-1]) for uu in range(nuniq)]
    return pinv, index


def bandpass_mmode_filter(ra, m_center, m_cut, flag, epsilon=1e-10):
    """Construct a band-pass m-mode filter with the pass band ``[m_center - m_cut, m_center + m_cut]``
    (``dayenu.py:1235-1293``).

    ``ra [nra]`` in radians, ``flag [..., nra]`` with two or more axes.  Returns ``(pinv, index)``: ``pinv [nuniq, nra,
    nra]`` float64 **on the device**, one filter per unique RA mask, and ``index``, the positions in the leading axes
    of ``flag`` each applies to (``numpy.unravel_index``, as the reference).  ``nra`` outside 1 ... 4096 raises
    ``ValueError``; a matrix that is not positive definite raises ``numpy.linalg.LinAlgError``.
    """
    return _mmode_filter("bandpass_mmode_filter", ra, flag, _mmode_params(np.asarray(ra, dtype=np.float64), "bandpass", m_cut, m_center, epsilon))


def lowpass_mmode_filter(ra, m_cut, flag, epsilon=1e-10):
    """Construct a low-pass m-mode filter with the pass band ``[-m_cut, m_cut]`` (``dayenu.py:1296-1346``); arguments
    and result as :func:`bandpass_mmode_filter`."""
    return _mmode_filter("lowpass_mmode_filter", ra, flag, _mmode_params(np.asarray(ra, dtype=np.float64), "lowpass", m_cut, 0.0, epsilon))


def highpass_mmode_filter(ra, m_cut, flag, epsilon=1e-10):
    """Construct a high-pass m-mode filter with the stop band ``[-m_cut, m_cut]`` (``dayenu.py:1349-1396``); arguments
    and result as :func:`bandpass_mmode_filter`."""
    return _mmode_filter("highpass_mmode_filter", ra, flag, _mmode_params(np.asarray(ra, dtype=np.float64), "highpass", m_cut, 0.0, epsilon))


class DayenuMFilter(ContainerTask):
    """Apply a DAYENU band-pass m-mode filter to a sidereal stream (``dayenu.py:977-1122``).

    Attributes
    ----------
    dec : float
        The pass band is centred on the fringe rate of a source on the meridian at this declination, in degrees.
        Default 40.
    epsilon : float
        The stop-band rejection of the filter.  Default 1e-10.
    fkeep_intra : float
        Width of the pass band for intra-cylinder baselines as a fraction of the cylinder width.  Default 0.75.
    fkeep_inter : float
        The same for inter-cylinder baselines.  Default 0.75.
    workspace_mib : int
        Device memory the matrices and right-hand sides of one batch of frequencies may take.  Default 1024.

    Works in place and returns the input container with device-resident ``vis`` and ``vis_weight``.  Per frequency one
    RA mask serves all baselines (an RA is kept where more than 90 % of the baselines with any weight have weight);
    the weights are multiplied by it and not propagated through the filter.  A frequency whose factorisation fails
    keeps its data and loses its weight.  The telescope must give ``feedpositions``, ``cylinder_spacing`` and
    ``latitude``.
    """

    _config_names = ("dec", "epsilon", "fkeep_intra", "fkeep_inter", "workspace_mib")
    dec = 40.0
    epsilon = 1e-10
    fkeep_intra = 0.75
    fkeep_inter = 0.75
    workspace_mib = 1024

    def setup(self, telescope):
        """Set the telescope needed to obtain baselines."""
        self.telescope = io.get_telescope(telescope)

    def _get_cut(self, freq, xsep):
        """Fringe rate on the meridian at ``dec`` of an east-west separation ``xsep`` (metres) at ``freq`` (MHz)."""
        lmbda = scipy.constants.c / (freq * 1e6)
        u = xsep / lmbda
        return instantaneous_m(0.0, np.radians(self.telescope.latitude), np.radians(self.dec), u, 0.0)

    def process(self, stream):
        """Filter out m-modes from a SiderealStream, in place."""
        stream.redistribute("freq")
        ctx = Context.get()
        lib = _lib.lib
        tel = self.telescope
        spacing = tel.cylinder_spacing
        ra = np.ascontiguousarray(np.radians(stream.ra[:]), dtype=np.float64)
        freq = np.asarray(stream.freq[:], dtype=np.float64)
        prod = stream.prodstack
        vis = _dev_dataset(stream.vis, ctx, np.complex64)
        weight = _dev_dataset(stream.weight, ctx, np.float32)
        nfreq, nstack, nra = (int(s) for s in vis.shape)
        _check_nra(type(self).__name__, nra)
        if len(prod) != nstack or freq.size != nfreq or ra.size != nra:
            raise ValueError(f"{len(prod)} products, {freq.size} frequencies, {ra.size} RAs for a dataset of shape {(nfreq, nstack, nra)}")

        # east-west separation of every stack entry in whole cylinders; the intra-cylinder ones are not fringe-stopped
        baselines = tel.feedpositions[prod["input_a"], 0] - tel.feedpositions[prod["input_b"], 0]
        baselines = np.round(baselines / spacing) * spacing
        db = 0.5 * spacing
        is_intra = np.abs(baselines) < db
        entries = [np.flatnonzero(is_intra).astype(np.int32), np.flatnonzero(~is_intra).astype(np.int32)]

        # per frequency: (diag, coef, m_cut, m_center) of the two kinds and the mixer rates of the inter entries
        par = np.zeros((2, nfreq, 4))
        mix = np.zeros((nfreq, len(entries[1])))
        for ff, nu in enumerate(freq):
            m_cut = np.abs(self._get_cut(nu, db))
            par[0, ff] = _mmode_params(ra, "bandpass", 0.5 * self.fkeep_intra * m_cut, 0.5 * (2.0 - self.fkeep_intra) * m_cut, self.epsilon)
            par[1, ff] = _mmode_params(ra, "lowpass", self.fkeep_inter * m_cut, 0.0, self.epsilon)
            mix[ff] = self._get_cut(nu, baselines[entries[1]])
        check_mmode_eigenvalue_cut(ra, par)

        flag_d = ctx.empty((nfreq, nra), np.uint8)
        state_d = ctx.empty((nfreq,), np.int32)
        _lib.check(lib.dmm_mfilter_mask(ctx.handle, nfreq, nstack, nra, ptr(weight), ptr(flag_d), ptr(state_d)))
        flags, state = flag_d.cpu().numpy(), state_d.cpu().numpy()
        todo = np.flatnonzero(state == _lib.DMM_MFILTER_FILTER).astype(np.int32)
        self.log.debug(f"{nfreq} frequencies, {todo.size} to filter, {int((state == _lib.DMM_MFILTER_UNTOUCHED).sum())} without any weight.")

        ra_d = ctx.to_device(ra)
        entries_d = [ctx.to_device(e) for e in entries]
        per = max(1, min(65535, (int(self.workspace_mib) << 20) // (8 * nra * (nra + 2 * nstack))))
        for b0 in range(0, todo.size, per):
            fs = todo[b0 : b0 + per]
            nmat = fs.size
            fs_d = ctx.to_device(fs)
            mask_d = ctx.to_device(np.ascontiguousarray(flags[fs]))
            G = ctx.empty((nmat, nra, nra), np.float64)
            work = []
            for kind in (0, 1):
                nent = int(entries[kind].size)
                if nent == 0:
                    continue
                par_d = ctx.to_device(np.ascontiguousarray(par[kind, fs]))
                mix_d = ctx.to_device(np.ascontiguousarray(mix[fs])) if kind == 1 else None
                status = ctx.empty((nmat,), np.int32)
                Y = ctx.empty((nmat, 2 * nent, nra), np.float64)
                _lib.check(lib.dmm_mfilter_cov(ctx.handle, nra, nmat, ptr(ra_d), ptr(par_d), ptr(mask_d), ptr(G), ptr(status)))
                _lib.check(lib.dmm_mfilter_pack(ctx.handle, nra, nstack, nmat, nent, ptr(fs_d), ptr(entries_d[kind]), ptr(mix_d), ptr(ra_d), ptr(mask_d), ptr(status), ptr(vis), ptr(Y)))
                _lib.check(lib.dmm_mfilter_solve(ctx.handle, nra, 2 * nent, nmat, ptr(G), ptr(Y), ptr(status)))
                work.append((kind, nent, mix_d, Y, status))
                ctx.uses(par_d, mix_d, Y, status)
            # a frequency is written back only if both of its matrices were factored
            failed = np.zeros(nmat, dtype=np.int32)
            for _, _, _, _, status in work:
                failed |= status.cpu().numpy()
            for i in np.flatnonzero(failed):
                self.log.error(
                    f"Failed to factorise the covariance while processing freq {int(fs[i])} [{freq[fs[i]]:0.3f} MHz]\n"
                    f"Percentage unmasked right ascensions:  {100 * flags[fs[i]].mean():0.1f}"
                )
                weight[int(fs[i])].zero_()
            failed_d = ctx.to_device(failed)
            for kind, nent, mix_d, Y, _ in work:
                _lib.check(lib.dmm_mfilter_unpack(ctx.handle, nra, nstack, nmat, nent, ptr(fs_d), ptr(entries_d[kind]), ptr(mix_d), ptr(ra_d), ptr(mask_d), ptr(failed_d), ptr(Y), ptr(vis)))
            ctx.uses(fs_d, mask_d, G, failed_d)
        ctx.uses(ra_d, flag_d, state_d, *entries_d)
        stream.vis.set_device(vis)
        stream.weight.set_device(weight)
        return stream


__all__ = [
    "DayenuDelayFilter",
    "DayenuDelayFilterHybridVis",
    "DayenuDelayFilterMap",
    "DayenuMFilter",
    "bandpass_mmode_filter",
    "delay_filter",
    "highpass_delay_filter",
    "highpass_mmode_filter",
    "instantaneous_m",
    "lowpass_mmode_filter",
]
