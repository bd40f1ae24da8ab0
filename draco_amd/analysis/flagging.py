"""Flagging of bad or unwanted data on the GPU: m-mode masking ahead of map-making, and the RFI mask tasks.

``MaskMModeData`` is the drop-in for ``draco/analysis/flagging.py:113-173``: same config attributes
(``auto_correlations``, ``m_zero``, ``positive_m``, ``negative_m``, ``mask_low_m``) and the same
in-place semantics (the input container is returned with its weights zeroed).  It sits between
``MModeTransform`` and the map-makers in the reference's real-data pipeline
(``test/pipe_config.yaml:100-131``); the map-makers treat zero weights as "row absent".

The RFI part (``flagging.py:1808-2377`` and ``:3231-3381``): ``RFISensitivityMask``, ``RFIMask`` and
``ApplyTimeFreqMask`` (alias ``ApplyRFIMask``), ``NegativeAutosMask`` (``:666-699``), with the functions ``mad``,
``tv_channels_flag``, ``sigma_to_p``, ``p_to_sigma`` and ``inverse_binom_cdf_prob``; and ``RFIMaskChisqHighDelay``
(``:1425-1805``), the mask from a chi-squared test statistic, whose medians are weighted (``dmm_rfi_wmedfilt``, DESIGN.md
section 7s); and ``RFIVisMask`` / ``RFITransientVisMask`` (``:1042-1277``), the mask made from the visibilities themselves
(``csrc/vismask.hip``).  The planes stay on the device across the iterations of a mask task:
medians, SumThreshold, SIR and the elementwise stages are the kernels of ``csrc/rfi.hip``; only scalars (the TV
thresholds, from SciPy) and the frequency-length arrays of the static channel mask are formed on the host.  The
convention is ``True`` for contaminated samples.
"""

from __future__ import annotations

import copy as _copy
import ctypes as C
import logging

import numpy as np
import torch

from .. import _lib
from ..core import containers, io
from ..core.task import ContainerTask
from ..device import Context, ptr
from ..util import filters, rfi, tools
from ..util.rfi import apply_hysteresis_threshold  # noqa: F401  (the name the reference's module carries)
from . import transform
from .transform import _dev_dataset, axis_reduce_device


def _prodstack(cont):
    """Representative (input_a, input_b) of every stack entry (``containers.py:211-229``)."""
    prod = cont.index_map.get("prod")
    stack = cont.index_map.get("stack")
    if prod is None:
        return None
    if stack is not None and stack.dtype.names is not None and "prod" in stack.dtype.names:
        return prod[stack["prod"]]
    return prod


class MaskMModeData(ContainerTask):
    """Mask out m-mode data ahead of map making (``flagging.py:113-173``).

    Attributes
    ----------
    auto_correlations : bool
        Exclude auto correlations if set (default False: autos ARE masked, as in the reference).
    m_zero : bool
        Ignore the m=0 mode (default False: m=0 is masked).
    positive_m, negative_m : bool
        Include positive / negative m-modes (default True).
    mask_low_m : int, optional
        If set, mask out m's lower than this threshold.
    """

    auto_correlations = False
    m_zero = False
    positive_m = True
    negative_m = True
    mask_low_m = None
    _config_names = ("auto_correlations", "m_zero", "positive_m", "negative_m", "mask_low_m")

    def process(self, mmodes):
        mmodes.redistribute("freq")
        ctx = Context.get()
        mw = _dev_dataset(mmodes.weight, ctx, np.float64)
        n_m, _, nfreq, nstack = mw.shape
        is_auto = None
        if not self.auto_correlations:
            ps = _prodstack(mmodes)
            if ps is None or len(ps) != nstack:
                raise ValueError("MaskMModeData needs the prod/stack index maps to find the auto-correlations")
            is_auto = ctx.to_device((ps["input_a"] == ps["input_b"]).astype(np.uint8))
        _lib.check(
            _lib.lib.dmm_mask_mmode_weight(
                ctx.handle, ptr(mw), int(n_m), int(nfreq), int(nstack), ptr(is_auto), int(bool(self.m_zero)),
                int(bool(self.positive_m)), int(bool(self.negative_m)), int(self.mask_low_m or 0),
            )
        )
        mmodes.weight.set_device(mw)
        return mmodes


# ---------------------------------------------------------------------------------------------------------------
# RFI flagging


def _u8(ctx, mask):
    """A uint8 device plane, 1 where ``mask`` is set (a fresh tensor)."""
    if isinstance(mask, torch.Tensor):
        return mask.to(ctx.device).ne(0).to(torch.uint8).contiguous()
    return ctx.to_device(np.ascontiguousarray(np.asarray(mask) != 0).view(np.uint8))


def _mask_op(ctx, op, a, b, c=None, out=None):
    out = torch.empty_like(a) if out is None else out
    _lib.check(_lib.lib.dmm_rfi_mask_op(ctx.handle, op, ptr(a), ptr(b), ptr(c), a.numel(), ptr(out)))
    return out


def _or_into(ctx, a, b):
    """``a |= b`` on the device."""
    return _mask_op(ctx, _lib.DMM_RFI_OR, a, b, out=a)


def _absdev(ctx, y, med, y_imag=None, med_imag=None, want_dy=True):
    dy = torch.empty_like(y) if want_dy else None
    ady = torch.empty_like(y)
    _lib.check(_lib.lib.dmm_rfi_absdev(ctx.handle, ptr(y), ptr(med), ptr(y_imag), ptr(med_imag), y.numel(), ptr(dy), ptr(ady)))
    return dy, ady


def _nsigma(ctx, ady, mad_, scale, nsigma, divide=False, nan_fill=float("nan"), want_var=False, want_mask=True):
    ratio = torch.empty_like(ady)
    var = torch.empty_like(ady) if want_var else None
    mask = torch.empty(ady.shape, dtype=torch.uint8, device=ady.device) if want_mask else None
    _lib.check(
        _lib.lib.dmm_rfi_nsigma(ctx.handle, ptr(ady), ptr(mad_), float(scale), float(nsigma), float(nan_fill), int(bool(divide)), ady.numel(), ptr(ratio), ptr(var), ptr(mask))
    )
    return ratio, var, mask


def mad(x, mask, base_size=(11, 3), mad_size=(21, 21), debug=False, sigma=True):
    """Deviation of every sample of a ``[freq, time]`` plane from its local median, in units of the local MAD.

    Two masked moving medians (``filters.medfilt``): one of ``base_size`` gives the baseline, one of ``mad_size`` over
    ``|x - baseline|`` the scale, multiplied by 1.4826 when ``sigma`` asks for Gaussian sigmas.  The quotient is NaN
    where a window held no sample.  Complex planes are filtered part by part and the modulus taken.  ``debug`` adds
    the deviation and the scale to the result.  The kind that goes in comes out: NumPy arrays or device tensors.
    """
    on_device = isinstance(x, torch.Tensor)
    windows = filters.check_size(base_size, 2), filters.check_size(mad_size, 2)
    ctx = Context.get()
    out = _mad_device(ctx, x if on_device else np.asarray(x), _u8(ctx, mask), *windows, sigma)
    if not on_device:
        out = tuple(t.cpu().numpy() for t in out)
    return out if debug else out[0]


def _mad_device(ctx, x, flag, base_size, mad_size, sigma=True, nan_fill=float("nan"), nsigma=None):
    """``(ratio, deviation, scale)`` of a plane on the device; with ``nsigma`` the first entry is the pair ``(ratio,
    ratio > nsigma)``.  ``nan_fill``: what a NaN ratio is replaced by (NaN: kept)."""
    parts = [x.real, x.imag] if (x.is_complex() if isinstance(x, torch.Tensor) else np.iscomplexobj(x)) else [x]
    parts = [ctx.to_device(p, np.float64) for p in parts]
    base = [filters.medfilt_device(ctx, p, flag, base_size) for p in parts]
    if len(parts) == 2:
        _, dev = _absdev(ctx, parts[0], base[0], parts[1], base[1], want_dy=False)
    else:
        _, dev = _absdev(ctx, parts[0], base[0], want_dy=False)
    scale = filters.medfilt_device(ctx, dev, flag, mad_size)
    factor = 1.4826 if sigma else 1.0
    ratio, _, over = _nsigma(ctx, dev, scale, factor, 0.0 if nsigma is None else nsigma, divide=True, nan_fill=nan_fill, want_mask=nsigma is not None)
    if sigma:
        scale = scale * factor
    return (ratio if nsigma is None else (ratio, over)), dev, scale


def inverse_binom_cdf_prob(k, N, F):
    """The success probability ``p`` at which a binomial of ``N`` trials has ``Pr(X <= k) = F``, through the
    incomplete beta function that the binomial's cumulative distribution is."""
    from scipy.special import betaincinv

    return betaincinv(k + 1, N - k, 1 - F)


def sigma_to_p(sigma):
    """Two-sided tail probability of a Gaussian beyond ``sigma``."""
    from scipy.stats import norm

    return 2 * norm.sf(sigma)


def p_to_sigma(p):
    """The inverse of :func:`sigma_to_p`."""
    from scipy.stats import norm

    return norm.isf(p / 2)


class _TVBands:
    """The 6 MHz digital-TV bands (67 of them, from 398 MHz up) that a frequency axis touches.

    A row belongs to every band its channel, of the axis' median spacing, overlaps; the fraction it finally carries is
    that of the last such band, because the reference writes the bands in ascending order.  Rows, band membership in
    CSR form and that last-band index are device tables built once per frequency axis.
    """

    first_mhz, width_mhz, nband = 398, 6, 67

    def __init__(self, ctx, freq):
        freq = np.asarray(freq, dtype=np.float64)
        half = 0.5 * np.median(np.abs(np.diff(freq)))
        edges = self.first_mhz + self.width_mhz * np.arange(self.nband + 1)
        member = (freq[None, :] + half >= edges[:-1, None]) & (freq[None, :] - half <= edges[1:, None])  # [band, row]
        member = member[member.any(axis=1)]  # bands without a row are not looked at
        self.counts = [int(n) for n in member.sum(axis=1)]
        keeps = np.full(len(freq), -1, dtype=np.int32)
        for b, rows in enumerate(member):
            keeps[rows] = b
        offsets = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int32)
        self.nrows = int(offsets[-1])
        self.row_chan = ctx.to_device(keeps)
        self.chan_ptr = ctx.to_device(offsets)
        self.chan_rows = ctx.to_device(np.nonzero(member)[1].astype(np.int32)) if self.nrows else None

    def thresholds(self, sigma, f):
        """Per band of N rows the level that more than ``int(f N)`` of N Gaussian samples exceed with the two-sided
        probability of ``sigma`` only (host scalars, from SciPy)."""
        p_false = sigma_to_p(sigma)
        return np.array([p_to_sigma(inverse_binom_cdf_prob(int(f * n), n, 1 - p_false)) for n in self.counts], dtype=np.float64)

    def flag(self, ctx, x, sigma, f, want_frac=False):
        """``(mask, fractions or None)`` of a float64 ``[freq, time]`` device plane."""
        nf, nt = (int(s) for s in x.shape)
        levels = self.thresholds(sigma, f)
        levels_d = ctx.to_device(levels) if len(levels) else None
        frac = torch.empty(x.shape, dtype=torch.float32, device=x.device) if want_frac else None
        mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        _lib.check(
            _lib.lib.dmm_rfi_tv_flag(
                ctx.handle, ptr(x), nf, nt, ptr(self.row_chan), len(self.counts), ptr(self.chan_ptr), ptr(self.chan_rows), self.nrows, ptr(levels_d), float(f), ptr(frac), ptr(mask)
            )
        )
        return mask, frac


def tv_channels_flag(x, freq, sigma=5, f=0.5, debug=False):
    """Flag whole digital-TV bands in which many samples are mildly high.

    ``x [freq, time]`` holds deviations in sigmas and ``freq`` the channel centres in MHz.  Per band and time sample
    the fraction of rows above the band's level (:meth:`_TVBands.thresholds`) is formed; rows of a band whose fraction
    exceeds ``f`` are flagged, and rows outside every band carry the fraction 1.  ``debug`` returns the float32
    fractions beside the mask.  Counting and comparison are ``dmm_rfi_tv_flag``.
    """
    on_device = isinstance(x, torch.Tensor)
    ctx = Context.get()
    plane = ctx.to_device(x if on_device else np.asarray(x), np.float64)
    if plane.dim() != 2 or plane.shape[0] != len(freq):
        raise ValueError(f"x {tuple(plane.shape)} is not [freq, time] with {len(freq)} frequencies")
    mask, frac = _TVBands(ctx, freq).flag(ctx, plane, sigma, f, want_frac=debug)
    mask = mask.ne(0)
    if not on_device:
        mask, frac = mask.cpu().numpy(), (frac.cpu().numpy() if debug else None)
    return (mask, frac) if debug else mask


class RFISensitivityMask(ContainerTask):
    """RFI mask from the ratio of the measured to the radiometer sensitivity (drop-in for ``flagging.py:1808-2117``).

    Config (names and defaults are the reference's):

    ``mask_type`` ("combine")
        "mad", "sumthreshold", or "combine": SumThreshold except where ``_combine_st_mad_hook`` selects the MAD mask.
    ``include_pol`` (None)
        polarisations to process; the others contribute nothing to the mask.  None: all.
    ``nsigma_1d`` (5.0), ``quantile_1d`` (0.15), ``win_f_1d`` (191)
        the channel test ahead of the iterations: a channel is dropped when its ``quantile_1d`` over time lies more
        than ``nsigma_1d`` scaled MADs from the median over ``win_f_1d`` neighbouring channels (None: over all
        channels).  ``nsigma_1d = None`` skips the test.
    ``nsigma`` (5.0), ``niter`` (5), ``rho`` (1.5)
        the threshold of the last of ``niter`` passes; every earlier pass is looser by another factor ``rho``.
    ``base_size`` (37, 181), ``mad_size`` (101, 31)
        (freq, time) windows of the baseline median and of the MAD.
    ``tv_fraction`` (0.5), ``max_m`` (64)
        as ``f`` of :func:`tv_channels_flag` and ``max_m`` of ``rfi.sumthreshold``.
    ``sir`` (False), ``eta`` (0.2), ``only_time`` (False)
        SIR over the final mask, its aggressiveness, and whether it runs along time only.
    """

    mask_type = "combine"
    include_pol = None
    nsigma_1d = 5.0
    quantile_1d = 0.15
    win_f_1d = 191
    nsigma = 5.0
    niter = 5
    rho = 1.5
    base_size = (37, 181)
    mad_size = (101, 31)
    tv_fraction = 0.5
    max_m = 64
    sir = False
    eta = 0.2
    only_time = False
    _config_names = ("mask_type", "include_pol", "nsigma_1d", "quantile_1d", "win_f_1d", "nsigma", "niter", "rho", "base_size", "mad_size", "tv_fraction", "max_m", "sir",
                     "eta", "only_time")

    MAD_TO_RMS = 1.4826  # a Gaussian's standard deviation in units of its MAD

    def read_config(self, params):
        params = dict(params)
        nullable = {k: params.pop(k) for k in ("nsigma_1d", "win_f_1d") if k in params and params[k] is None}
        super().read_config(params)
        for k, v in nullable.items():
            setattr(self, k, v)
        if self.mask_type not in ("mad", "sumthreshold", "combine"):
            raise ValueError(f"mask_type must be 'mad', 'sumthreshold' or 'combine', not {self.mask_type!r}")
        for name in ("base_size", "mad_size"):
            size = tuple(int(s) for s in getattr(self, name))
            if len(size) != 2:
                raise ValueError(f"{name} must have two entries, got {size}")
            setattr(self, name, size)

    def setup(self):
        """The threshold of every pass: ``nsigma`` for the last, a factor ``rho`` more for each one before it."""
        loosened = np.arange(self.niter - 1, -1, -1)  # how many factors of rho each pass is above the last
        self.threshold = self.nsigma * self.rho**loosened

    def process(self, sensitivity):
        """``containers.SystemSensitivity`` -> ``containers.RFIMask``, the OR over the processed polarisations."""
        if not hasattr(self, "threshold"):
            self.setup()
        sensitivity.redistribute("pol")
        ctx = Context.get()
        freq, time = sensitivity.freq, sensitivity.time
        static = ~np.asarray(self._static_rfi_mask_hook(freq, time[0]), dtype=bool)  # the hook answers "keep"
        planes = self._radiometer_planes(ctx, sensitivity)
        nfreq, ntime = (int(s) for s in planes[0].shape[1:])
        state = {
            "ctx": ctx,
            "windows": (filters.check_size(self.base_size, 2), filters.check_size(self.mad_size, 2)),
            "static": _u8(ctx, static),
            "tv": _TVBands(ctx, freq),
            "use_mad": None,
        }
        if self.mask_type == "combine":
            state["use_mad"] = _u8(ctx, np.broadcast_to(np.asarray(self._combine_st_mad_hook(time, freq), dtype=bool), (nfreq, ntime)))

        total = torch.zeros((nfreq, ntime), dtype=torch.uint8, device=ctx.device)
        for p, name in enumerate(sensitivity.pol):
            if self.include_pol and name not in self.include_pol:
                continue
            _or_into(ctx, total, self._flag_polarisation(state, planes[0][p], planes[1][p]))

        mask = total.cpu().numpy().astype(bool)
        self._report("RFISensitivityMask", mask)
        if self.sir:
            mask = self._apply_sir(mask, static)
            self._report("SIR operator", mask)
        out = containers.RFIMask(axes_from=sensitivity, attrs_from=sensitivity)
        out.mask[:] = mask
        return out

    def _report(self, stage, mask):
        self.log.info(f"After {stage}, {100.0 * mask.mean() if mask.size else 0.0:0.2f} percent of data will be masked.")

    def _radiometer_planes(self, ctx, sensitivity):
        """``(y, flag)``, both ``[pol, freq, time]`` on the device: the float32 ratio measured / radiometer (0 where
        the radiometer estimate is 0) widened to float64, and where the weight is zero."""
        meas, radm, wgt = (_dev_dataset(ds, ctx, np.float32) for ds in (sensitivity.measured, sensitivity.radiometer, sensitivity.weight))
        nfreq, npol, ntime = (int(s) for s in meas.shape)
        y = torch.empty((npol, nfreq, ntime), dtype=torch.float64, device=ctx.device)
        flag = torch.empty((npol, nfreq, ntime), dtype=torch.uint8, device=ctx.device)
        _lib.check(_lib.lib.dmm_rfi_radiometer(ctx.handle, ptr(meas), ptr(radm), ptr(wgt), nfreq, npol, ntime, ptr(y), ptr(flag)))
        return y, flag

    def _flag_polarisation(self, state, y, flag):
        """All passes over one polarisation's plane.  ``y`` and ``flag`` are updated in place; nothing but scalars
        crosses to the host inside the loop."""
        ctx = state["ctx"]
        nfreq, ntime = (int(s) for s in y.shape)
        _lib.check(_lib.lib.dmm_rfi_rows(ctx.handle, None, ptr(flag), None, ptr(state["static"]), nfreq, ntime))
        if self.nsigma_1d is not None:  # drop outlying channels and take each channel's level out of the plane
            bad, level = self._mask_1d(y, flag)
            bad = bad.to(torch.uint8)
            _lib.check(_lib.lib.dmm_rfi_rows(ctx.handle, ptr(y), ptr(flag), ptr(level), ptr(bad), nfreq, ntime))
        for nsigma in self.threshold:
            _or_into(ctx, flag, self._one_pass(state, y, flag, float(nsigma)))
        return flag

    def _one_pass(self, state, y, flag, nsigma):
        """What one pass at threshold ``nsigma`` adds to ``flag`` (a new plane)."""
        ctx = state["ctx"]
        base_size, mad_size = state["windows"]
        dy, ady = _absdev(ctx, y, filters.medfilt_device(ctx, y, flag, base_size))
        spread = filters.medfilt_device(ctx, ady, flag, mad_size)
        # ratio = ady * invert_no_zero(MAD_TO_RMS * spread); its test against nsigma; the variance SumThreshold takes
        ratio, variance, by_mad = _nsigma(ctx, ady, spread, self.MAD_TO_RMS, nsigma, want_var=self.mask_type != "mad")
        tvmask, _ = state["tv"].flag(ctx, ratio, nsigma, self.tv_fraction)
        _or_into(ctx, by_mad, tvmask)
        if self.mask_type == "mad":
            return by_mad
        by_st = _mask_op(ctx, _lib.DMM_RFI_OR, flag, tvmask)  # SumThreshold starts from everything known so far
        rfi.sumthreshold_device(ctx, dy, by_st, self.max_m, nsigma, 1.0, (1, 0), variance=variance, correct_for_missing=True)
        if self.mask_type == "sumthreshold":
            return by_st
        mixed = _mask_op(ctx, _lib.DMM_RFI_SELECT, by_mad, by_st, state["use_mad"])
        if not self.sir:
            # no SIR at the end: the stretches given to the MAD mask get one along time here (eta 0.2, as the
            # reference has it), which carries SumThreshold's flags from either side across them
            grown = rfi.sir_device(ctx, mixed, 0.2, 1)
            _mask_op(ctx, _lib.DMM_RFI_SELECT, grown, mixed, state["use_mad"], out=mixed)
        return mixed

    def _combine_st_mad_hook(self, times, freq):
        """Hook for subclasses: where "combine" takes the MAD mask (True) and where the SumThreshold mask (False), as
        a Boolean ``[nfreq, ntime]`` array.  ``times`` are UNIX seconds, ``freq`` MHz.  The default takes the MAD mask
        everywhere; a subclass marks the transits of bright sources, where SumThreshold eats signal."""
        return np.full((len(freq), len(times)), True)

    def _static_rfi_mask_hook(self, freq, timestamp=None):
        """Hook for subclasses: the channels to keep, ``[nfreq]`` Boolean (False drops a channel for the whole day).
        ``timestamp`` is the first time sample.  The default keeps all."""
        return np.full(np.shape(freq), True)

    def _mask_1d(self, rad, mask):
        """The channel test: ``(bad [nfreq], level [nfreq])`` with ``level`` the ``quantile_1d`` of every channel over
        its unflagged samples.  Quantiles and the medians over frequency run on the device; the last comparison, on
        ``nfreq`` numbers, is NumPy's.  Device tensors in, device tensors out; arrays in, arrays out."""
        on_device = isinstance(rad, torch.Tensor)
        ctx = Context.get()
        y = ctx.to_device(rad if on_device else np.asarray(rad), np.float64)
        flag = mask if (isinstance(mask, torch.Tensor) and mask.dtype == torch.uint8) else _u8(ctx, mask)
        nfreq = int(y.shape[0])
        level_d, kept = filters.quantile_device(ctx, y, flag, self.quantile_1d, count=True)
        empty = kept.eq(0).to(torch.uint8)  # channels with no sample take no part in the medians

        def over_freq(v):
            if self.win_f_1d is None:
                return filters.quantile_device(ctx, v.reshape(1, nfreq), empty.reshape(1, nfreq), 0.5).cpu().numpy()[0]
            window = filters.check_size(self.win_f_1d, 1)
            return filters.medfilt_device(ctx, v.reshape(nfreq, 1), empty.reshape(nfreq, 1), window).reshape(nfreq).cpu().numpy()

        level = level_d.cpu().numpy()
        offset = np.abs(level - over_freq(level_d))
        scale = self.MAD_TO_RMS * over_freq(ctx.to_device(offset))
        with np.errstate(invalid="ignore"):
            bad = offset > (self.nsigma_1d * scale)
        if on_device:
            return ctx.to_device(bad.view(np.uint8)).ne(0), level_d
        return bad, level

    def _apply_sir(self, mask, baseflag, eta=0.2):
        """``mask`` grown by SIR (``self.eta``; along time only with ``only_time``).  Channels in ``baseflag [nfreq]``
        do not seed the growth, or a statically dropped band would spread; they stay masked in the result."""
        seed = mask & ~np.asarray(baseflag, dtype=bool)[:, None]
        along = (-1,) if self.only_time else (0, -1)
        return mask | rfi.scale_invariant_rank(seed, eta=self.eta, axis=along)


class RFIMaskChisqHighDelay(ContainerTask):
    """Mask frequencies and times with an anomalous chi-squared test statistic (drop-in for ``flagging.py:1425-1805``).

    The input holds a chi-squared per degree of freedom in its visibility (or map) dataset and the number of degrees of
    freedom in its weight, as ``ReduceChisq`` leaves them after a delay filter.  Every axis that is neither frequency
    nor time / RA (nor ``pol`` with ``separate_pol``) is averaged away with the weights; then whole channels are dropped
    whose median over time lies far from a smooth baseline over frequency (``mask_1d``), and samples that lie far from
    the weighted moving median of the plane (``mask_2d``, or ``mask_2d_sumthreshold``).

    Config (names and defaults are the reference's):

    ``flag_ew`` (None)
        multiplied into the weights along an ``ew`` axis before the average.
    ``reg_arpls`` (1e5), ``nsigma_1d`` (5.0)
        smoothness of the baseline over frequency, and the cut of the channel test in scaled MADs (0: no test).
    ``win_t`` (601), ``win_f`` (1), ``nsigma_2d`` (5.0)
        the window of the moving median, and the cut in expected standard deviations ``sqrt(2 / ndof)`` (0: no test).
    ``estimate_var`` (False)
        scale the deviations by their own moving MAD over the same window.
    ``only_positive`` (False), ``separate_pol`` (False)
        flag positive excursions only; one mask per polarisation.
    ``mask_type`` ("mad"), ``niter`` (5), ``rho`` (1.5), ``max_m`` (32)
        "mad" or "sumthreshold"; for the latter the passes, the factor between their thresholds, the largest window.

    The collapse is ``dmm_axis_reduce``, the medians ``dmm_rfi_quantile`` and ``dmm_rfi_wmedfilt``; the plane stays on
    the device across the iterations.  Only the baseline fit over the frequency axis (``tools.arPLS_1d``) and the hooks
    run on the host.  An empty row's median enters the baseline fit as 0.0 (it carries no weight there); an empty
    moving window gives NaN, and a NaN deviation is not flagged by the comparison.
    """

    flag_ew = None
    reg_arpls = 1e5
    nsigma_1d = 5.0
    win_t = 601
    win_f = 1
    nsigma_2d = 5.0
    estimate_var = False
    only_positive = False
    separate_pol = False
    mask_type = "mad"
    niter = 5
    rho = 1.5
    max_m = 32
    _config_names = ("flag_ew", "reg_arpls", "nsigma_1d", "win_t", "win_f", "nsigma_2d", "estimate_var", "only_positive", "separate_pol", "mask_type", "niter", "rho",
                     "max_m")

    MAD_TO_RMS = 1.48625  # as the reference writes it here

    telescope = None

    def read_config(self, params):
        super().read_config(params)
        if self.mask_type not in ("mad", "sumthreshold"):
            raise ValueError(f"mask_type must be 'mad' or 'sumthreshold', not {self.mask_type!r}")
        if self.flag_ew is not None:
            self.flag_ew = np.asarray(self.flag_ew)

    def setup(self, telescope=None):
        """``telescope``: only used to convert (LSD, RA) to UNIX time for sidereal streams."""
        self.telescope = None if telescope is None else io.get_telescope(telescope)
        if self.mask_type == "sumthreshold":
            self.threshold = self.nsigma_2d * self.rho ** np.arange(self.niter)[::-1]

    def process(self, stream):
        """``TimeStream | SiderealStream | HybridVisStream | RingMap`` -> ``RFIMask | SiderealRFIMask | RFIMaskByPol |
        SiderealRFIMaskByPol``, True where a sample is flagged."""
        if self.mask_type == "sumthreshold" and not hasattr(self, "threshold"):
            self.setup(self.telescope)
        stream.redistribute("freq")
        freq = stream.freq
        sidereal = "ra" in stream.index_map

        multiple_days = False
        if sidereal:
            if self.telescope is None:
                raise RuntimeError("For sidereal streams, must provide telescope object during setup.")
            csd = stream.attrs.get("lsd", stream.attrs.get("csd"))
            if csd is None:
                raise ValueError("Data does not have a `csd` or `lsd` attribute.")
            if not np.isscalar(csd):
                csd = np.floor(np.mean(csd))
                multiple_days = True
            timestamp = self.telescope.lsd_to_unix(csd + stream.ra / 360.0)
        else:
            timestamp = stream.time

        ctx = Context.get()
        data = stream.datasets["vis" if "vis" in stream.datasets else "map"]
        dax = list(data.attrs["axis"])
        separate_pol = bool(self.separate_pol) and "pol" in dax
        chisq, wsum = self._collapse(ctx, stream, data, dax, separate_pol)  # [(pol,) freq, time] float64
        nfreq, ntime = (int(s) for s in chisq.shape[-2:])
        mask_input = wsum.eq(0.0).to(torch.uint8)

        if multiple_days:
            mask_daytime = np.zeros(timestamp.size, dtype=bool)
        else:
            mask_daytime = np.asarray(self._day_flag_hook(timestamp), dtype=bool)
        mask_sources = _u8(ctx, np.broadcast_to(np.asarray(self._source_flag_hook(timestamp, freq), dtype=bool), (nfreq, ntime)))
        day_rows = _u8(ctx, np.broadcast_to(mask_daytime, (nfreq, ntime)))

        if separate_pol:
            kind = containers.SiderealRFIMaskByPol if sidereal else containers.RFIMaskByPol
        else:
            kind = containers.SiderealRFIMask if sidereal else containers.RFIMask
        output = kind(axes_from=stream, attrs_from=stream, allocate=False)

        planes = []
        for p in range(chisq.shape[0] if separate_pol else 1):
            y, ws, m_in = (chisq[p], wsum[p], mask_input[p]) if separate_pol else (chisq, wsum, mask_input)
            mask = _mask_op(ctx, _lib.DMM_RFI_OR, m_in.contiguous(), mask_sources)
            result = torch.zeros((nfreq, ntime), dtype=torch.uint8, device=ctx.device)
            if self.nsigma_1d > 0.0:
                rows = self.mask_1d(y, _mask_op(ctx, _lib.DMM_RFI_OR, mask, day_rows)).to(torch.uint8)
                _lib.check(_lib.lib.dmm_rfi_rows(ctx.handle, None, ptr(mask), None, ptr(rows), nfreq, ntime))
                _lib.check(_lib.lib.dmm_rfi_rows(ctx.handle, None, ptr(result), None, ptr(rows), nfreq, ntime))
            if self.nsigma_2d > 0.0:
                # the inverse variance of a chi-squared per degree of freedom is ndof / 2, and ndof is the weight
                w = mask.eq(0).to(torch.float64) * ws / 2.0
                found = self.mask_2d(y, w) if self.mask_type == "mad" else self.mask_2d_sumthreshold(y, w)
                _or_into(ctx, result, found.to(torch.uint8) * day_rows.eq(0).to(torch.uint8))
            planes.append(result)
        total = torch.stack(planes) if separate_pol else planes[0]
        output.attach("mask", total.view(torch.bool))
        return output

    def _collapse(self, ctx, stream, data, dax, separate_pol):
        """The weighted average of the real part of the data over every axis but frequency, time / RA and, if kept,
        polarisation: ``(chisq, wsum)``, float64 on the device.  The weight is broadcast along the axes it lacks, so
        ``wsum`` counts every sample of them: the reference's factor on the summed weight is in the sum.  The reduced axes are brought together first (a copy, when the dataset does not hold them adjacent with
        the time-like axis last)."""
        weight = stream.weight
        wax = list(weight.attrs["axis"])
        x = data.device(ctx)
        if x.dtype not in (torch.float32, torch.float64, torch.complex64, torch.complex128):
            raise TypeError(f"the data must be real or complex floating point, got {x.dtype}")
        w = weight.device(ctx)
        w = w.reshape([w.shape[wax.index(ax)] if ax in wax else 1 for ax in dax])
        if self.flag_ew is not None and "ew" in dax:
            few = ctx.to_device(np.asarray(self.flag_ew), np.dtype(weight.dtype)).reshape([-1 if ax == "ew" else 1 for ax in dax])
            w = w * few
        keep = ["freq", "time", "ra"] + (["pol"] if separate_pol else [])
        timelike = [i for i, ax in enumerate(dax) if ax in ("time", "ra")]
        lead = [i for i, ax in enumerate(dax) if ax in keep and i not in timelike]
        red = [i for i, ax in enumerate(dax) if ax not in keep]
        order = lead + red + timelike
        if order != list(range(len(dax))):
            x = x.permute(order).contiguous()
            w = w.expand(*data.shape).permute(order) if w.dim() else w
        shape = [int(s) for s in x.shape]
        if not red:  # nothing to average: one reduced sample per column
            x, w = x.unsqueeze(len(lead)), w.unsqueeze(len(lead))
            red = [0]
        first = len(lead)
        chisq, wsum = axis_reduce_device(ctx, _lib.DMM_REDUCE_WMEAN, x, w, first, first + len(red) - 1)
        kept = [shape[i] for i in range(len(lead))] + [shape[-1]]
        return chisq.reshape(kept), wsum.reshape(kept)

    def mask_1d(self, y, m):
        """Frequency channels whose median chi-squared over time deviates from the neighbouring channels.

        ``y [nfreq, ntime]``: chi-squared per degree of freedom; ``m``: the samples to ignore in the median over time.
        Returns the Boolean ``[nfreq]``.  Device tensors in, a device tensor out; arrays in, an array out.  The row
        medians and the MAD are ``dmm_rfi_quantile``; the baseline fit runs on the host."""
        on_device = isinstance(y, torch.Tensor)
        ctx = Context.get()
        yd = ctx.to_device(y if on_device else np.asarray(y), np.float64)
        flag = m if (isinstance(m, torch.Tensor) and m.dtype == torch.uint8) else _u8(ctx, m)
        nfreq = int(yd.shape[0])
        med_d, kept = filters.quantile_device(ctx, yd, flag.contiguous(), 0.5, count=True)
        med_m = kept.cpu().numpy() == 0
        med_y = np.where(med_m, 0.0, med_d.cpu().numpy())  # (an empty row has no median: any finite value does)
        baseline = tools.arPLS_1d(med_y, mask=med_m, lam=self.reg_arpls)
        abs_dev = np.where(med_m, 0.0, np.abs(med_y - baseline))
        spread = filters.quantile_device(ctx, ctx.to_device(abs_dev).reshape(1, nfreq), _u8(ctx, med_m).reshape(1, nfreq), 0.5).cpu().numpy()[0]
        scale = self.MAD_TO_RMS * (0.0 if np.isnan(spread) else spread)
        bad = abs_dev > (self.nsigma_1d * scale)
        return ctx.to_device(bad.view(np.uint8)).ne(0) if on_device else bad

    def _planes(self, y, w):
        ctx = Context.get()
        on_device = isinstance(y, torch.Tensor)
        yd = ctx.to_device(y if on_device else np.asarray(y), np.float64)
        wd = ctx.to_device(w if isinstance(w, torch.Tensor) else np.asarray(w), np.float64)
        return ctx, on_device, yd, wd, filters.check_weighted_size((self.win_f, self.win_t), 2)

    def _deviation(self, ctx, y, w, f, size):
        """``(dy, |dy|)`` with ``dy = (y - median) sqrt(w)``, the median weighted by ``f``."""
        med = filters.moving_weighted_median_device(ctx, y, f, size)
        dy, ady = torch.empty_like(y), torch.empty_like(y)
        _lib.check(_lib.lib.dmm_rfi_wdev(ctx.handle, ptr(y), ptr(med), ptr(w), y.numel(), ptr(dy), ptr(ady)))
        return dy, ady

    def mask_2d(self, y, w):
        """Samples whose chi-squared deviates from the local weighted median.

        ``y [nfreq, ntime]``: chi-squared per degree of freedom; ``w``: its inverse variance, zero for samples
        already masked.  Returns the Boolean plane; device tensors in, a device tensor out."""
        ctx, on_device, y, w, size = self._planes(y, w)
        dy, ady = self._deviation(ctx, y, w, w, size)
        if self.estimate_var:
            spread = filters.moving_weighted_median_device(ctx, ady, w.gt(0.0).to(torch.float64), size)
        else:
            spread = torch.ones_like(y)
        scale = self.MAD_TO_RMS if self.estimate_var else 1.0
        _, _, mask = _nsigma(ctx, dy if self.only_positive else ady, spread, scale, self.nsigma_2d)
        mask = mask.ne(0)
        return mask if on_device else mask.cpu().numpy()

    def mask_2d_sumthreshold(self, y, w):
        """The same by SumThreshold, iterated: every pass re-estimates the median (and the variance) with the mask so
        far and lowers the threshold by ``rho``.  Arguments and result as :meth:`mask_2d`."""
        if not hasattr(self, "threshold"):
            self.setup(self.telescope)
        ctx, on_device, y, w, size = self._planes(y, w)
        flag = w.eq(0.0).to(torch.uint8)
        ones = torch.ones_like(y)
        for nsigma in self.threshold:
            f = flag.eq(0).to(torch.float64) * w
            dy, ady = self._deviation(ctx, y, w, f, size)
            if self.estimate_var:
                spread = filters.moving_weighted_median_device(ctx, ady, f.gt(0.0).to(torch.float64), size)
                _, variance, _ = _nsigma(ctx, ady, spread, self.MAD_TO_RMS, float(nsigma), want_var=True, want_mask=False)
            else:
                variance = ones
            rfi.sumthreshold_device(ctx, dy, flag, self.max_m, float(nsigma), 1.0, (1, 0), variance=variance, correct_for_missing=True, only_positive=self.only_positive)
        mask = flag.ne(0)
        return mask if on_device else mask.cpu().numpy()

    def _source_flag_hook(self, times, freq):
        """Hook for subclasses: bright point sources to leave out, Boolean ``[nfreq, ntime]`` (True masks a sample)."""
        return np.zeros((freq.size, times.size), dtype=bool)

    def _day_flag_hook(self, times):
        """Hook for subclasses: the daytime samples, Boolean ``[ntime]``: they take no part in the channel test and are
        not flagged by the 2-D test."""
        return np.zeros(times.size, dtype=bool)


class RFIVisMask(ContainerTask):
    """Identify and flag RFI in visibility data: the non-functional base class (drop-in for ``flagging.py:1042-1188``).

    Config: ``stokes_i`` (True): flag on the instrumental Stokes-I visibilities (``transform.stokes_I``, a quarter of
    the baselines) rather than on every stack entry.

    ``process`` turns a ``TimeStream`` into an ``RFIMask`` and a ``SiderealStream`` into a ``SiderealRFIMask``; what
    the mask is made of is :meth:`generate_mask`, which a subclass supplies.  Visibilities, weights and the initial
    mask are device tensors.
    """

    stokes_i = True
    _config_names = ("stokes_i",)

    SPEED_OF_LIGHT = 299792458.0  # m / s

    telescope = None

    def setup(self, telescope):
        """``telescope``: the baselines, the latitude and the time maps are read from it."""
        self.telescope = io.get_telescope(telescope)

    def process(self, stream):
        """``TimeStream | SiderealStream`` with axes frequency, stack and time / RA -> ``RFIMask | SiderealRFIMask``,
        True where a sample is flagged."""
        stream.redistribute("freq")
        if "time" in stream.index_map:
            times = stream.time
            out = containers.RFIMask(axes_from=stream, attrs_from=stream, allocate=False)
        elif "ra" in stream.index_map:
            csd = stream.attrs.get("lsd", stream.attrs.get("csd"))
            if csd is None:
                raise ValueError("Dataset does not have a `csd` or `lsd` attribute.")
            times = self.telescope.lsd_to_unix(csd + stream.ra / 360.0)
            out = containers.SiderealRFIMask(axes_from=stream, attrs_from=stream, allocate=False)
        else:
            raise TypeError(f"Expected data with `time` or `ra` axis. Got {type(stream)}.")

        ctx = Context.get()
        freq = stream.freq
        if self.stokes_i:
            vis, weight, baselines = transform.stokes_I(stream, self.telescope)
        else:
            vis = _dev_dataset(stream.vis, ctx, np.complex64).contiguous()
            weight = _dev_dataset(stream.weight, ctx, np.float32).contiguous()
            baselines = self.telescope.baselines

        mask = weight.eq(0).all(dim=1).to(torch.uint8)
        static = np.asarray(self._static_rfi_mask_hook(freq, times[0]), dtype=bool)
        _lib.check(_lib.lib.dmm_rfi_rows(ctx.handle, None, ptr(mask), None, ptr(_u8(ctx, static)), int(mask.shape[0]), int(mask.shape[1])))
        if self.log.isEnabledFor(logging.DEBUG):
            self.log.debug(f"{100.0 * float(mask.float().mean()):.2f}% of data initially flagged.")

        result = self.generate_mask(vis, weight, mask, freq, baselines, times)
        result = result if isinstance(result, torch.Tensor) else ctx.to_device(np.ascontiguousarray(np.asarray(result, dtype=bool)).view(np.uint8))
        out.attach("mask", result.ne(0) if result.dtype != torch.bool else result)
        return out

    def generate_mask(self, vis, weight, mask, freq, baselines, times):
        """The time-frequency mask, ``[nfreq, ntime]`` (a device tensor or an array), True masking a sample.

        ``vis``, ``weight [nfreq, nstack, ntime]``: complex64 / float32 device tensors; ``mask [nfreq, ntime]``: the
        initial mask, a uint8 device tensor; ``freq`` in MHz; ``baselines [nstack, 2]`` in metres; ``times``: UNIX
        seconds.  Not implemented in the base class.
        """
        raise NotImplementedError

    def _static_rfi_mask_hook(self, freq, timestamp=None):
        """Hook for subclasses: the channels to mask for the whole stream, ``[nfreq]`` Boolean (True masks a channel).
        ``timestamp`` is the first time sample.  The default masks none."""
        return np.zeros_like(freq, dtype=bool)


class RFITransientVisMask(RFIVisMask):
    """Identify and flag transient RFI in visibility data (drop-in for ``flagging.py:1191-1277``).

    Each frequency is high-pass filtered along time (``filters.highpass_weighted_convolution_filter``), transformed
    across the baseline axis into "beams" and its modulus compared with its moving median in units of its moving MAD
    (:func:`mad`); a hysteresis threshold keeps what is above ``sigma_high`` and what is above ``sigma_low`` and
    connected to it.  The SIR operator then runs along time and along frequency, and a time-frequency sample is flagged
    if more than ``frac_samples`` of its beams are.

    Config (names and defaults are the reference's): ``mad_base_size`` ([1, 101]) and ``mad_dev_size`` ([1, 51]), the
    (beam, time) windows of the median and of the MAD; ``sigma_high`` (8.0), ``sigma_low`` (2.0); ``frac_samples``
    (0.01).  ``workspace_mib`` (1024): the device memory the frequency batches of the first phase and the beam slabs of
    the second are sized for; the result does not depend on it.

    Everything from the stream to the mask runs on the device (``csrc/vismask.hip`` and ``csrc/rfi.hip``, DESIGN.md
    section 7t); the flag cube ``[freq, beam, time]``, a byte per sample, stays there if it takes at most half the
    workspace and is staged through the host otherwise.
    """

    mad_base_size = (1, 101)
    mad_dev_size = (1, 51)
    sigma_high = 8.0
    sigma_low = 2.0
    frac_samples = 0.01
    workspace_mib = 1024.0
    _config_names = ("stokes_i", "mad_base_size", "mad_dev_size", "sigma_high", "sigma_low", "frac_samples", "workspace_mib")

    # device bytes per (beam, time) sample of one frequency in the first phase: the Stokes-I planes (12), the filtered
    # plane (16), the modulus (8), the two medians, the deviation, the ratio and the flags of `_mad_device` (8 each,
    # real and imaginary baseline counted), the hysteresis state
    _PHASE1_BYTES = 12 + 16 + 8 + 6 * 8 + 4
    # ... and per flag of the second phase: the slab, its copy, the result and the 16 bytes of SIR scratch
    _PHASE2_BYTES = 3 + 16

    def read_config(self, params):
        super().read_config(params)
        for name in ("mad_base_size", "mad_dev_size"):
            size = tuple(int(s) for s in getattr(self, name))
            if len(size) != 2:
                raise ValueError(f"{name} must have two entries, got {size}")
            setattr(self, name, size)

    def generate_mask(self, vis, weight, mask, freq, baselines, times, info=None):
        """Mask scattered transient RFI.  Arguments as :meth:`RFIVisMask.generate_mask`; returns a Boolean array.
        ``info``: a dict that receives the batch sizes and the largest sweep count of the hysteresis."""
        ctx = Context.get()
        windows = filters.check_size(self.mad_base_size, 2), filters.check_size(self.mad_dev_size, 2)
        ra = np.unwrap(self.telescope.unix_to_lsa(times), period=360.0) * np.pi / 180.0
        dec = np.deg2rad(self.telescope.latitude)
        lambda_inv = np.min(freq) * 1e6 / self.SPEED_OF_LIGHT
        hpf_cut = lambda_inv * np.asarray(baselines)[:, 0].max() / np.cos(dec)
        taps = ctx.to_device(filters.convolution_taps(ra, hpf_cut))

        nfreq, nbeam, ntime = (int(s) for s in vis.shape)
        if not _lib.lib.dmm_beam_abs_fft_supported(nbeam):
            raise _lib.DmmError(_lib.DMM_E_UNSUPPORTED, f"RFITransientVisMask: {nbeam} baselines do not fit the in-LDS transform")
        budget = max(int(float(self.workspace_mib) * (1 << 20)), 1)  # (a fraction of a MiB is accepted: one frequency, one beam at a time)
        cube_dev = ctx.device if nfreq * nbeam * ntime <= budget // 2 else torch.device("cpu")
        cube = torch.empty((nfreq, nbeam, ntime), dtype=torch.uint8, device=cube_dev)
        cube.copy_(mask[:, None, :].expand(nfreq, nbeam, ntime))

        # phase 1: per frequency, in batches
        active = np.flatnonzero(~mask.ne(0).all(dim=1).cpu().numpy())  # a fully masked frequency is skipped
        per = max(1, budget // (self._PHASE1_BYTES * nbeam * ntime))
        sweeps = 0
        hinfo = {}
        for i0 in range(0, len(active), per):
            sel = active[i0 : i0 + per]
            run = len(sel) == sel[-1] - sel[0] + 1  # adjacent frequencies: views, no gather
            take = slice(int(sel[0]), int(sel[-1]) + 1) if run else ctx.to_device(sel.astype(np.int64))
            v, w = vis[take].contiguous(), weight[take].contiguous()
            hp = filters.wconv_filter_device(ctx, v, w, taps, highpass=True)
            beams = torch.empty(hp.shape, dtype=torch.float64, device=hp.device)
            _lib.check(_lib.lib.dmm_beam_abs_fft(ctx.handle, ptr(hp), len(sel), nbeam, ntime, ptr(beams)))
            del hp
            flags = mask[take][:, None, :].expand(len(sel), nbeam, ntime).contiguous()
            ratio = _mad_device(ctx, beams, flags, *windows)[0]
            rfi.hysteresis_device(ctx, ratio, self.sigma_low, self.sigma_high, out=flags, info=hinfo)
            sweeps = max(sweeps, hinfo["sweeps"])
            cube[take if run else torch.as_tensor(sel, device=cube_dev)] = flags.to(cube_dev)
        ctx.uses(taps)

        # phase 2: SIR along time and along frequency, in slabs of beams, and the count over beams
        count = torch.zeros((nfreq, ntime), dtype=torch.int32, device=ctx.device)
        slab_beams = max(1, min(nbeam, budget // (self._PHASE2_BYTES * nfreq * ntime)))
        keep = mask.eq(0).to(torch.uint8)[:, None, :]
        for b0 in range(0, nbeam, slab_beams):
            slab = cube[:, b0 : b0 + slab_beams, :].contiguous().to(ctx.device)
            nb = int(slab.shape[1])
            seed = slab * keep  # nothing that was masked to begin with is extended
            grown = rfi.sir_device(ctx, seed.view(nfreq * nb, ntime), 0.2, 1)
            rfi.sir_device(ctx, seed.view(nfreq, nb * ntime), 0.1, 0, out=grown.view(nfreq, nb * ntime))
            _or_into(ctx, slab, grown.view(nfreq, nb, ntime))
            _lib.check(_lib.lib.dmm_rfi_beam_count(ctx.handle, ptr(slab), nfreq, nb, ntime, ptr(count)))
        if info is not None:
            info.update(freq_per_batch=per, beams_per_slab=slab_beams, sweeps=sweeps, cube_on_device=cube_dev.type != "cpu")
        # count / nbeam is the reference's mean over beams of a Boolean array: an exact integer over nbeam, in float64
        # (one small plane, compared on the host with NumPy's own division)
        return (count.cpu().numpy().astype(np.float64) / nbeam) > self.frac_samples


def _stack_plane(ds, ind):
    """``ds[:, ind]`` on the host, without bringing the rest of a device-resident dataset back."""
    if isinstance(ds, containers.Dataset) and ds.on_device:
        return ds._dev[:, ind].cpu().numpy()
    return np.asarray(ds[:])[:, ind]


class RFIMask(ContainerTask):
    """A quick RFI mask from one stack entry (drop-in for ``flagging.py:2120-2219``): :func:`mad` with its default
    windows, the ``sigma`` cut, and :func:`tv_channels_flag`.

    Config: ``sigma`` (5.0), the cut in Gaussian sigmas; ``tv_fraction`` (0.5), the ``f`` of the TV test;
    ``stack_ind``, the stack entry whose visibilities stand for the whole data set.  A ``SiderealStream`` gives a
    ``SiderealRFIMask``, a ``TimeStream`` an ``RFIMask``.
    """

    sigma = 5.0
    tv_fraction = 0.5
    stack_ind = None
    _config_names = ("sigma", "tv_fraction", "stack_ind")

    def process(self, sstream):
        kind = containers.SiderealRFIMask if "ra" in sstream.index_map else containers.RFIMask
        sstream.redistribute(["stack", "prod"])
        if self.stack_ind is None:
            raise ValueError("RFIMask needs stack_ind")
        ind, nstack = int(self.stack_ind), sstream.vis.shape[1]
        if not 0 <= ind < nstack:
            raise ValueError(f"stack_ind {ind} is outside the {nstack} stack entries")

        # The one stack entry's two planes come to the host and go back: the cut below is a ten-thousandth of the
        # MEAN weight, and NumPy's float32 pairwise mean is what the recorded masks were made with; a device
        # reduction would round differently and could move samples across the cut.  One plane each way, once.
        vis = _stack_plane(sstream.vis, ind)
        weight = _stack_plane(sstream.weight, ind)
        negligible = weight < 1e-4 * weight.mean()

        ctx = Context.get()
        # a sample whose windows held no data has no deviation: it is given 2 sigma, which the cut always catches
        (dev, over), _, _ = _mad_device(ctx, vis, _u8(ctx, negligible), (11, 3), (21, 21), nan_fill=2 * self.sigma, nsigma=self.sigma)
        tvmask, _ = _TVBands(ctx, sstream.freq).flag(ctx, dev, self.sigma, self.tv_fraction)
        mask = _or_into(ctx, tvmask, over).cpu().numpy().astype(bool)
        out = kind(axes_from=sstream, attrs_from=sstream)
        out.mask[:] = mask
        self.log.info("Flagging %0.2f%% of data due to RFI." % (100.0 * mask.mean()))
        return out


class NegativeAutosMask(ContainerTask):
    """Flag a (frequency, time) sample if any autocorrelation is negative there (drop-in for ``flagging.py:666-699``).

    The autocorrelations are the stack entries whose ``prodstack`` pair is one input twice; their rows are read on the
    device (``dmm_sens_negative_autos``, the row list ``ComputeSystemSensitivity``'s radiometer kernel takes) and the
    mask of the ``RFIMask`` that comes back is written there.
    """

    def process(self, data):
        data.redistribute("freq")
        ps = _prodstack(data)
        ctx = Context.get()
        vis = _dev_dataset(data.vis, ctx, np.complex64)
        nfreq, nstack, ntime = (int(s) for s in vis.shape)
        if ps is None or len(ps) != nstack:
            raise ValueError("NegativeAutosMask needs the prod/stack index maps to find the auto-correlations")
        rows = np.ascontiguousarray(np.flatnonzero(ps["input_a"] == ps["input_b"]), dtype=np.int32)
        mask = torch.empty((nfreq, ntime), dtype=torch.uint8, device=ctx.device)
        table = torch.empty((len(rows) + 1,), dtype=torch.int32, device=ctx.device)
        _lib.check(_lib.lib.dmm_sens_negative_autos(ctx.handle, ptr(vis), nfreq, nstack, ntime, len(rows), C.c_void_p(rows.ctypes.data), ptr(table), ptr(mask)))
        if self.log.isEnabledFor(logging.DEBUG):
            self.log.debug(f"{100.0 * float(mask.float().mean()):.2f}% of data flagged due to negative autos.")
        out = containers.RFIMask(axes_from=data, attrs_from=data, allocate=False)
        out.attach("mask", mask.view(torch.bool))
        return out


def _copy_container(cont, shared):
    """``cont.copy(shared=...)`` that keeps device-resident datasets on the device."""
    out = cont.copy(shared=tuple(cont.datasets))
    for name, ds in cont.datasets.items():
        if name in shared:
            continue
        if ds.on_device:
            out.datasets[name] = containers.Dataset(dev=ds._dev.clone(), attrs=_copy.deepcopy(ds.attrs))
        else:
            out.datasets[name] = containers.Dataset(host=np.array(ds.host(), copy=True), attrs=_copy.deepcopy(ds.attrs))
    return out


class ApplyTimeFreqMask(ContainerTask):
    """Zero the weights of a stream where a time-frequency mask is set (drop-in for ``flagging.py:2222-2377``).

    Config (the reference's):

    ``share`` ("all")
        "all" works in place and returns the input; "vis" / "map" return a container that shares that dataset with
        the input and owns a new weight; "none" copies everything.
    ``collapse_pol`` (False)
        a by-polarisation mask is OR-ed over polarisation first (always, if the stream's weight has no ``pol`` axis).
    ``match_axes`` (True)
        the time-like axes must be equal; if False the mask is applied to the samples the two axes have in common
        and the rest of the stream is left alone.

    A weight that lives on the device is multiplied there (``dmm_rfi_apply_mask``, time-like axis last); a weight on
    the host is multiplied on the host.
    """

    share = "all"
    collapse_pol = False
    match_axes = True
    _config_names = ("share", "collapse_pol", "match_axes")

    # mask classes by their time-like axis, with the word the error message uses for the stream they need
    _KINDS = (("time", (containers.RFIMask, containers.RFIMaskByPol), "timestream"), ("ra", (containers.SiderealRFIMask, containers.SiderealRFIMaskByPol), "sidereal stream"))

    def read_config(self, params):
        super().read_config(params)
        if self.share not in ("none", "vis", "map", "all"):
            raise ValueError(f"share must be one of 'none', 'vis', 'map', 'all', not {self.share!r}")

    def process(self, tstream, rfimask):
        """``tstream``: anything with ``freq``, a ``time`` or ``ra`` axis and a ``weight``; ``rfimask``: one of the four
        mask containers.  Returns the masked stream."""
        axis = self._timelike_axis(tstream, rfimask)
        if not np.array_equal(tstream.freq, rfimask.freq):
            raise ValueError("timestream and mask data have different freq axes.")
        data_sel, mask_sel = self._pair_samples(np.asarray(getattr(tstream, axis)), np.asarray(getattr(rfimask, axis)))
        tstream.redistribute("freq")
        w_axes = list(tstream.weight.attrs["axis"])
        mask, m_axes = self._mask_for(tstream, rfimask, w_axes)
        shared = {"all": None, "vis": ("vis",), "map": ("map",), "none": ()}[self.share]
        out = tstream if shared is None else _copy_container(tstream, shared)
        if out.weight.on_device:
            self._apply_device(out.weight, w_axes, m_axes, mask, axis, data_sel, mask_sel)
        else:
            self._apply_host(out.weight, w_axes, m_axes, mask, axis, data_sel, mask_sel)
        return out

    def _timelike_axis(self, tstream, rfimask):
        for axis, classes, word in self._KINDS:
            if isinstance(rfimask, classes):
                if not hasattr(tstream, axis):
                    raise TypeError(f"Expected a {word} like type. Got {type(tstream)}.")
                return axis
        raise TypeError(f"Require a RFIMask or SiderealRFIMask. Got {type(rfimask)}.")

    def _pair_samples(self, of_data, of_mask):
        """Positions along the time-like axis, in the stream and in the mask, of the samples to treat."""
        if self.match_axes:
            if not np.array_equal(of_data, of_mask):
                raise ValueError("timestream and mask data have different time-like axes.")
            both = np.arange(len(of_data))
            return both, both
        data_sel = np.flatnonzero(np.isin(of_data, of_mask))
        mask_sel = np.flatnonzero(np.isin(of_mask, of_data))
        if len(data_sel) == 0:
            raise ValueError(f"No overlapping samples found in timelike axis.Data axis: {of_data}\nMask axis: {of_mask}")
        if len(data_sel) != len(mask_sel):
            raise ValueError("the overlapping samples of the time-like axes do not pair up.")
        return data_sel, mask_sel

    def _mask_for(self, tstream, rfimask, w_axes):
        """The Boolean mask and its axis names, polarisation folded away where the weight has none or on request."""
        mask = np.asarray(rfimask.mask[:], dtype=bool)
        m_axes = list(rfimask.mask.attrs["axis"])
        if "pol" in m_axes:
            if self.collapse_pol or "pol" not in w_axes:
                mask = mask.any(axis=m_axes.index("pol"))
                m_axes.remove("pol")
            elif not np.array_equal(tstream.index_map["pol"], rfimask.pol):
                raise ValueError("timestream and mask data have different pol axes.")
        return mask, m_axes

    @staticmethod
    def _apply_host(weight, w_axes, m_axes, mask, axis, data_sel, mask_sel):
        # the mask in the weight's axis order with length-1 axes where it has none, both with the time-like axis last
        order = [m_axes.index(ax) for ax in w_axes if ax in m_axes]
        shape = [mask.shape[m_axes.index(ax)] if ax in m_axes else 1 for ax in w_axes]
        keep = np.moveaxis(~mask.transpose(order).reshape(shape), w_axes.index(axis), -1)
        w = weight.host()
        view = np.moveaxis(w, w_axes.index(axis), -1)
        view[..., data_sel] = view[..., data_sel] * keep[..., mask_sel]
        weight[:] = w

    @staticmethod
    def _apply_device(weight, w_axes, m_axes, mask, axis, data_sel, mask_sel):
        if w_axes[-1] != axis or m_axes[-1] != axis:
            raise NotImplementedError(f"the device form needs the time-like axis last, the weight has {w_axes} and the mask {m_axes}")
        if [ax for ax in w_axes if ax in m_axes] != m_axes:
            raise NotImplementedError(f"the device form needs the mask's axes {m_axes} in the weight's order {w_axes}")
        lead = w_axes[:-1]
        if len(lead) > 4:
            raise NotImplementedError(f"the device form takes at most four axes ahead of the time-like one, got {lead}")
        ctx = Context.get()
        w = weight.device(ctx)
        if w.dtype != torch.float32:
            raise TypeError(f"the weight must be float32, got {w.dtype}")
        w = w.contiguous()
        mask = np.ascontiguousarray(mask)
        mstride = np.array(mask.strides, dtype=np.int64) // mask.itemsize
        dims = np.array([w.shape[i] for i in range(len(lead))], dtype=np.int64)
        strides = np.array([mstride[m_axes.index(ax)] if ax in m_axes else 0 for ax in lead], dtype=np.int64)
        # (named, so that all three stay allocated until the launch)
        mask_d, data_d, sel_d = _u8(ctx, mask), ctx.to_device(data_sel.astype(np.int32)), ctx.to_device(mask_sel.astype(np.int32))
        _lib.check(
            _lib.lib.dmm_rfi_apply_mask(
                ctx.handle, ptr(w), len(lead), C.c_void_p(dims.ctypes.data), int(w.shape[-1]), ptr(mask_d), C.c_void_p(strides.ctypes.data), int(mstride[-1]),
                int(mask.shape[-1]), len(data_sel), ptr(data_d), ptr(sel_d),
            )
        )
        weight.set_device(w)


ApplyRFIMask = ApplyTimeFreqMask  # the reference's older name for the task
