"""Delay spectrum estimation on the GPU: inverse-FFT and Wiener-filter delay transforms.

Drop-in for the frequency-to-delay transforms of ``draco/analysis/delay.py``:

* :func:`delay_spectrum_fft`, :func:`delay_spectrum_wiener_filter`                      ``delay.py:2102-2201``
* :func:`fourier_matrix_r2c`, :func:`fourier_matrix_c2r`, :func:`fourier_matrix_c2c`, :func:`fourier_matrix`   ``delay.py:1480-1613``
* :class:`DelaySpectrumFFT`, :class:`DelaySpectrumWienerFilter`, :class:`DelaySpectrumWienerFilterIteratePS`   ``delay.py:347-1053``
* :class:`DelaySpectrumToPowerSpectrum`                                                  ``delay.py:1061-1106``
* :class:`DelayPowerSpectrumBase`, :class:`DelayPowerSpectrumNRML`                        ``delay.py:744-818, 1114-1215, 1270-1301``
* :class:`DelayFilter`, :class:`DelayFilterBase` (the delay null-space filter)             ``delay.py:29-339``

Same names, config attributes, defaults and ``setup`` / ``process`` signatures.  The arithmetic runs in
``libdraco_amd.so`` (``csrc/delay.hip``), batched over baselines: a prepare pass (the ``time_frac`` / ``freq_frac``
masks, the mean over the retained samples, the averaged weights), a projection onto one Fourier matrix shared by every
baseline on the f64 matrix cores, a blocked float64 Cholesky solve of the Wiener matrix, and a store that applies the
task's ``fftshift``.  The input datasets are read through strides where they lie (on the device if they are already
there) and are not modified; the output ``spectrum`` stays on the device.

``F^T N^-1 F`` is circulant (2 x 2 block circulant in the complex time domain), so the Wiener matrix is filled from
one cosine (and one sine) sequence that the projection delivers as one more right-hand side; a cut channel is a zero
coefficient, not a smaller matrix.  The order of the solve, ``ndelay`` (real time domain) or ``2 ndelay`` (complex),
may be 1 ... 2048.

The transform needs the whole band in one process: frequency sharding does not apply to these tasks.

Out of scope (``NotImplementedError`` where a parameter asks for it): ``use_average_weights=False`` (the reference's
Wiener function cannot take per-sample weights either) and ``scale_freq=True``; not provided: the Gibbs and
cross-spectrum estimators.  The NRML estimator's optimiser and evaluators are in
:mod:`draco_amd.analysis.delayopt`.  (The ``DelayTransformOperator`` container and the
Wiener delay transform of a filtered ring map that fills it are in ``draco_amd.analysis.powerspec``.)

The two filter tasks project every item (a stack entry, an ``el`` of a ring map) onto the null space of the
delays below its cut: a mask pass and a batched Jacobi SVD in ``csrc/nullfilter.hip`` (``draco_amd.util.filters``),
then the in-place product of ``csrc/dayenu.hip``; the datasets stay on the device.  Of ``DelayFilterBase``'s four
default containers the ``HybridVisMModes`` / ``m`` and ``GridBeam`` / ``theta`` layouts, and any non-default ``axis``,
raise ``NotImplementedError``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.constants
import torch

from .. import _lib
from ..core import containers, io
from ..core.task import ContainerTask
from ..device import Context, ptr
from ..util import filters, tools
from .transform import _dev_dataset

MAX_ORDER = 2048
_WINDOWS = ("uniform", "hann", "hanning", "hamming", "blackman", "nuttall", "blackman_nuttall", "blackman_harris")
_DTYPE = {
    np.dtype(np.float32): _lib.DMM_DELAY_F32,
    np.dtype(np.float64): _lib.DMM_DELAY_F64,
    np.dtype(np.complex64): _lib.DMM_DELAY_C64,
    np.dtype(np.complex128): _lib.DMM_DELAY_C128,
}
_TORCH2NP = {torch.float32: np.float32, torch.float64: np.float64, torch.complex64: np.complex64, torch.complex128: np.complex128}


# ---- Fourier matrices


def _channels(fsel, count):
    return np.arange(count) if fsel is None else np.asarray(fsel)


def _host_trig(N, chan):
    """``cos`` and ``sin`` of the phase ``2 pi f t / N`` of channel ``f`` at time sample ``t``, ``[nsel, N]``, in
    NumPy.  The phase is taken as the plain float64 product (the host forms agree with the reference's values to
    1e-15; the device forms reduce ``f t`` modulo ``N`` in integers and are the accurate ones)."""
    phase = np.multiply.outer(chan, 2 * np.pi * np.arange(N)) / N
    return np.cos(phase), np.sin(phase)


def _fourier_device(N, chan, complex_td):
    ctx = Context.get()
    chan = np.ascontiguousarray(chan, dtype=np.int32)
    if chan.ndim != 1 or chan.size == 0 or N < 1 or np.any(chan < 0):
        raise ValueError("fourier matrix: N must be positive and fsel a non-empty 1-D list of non-negative channel indices")
    chan_d = ctx.to_device(chan)
    F = ctx.empty((2 * chan.size, 2 * N if complex_td else N), np.float64)
    _lib.check(_lib.lib.dmm_delay_fourier(ctx.handle, int(N), int(chan.size), int(complex_td), ptr(chan_d), ptr(F)))
    ctx.uses(chan_d)
    return F


def fourier_matrix_r2c(N, fsel=None, device=True):
    """Fourier matrix of a real to complex FFT: ``[2 nsel, N]``, a (cos, -sin) pair of rows per channel (the real and
    the imaginary part of that channel).  ``fsel`` defaults to the ``N // 2 + 1`` channels of an even ``N``.  On the
    device (a float64 tensor, arguments reduced exactly); with ``device=False`` a NumPy array."""
    chan = _channels(fsel, N // 2 + 1)
    if device:
        return _fourier_device(N, chan, False)
    c, s = _host_trig(N, chan)
    return np.stack([c, -s], axis=1).reshape(2 * len(chan), N)


def fourier_matrix_c2r(N, fsel=None, device=True):
    """Fourier matrix of a complex to real FFT: ``[N, 2 nsel]``, the transpose of :func:`fourier_matrix_r2c` with every
    channel weighted ``2 / N``, or ``1 / N`` for the strictly real channels 0 and ``N / 2``."""
    chan = _channels(fsel, N // 2 + 1)
    c, s = _host_trig(N, chan)
    share = np.where((chan == 0) | (chan == N // 2), 1.0, 2.0) / N
    F = np.stack([c * share[:, np.newaxis], -s * share[:, np.newaxis]], axis=1).reshape(2 * len(chan), N).T.copy()
    return Context.get().to_device(F) if device else F


def fourier_matrix_c2c(N, fsel=None, device=True):
    """Fourier matrix of a complex to complex FFT in ``numpy.fft.fft``'s sign convention: ``[2 nsel, 2 N]``, input and
    output as alternating real and imaginary elements, so each (channel, sample) entry is the rotation
    ``[[cos, sin], [-sin, cos]]``."""
    chan = _channels(fsel, N)
    if device:
        return _fourier_device(N, chan, True)
    c, s = _host_trig(N, chan)
    rot = np.stack([np.stack([c, s], axis=-1), np.stack([-s, c], axis=-1)], axis=1)  # [nsel, 2, N, 2]
    return rot.reshape(2 * len(chan), 2 * N)


def fourier_matrix(N, fsel=None, device=True):
    """The complex Fourier matrix ``exp(-2 pi i f t / N)``: ``[nsel, N]`` complex128."""
    c, s = _host_trig(N, _channels(fsel, N))
    F = c - 1j * s
    return Context.get().to_device(F) if device else F


# ---- the batched pipeline


def _view(t, dtype_code, s_sample, s_freq, s_fold=()):
    fold = (C.c_int64 * 4)(*([int(s) for s in s_fold] + [0] * (4 - len(s_fold))))
    return _lib.dmm_delay_view(C.c_void_p(t.data_ptr()), int(dtype_code), int(s_sample), int(s_freq), fold)


def _shifted_inverse(ps, complex_td):
    """``Si`` of the solve from prior rows ``ps [..., ndelay]`` as the task holds them: the reference passes
    ``fftshift`` of the row, inverts where non-zero, and doubles and repeats per component in the complex case."""
    si = tools.invert_no_zero(np.fft.fftshift(np.asarray(ps, dtype=np.float64), axes=-1))
    if complex_td:
        si = 2.0 * np.repeat(si, 2, axis=-1)
    return np.ascontiguousarray(si)


def _transform(ctx, data_v, weight_v, fold_n, nbase, nsample, channel_ind, ndelay, complex_td, coef, si, *, remove_mean, time_frac, freq_frac, weight_boost, spectrum, mask=None,
               workspace_mib=1024, what="baseline"):
    """Run prepare / project / (solve) / store over ``nbase`` baselines in batches; ``si [nbase, order]`` (host) selects
    the Wiener filter, ``None`` the inverse FFT.  Returns the status words (host)."""
    wiener = si is not None
    nchan = int(len(channel_ind))
    order = 2 * ndelay if complex_td else ndelay
    if nsample > 65535:
        raise ValueError(f"delay transform: {nsample} samples, the kernels take at most 65535")
    nrow = nsample + (1 if wiener else 0)
    chan_d = ctx.to_device(np.ascontiguousarray(channel_ind, dtype=np.int32))
    coef_d = ctx.to_device(np.ascontiguousarray(coef, dtype=np.float64))
    F = ctx.empty((2 * nchan, order), np.float64)
    _lib.check(_lib.lib.dmm_delay_fourier(ctx.handle, ndelay, nchan, int(complex_td), ptr(chan_d), ptr(F)))
    fold = (C.c_int64 * max(1, len(fold_n)))(*[int(x) for x in fold_n])
    per_bytes = 8 * (nrow * 2 * nchan + nrow * order + (order * order if wiener else 0)) + nsample + 64
    per = max(1, min(65535, (int(workspace_mib) << 20) // per_bytes))
    status_all = np.zeros(nbase, dtype=np.int32)
    for b0 in range(0, nbase, per):
        nb = min(per, nbase - b0)
        X = ctx.empty((nb, nrow, 2 * nchan), np.float64)
        Y = ctx.empty((nb, nrow, order), np.float64)
        nzt = ctx.empty((nb, nsample), np.uint8)
        status = ctx.empty((nb,), np.int32)
        _lib.check(
            _lib.lib.dmm_delay_prepare(
                ctx.handle, ndelay, nchan, nsample, nb, b0, len(fold_n), fold, C.byref(data_v), C.byref(weight_v), int(complex_td), int(wiener), int(bool(remove_mean)),
                float(time_frac), float(freq_frac), float(weight_boost), ptr(coef_d), ptr(chan_d), ptr(X), ptr(nzt), ptr(status),
            )
        )
        _lib.check(_lib.lib.dmm_delay_project(ctx.handle, order, nchan, nrow, nb, ptr(X), ptr(F), ptr(Y), ptr(status)))
        si_d = G = None
        if wiener:
            si_d = ctx.to_device(np.ascontiguousarray(si[b0 : b0 + nb]))
            G = ctx.empty((nb, order, order), np.float64)
            _lib.check(_lib.lib.dmm_delay_solve(ctx.handle, order, int(complex_td), nsample, nb, ptr(Y), ptr(si_d), ptr(G), ptr(status)))
        _lib.check(
            _lib.lib.dmm_delay_store(ctx.handle, ndelay, int(complex_td), nsample, nrow, nb, ptr(Y), ptr(nzt), ptr(status), ptr(spectrum[b0 : b0 + nb]), ptr(mask[b0 : b0 + nb]) if mask is not None else None)
        )
        status_all[b0 : b0 + nb] = status.cpu().numpy()
        ctx.uses(X, Y, nzt, status, si_d, G)
        bad = np.flatnonzero(status_all[b0 : b0 + nb] == _lib.DMM_DELAY_NOT_POSDEF)
        if bad.size:
            raise np.linalg.LinAlgError(f"delay transform: the Wiener matrix of {what} {b0 + int(bad[0])} is not positive definite")
        cut = np.flatnonzero(status_all[b0 : b0 + nb] == _lib.DMM_DELAY_CUT)
        if cut.size:
            raise ValueError(f"delay transform: {what} {b0 + int(cut[0])} has cut channels; the FFT estimator needs every one of the {ndelay} channels")
    ctx.uses(chan_d, coef_d, F)
    return status_all


def _check_order(order):
    if not 1 <= order <= MAX_ORDER:
        raise ValueError(f"delay transform: a solve of order {order}, the kernels take 1 ... {MAX_ORDER}")


def _sample_block(data, what):
    """A ``[nsample, nfreq]`` array as a contiguous device tensor of a dtype the kernels read."""
    ctx = Context.get()
    if isinstance(data, torch.Tensor):
        t = data.to(ctx.device)
        if t.dtype not in _TORCH2NP:
            t = t.to(torch.complex128 if t.is_complex() else torch.float64)
        t = t.contiguous()
    else:
        a = np.asarray(data)
        if a.dtype not in _DTYPE:
            a = a.astype(np.complex128 if a.dtype.kind == "c" else np.float64)
        t = ctx.to_device(a)
    if t.ndim != 2:
        raise ValueError(f"{what}: data must be [nsample, freq], not {tuple(t.shape)}")
    return ctx, t


def _window_coef(x, window):
    return np.ones(len(x)) if window is None else np.asarray(tools.window_generalised(np.asarray(x, dtype=np.float64), window=window), dtype=np.float64)


def delay_spectrum_fft(data, N, window="nuttall"):
    """Estimate the delay transform of ``data [nsample, N]`` by inverse FFT (``delay.py:2102-2129``).

    The window is evaluated at ``arange(N) / N``.  Returns ``[nsample, N]`` complex128 **on the device** (not shifted);
    ``data`` is not modified.  Only a complex time domain with every channel present has ``N`` channels: any other
    width raises ``ValueError``.
    """
    ctx, t = _sample_block(data, "delay_spectrum_fft")
    nsample, nfreq = (int(s) for s in t.shape)
    if nfreq != int(N):
        raise ValueError(f"delay_spectrum_fft: {nfreq} channels cannot be transformed to {N} delays")
    coef = _window_coef(np.arange(N) / N, window) / N
    ones = ctx.to_device(np.ones(nfreq, dtype=np.float64))
    spec = ctx.empty((1, nsample, N), np.complex128)
    _transform(ctx, _view(t, _DTYPE[np.dtype(_TORCH2NP[t.dtype])], nfreq, 1), _view(ones, _lib.DMM_DELAY_F64, 0, 1), (), 1, nsample, np.arange(N), int(N), True, coef, None,
               remove_mean=False, time_frac=-1.0, freq_frac=0.0, weight_boost=1.0, spectrum=spec)
    ctx.uses(t, ones)
    return torch.fft.ifftshift(spec[0], dim=-1)


def delay_spectrum_wiener_filter(delay_PS, data, N, Ni, window="nuttall", fsel=None, complex_timedomain=False):
    """Estimate the delay spectrum of ``data [nsample, freq]`` by Wiener filtering (``delay.py:2132-2201``).

    ``delay_PS [N]`` is the signal power spectrum, ``Ni [freq]`` the inverse noise variance, ``fsel`` the indices of
    the channels present among the ``N // 2 + 1`` (real time domain) or ``N`` (complex) of the full set; the window is
    evaluated at ``fsel / total``.  Returns ``[nsample, N]`` **on the device**, float64 in the real time domain and
    complex128 otherwise.  A matrix that is not positive definite raises ``numpy.linalg.LinAlgError``.
    """
    ctx, t = _sample_block(data, "delay_spectrum_wiener_filter")
    N = int(N)
    total = N if complex_timedomain else N // 2 + 1
    fsel = np.arange(total) if fsel is None else np.asarray(fsel)
    nsample, nfreq = (int(s) for s in t.shape)
    ni = np.ascontiguousarray(Ni, dtype=np.float64)
    if ni.shape != (nfreq,) or fsel.shape != (nfreq,):
        raise ValueError(f"delay_spectrum_wiener_filter: {nfreq} channels of data, Ni {ni.shape}, fsel {fsel.shape}")
    ps = np.asarray(delay_PS, dtype=np.float64)
    if ps.shape != (N,):
        raise ValueError(f"delay_spectrum_wiener_filter: delay_PS {ps.shape} for {N} delays")
    _check_order(2 * N if complex_timedomain else N)
    coef = _window_coef(fsel / total, window) ** 2
    si = tools.invert_no_zero(ps)
    si = (2.0 * np.repeat(si, 2) if complex_timedomain else si)[np.newaxis, :]
    ni_d = ctx.to_device(ni)
    spec = ctx.empty((1, nsample, N), np.complex128)
    _transform(ctx, _view(t, _DTYPE[np.dtype(_TORCH2NP[t.dtype])], nfreq, 1), _view(ni_d, _lib.DMM_DELAY_F64, 0, 1), (), 1, nsample, fsel, N, bool(complex_timedomain), coef, si,
               remove_mean=False, time_frac=-1.0, freq_frac=0.0, weight_boost=1.0, spectrum=spec, what="matrix")
    ctx.uses(t, ni_d)
    out = torch.fft.ifftshift(spec[0], dim=-1)
    return out if complex_timedomain else out.real.contiguous()


# ---- tasks


class DelayTransformBase(ContainerTask):
    """What the delay transforms share (``delay.py:347-866``): the delay grid, the view of the input as ``[baseline,
    sample, freq]``, the output container.

    Attributes
    ----------
    freq_zero : float, optional
        The physical frequency (MHz) of the zero (DC) channel of the F-engine.  Default: the first frequency.
    freq_spacing : float, optional
        The spacing between the underlying channels (MHz).  Default: the smallest gap found between channels.
    nfreq : int, optional
        The number of channels in the full set.  Default: the last included frequency is the last of the full set (the
        penultimate with ``skip_nyquist``).
    skip_nyquist : bool
        Whether the Nyquist frequency is missing from the data.  Default True.
    apply_window : bool
        Whether to apodise the frequency axis.  Default True.
    window : str
        One of the cosine-sum windows of :func:`draco_amd.util.tools.window_generalised`.  Default 'nuttall'.
    complex_timedomain : bool
        Whether the channelised time samples were complex; then ``freq_zero``, ``nfreq`` and ``skip_nyquist`` are
        ignored.  Default False.
    use_average_weights : bool
        Use noise weights averaged over the samples.  Default True; ``False`` raises ``NotImplementedError``.
    weight_boost : float
        Multiply the weights by this factor.  Default 1.0.
    freq_frac, time_frac : float
        A channel (a sample) is retained if its share of unmasked samples (channels) is strictly above this.  Default
        0.0 for both.
    remove_mean : bool
        Subtract the mean over the retained samples of each channel.  Default True.
    scale_freq : bool
        Default False; ``True`` raises ``NotImplementedError``.
    dataset : str, optional
        The dataset to transform.  Default: the container's main dataset (``vis``, or ``map`` of a ring map).
    sample_axis : str
        Every sample along this axis is drawn from the same power spectrum; all axes other than this one and ``freq``
        are folded into ``baseline``, slowest first.
    save_spectrum_mask : bool
        Add ``spectrum_mask [baseline, sample]``, set where a baseline was skipped or a sample dropped.  Default False.
    workspace_mib : int
        Device memory the scratch of one batch of baselines may take.  Default 1024.

    The whole band must be in this process.  The input datasets are not modified.
    """

    _config_names = (
        "freq_zero", "freq_spacing", "nfreq", "skip_nyquist", "apply_window", "window", "complex_timedomain", "use_average_weights", "weight_boost", "freq_frac", "time_frac",
        "remove_mean", "scale_freq", "dataset", "sample_axis", "save_spectrum_mask", "workspace_mib",
    )
    freq_zero = None
    freq_spacing = None
    nfreq = None
    skip_nyquist = True
    apply_window = True
    window = "nuttall"
    complex_timedomain = False
    use_average_weights = True
    weight_boost = 1.0
    freq_frac = 0.0
    time_frac = 0.0
    remove_mean = True
    scale_freq = False
    dataset = None
    sample_axis = None
    save_spectrum_mask = False
    workspace_mib = 1024

    def read_config(self, params):
        super().read_config(params)
        if self.window not in _WINDOWS:
            raise ValueError(f"window must be one of {_WINDOWS}, not {self.window!r}")

    def _check(self):
        if not self.use_average_weights:
            raise NotImplementedError(f"{type(self).__name__}: use_average_weights=False (weights per sample) is not on the GPU path")
        if self.scale_freq:
            raise NotImplementedError(f"{type(self).__name__}: scale_freq=True is not on the GPU path")

    def _calculate_delays(self, ss):
        """``(delays, channel_ind)``: the delay grid in micro-seconds, ascending through zero, and the index of every
        channel of the data in the full set of the F-engine.

        Complex time domain: the data's channels are the full set, one delay per channel.  Real time domain: a channel's
        index is its distance from ``freq_zero`` in units of the spacing, rounded down; the full set has ``nfreq``
        channels (by default it ends at the data's last channel, or one beyond it with ``skip_nyquist``) and belongs
        to frames of ``2 (nfreq - 1)`` real samples.  ``ss`` is a container with ``freq``, or a list of them."""
        first = ss if hasattr(ss, "freq") else (ss[0] if len(ss) > 0 else None)
        if first is None:
            raise TypeError("Could not find a frequency axis in the input.")
        freq = np.asarray(first.freq)
        spacing = np.abs(np.diff(freq)).min() if self.freq_spacing is None else self.freq_spacing
        if self.complex_timedomain:
            channel_ind = np.arange(len(freq))
            ndelay = len(freq)
        else:
            origin = freq[0] if self.freq_zero is None else self.freq_zero
            channel_ind = np.floor(np.abs(freq - origin) / spacing).astype(np.int64)
            full = self.nfreq if self.nfreq is not None else channel_ind[-1] + (2 if self.skip_nyquist else 1)
            ndelay = 2 * (full - 1)
        step = 1.0 / (ndelay * spacing)  # numpy.fft.fftfreq's own scaling, so the grid equals fftshift(fftfreq(...))
        return (np.arange(ndelay) - ndelay // 2) * step, channel_ind

    def _resolve(self, ss):
        """The dataset to transform, its axes, the axes of the weights and the axes folded into ``baseline``
        (``delay.py:696-741``); ``ValueError`` for an unknown dataset or sample axis."""
        if self.dataset is not None:
            if self.dataset not in ss.datasets:
                raise ValueError(f"{type(self).__name__}: {type(ss).__name__} has no dataset {self.dataset!r}")
            name = self.dataset
        else:
            name = next((n for n in ("vis", "map") if n in ss.datasets), None)
            if name is None:
                raise ValueError(f"{type(self).__name__}: {type(ss).__name__} has neither `vis` nor `map`; name the dataset")
        axes = list(ss.datasets[name].attrs["axis"])
        if self.sample_axis not in ss.index_map or self.sample_axis not in axes:
            raise ValueError(f"{type(self).__name__}: dataset {name!r} of {type(ss).__name__} has no sample axis {self.sample_axis!r}")
        if "freq" not in axes:
            raise ValueError(f"Dataset {name} of {type(ss)} has no freq axis.")
        waxes = list(ss.weight.attrs["axis"])
        if self.sample_axis not in waxes or "freq" not in waxes or any(ax not in axes for ax in waxes):
            raise ValueError(f"The weight axes {waxes} of {type(ss)} cannot be matched to the axes {axes} of {name}.")
        fold = [ax for ax in axes if ax not in (self.sample_axis, "freq")]
        if len(fold) > 4:
            raise NotImplementedError(f"{type(self).__name__}: {len(fold)} axes to fold into baseline, the kernels take at most 4")
        return name, axes, waxes, fold

    def _prepare_inputs(self, ss, ctx, name, axes, waxes, fold):
        """Device tensors of the data and the weights and their views as ``[baseline, sample, freq]`` (``delay.py:2238-2302``;
        a weight dataset that lacks a folded axis is broadcast: stride 0)."""
        data_ds, weight_ds = ss.datasets[name], ss.weight
        ddt = np.dtype(data_ds.dtype)
        wdt = np.dtype(weight_ds.dtype)
        data = _dev_dataset(data_ds, ctx, ddt.type if ddt in _DTYPE else (np.complex128 if ddt.kind == "c" else np.float64))
        weight = _dev_dataset(weight_ds, ctx, wdt.type if wdt in (np.dtype(np.float32), np.dtype(np.float64)) else np.float64)
        ds_, ws_ = data.stride(), weight.stride()
        data_v = _view(data, _DTYPE[np.dtype(_TORCH2NP[data.dtype])], ds_[axes.index(self.sample_axis)], ds_[axes.index("freq")], [ds_[axes.index(ax)] for ax in fold])
        weight_v = _view(weight, _DTYPE[np.dtype(_TORCH2NP[weight.dtype])], ws_[waxes.index(self.sample_axis)], ws_[waxes.index("freq")], [ws_[waxes.index(ax)] if ax in waxes else 0 for ax in fold])
        return data, weight, data_v, weight_v, [int(data.shape[axes.index(ax)]) for ax in fold]


class DelaySpectrumBase(DelayTransformBase):
    """Delay spectrum estimation into a :class:`~draco_amd.core.containers.DelayTransform` (``delay.py:821-957``)."""

    _wiener = False

    def _create_output(self, ss, delays, coord_axes, nbase, nsample, ctx):
        out = containers.DelayTransform(baseline=nbase, sample=ss.index_map[self.sample_axis], delay=delays, attrs_from=ss, weight_boost=self.weight_boost, allocate=False)
        for ax in coord_axes:
            out.create_index_map(ax, ss.index_map[ax])
        out.attrs["baseline_axes"] = coord_axes
        out.attrs["freq"] = np.asarray(ss.freq)
        out.attrs["window_los"] = self.window if self.apply_window else "None"
        return out

    def process(self, ss):
        """Estimate the delay spectrum of every baseline of ``ss``; returns a ``DelayTransform`` whose ``spectrum``
        is on the device."""
        self._check()
        delays, channel_ind = self._calculate_delays(ss)
        ndelay, nchan = len(delays), len(channel_ind)
        ss.redistribute("freq")
        name, axes, waxes, fold = self._resolve(ss)
        fold_n = [len(ss.index_map[ax]) for ax in fold]
        nbase = int(np.prod(fold_n)) if fold_n else 1
        nsample = len(ss.index_map[self.sample_axis])
        complex_td = bool(self.complex_timedomain)
        total = ndelay if complex_td else ndelay // 2 + 1
        if self._wiener:
            _check_order(2 * ndelay if complex_td else ndelay)
            coef = _window_coef(channel_ind / total, self.window if self.apply_window else None) ** 2
            si = self._get_prior(nbase, ndelay, complex_td)
        else:
            if not complex_td or nchan != ndelay:
                raise ValueError(f"{type(self).__name__}: {nchan} channels cannot be transformed to {ndelay} delays by inverse FFT; it takes the complex time domain and the whole band")
            coef = _window_coef(np.arange(ndelay) / ndelay, self.window if self.apply_window else None) / ndelay
            si = None
        ctx = Context.get()
        data, weight, data_v, weight_v, fold_n = self._prepare_inputs(ss, ctx, name, axes, waxes, fold)
        out = self._create_output(ss, delays, fold, nbase, nsample, ctx)
        spectrum = ctx.empty((nbase, nsample, ndelay), np.complex128)
        mask = ctx.empty((nbase, nsample), np.uint8) if self.save_spectrum_mask else None
        _transform(ctx, data_v, weight_v, fold_n, nbase, nsample, channel_ind, ndelay, complex_td, coef, si, remove_mean=self.remove_mean, time_frac=self.time_frac, freq_frac=self.freq_frac,
                   weight_boost=self.weight_boost, spectrum=spectrum, mask=mask, workspace_mib=self.workspace_mib)
        ctx.uses(data, weight)
        out.attach("spectrum", spectrum)
        if mask is not None:
            out.add_dataset("spectrum_mask", allocate=False)
            out.datasets["spectrum_mask"] = containers.Dataset(host=mask.cpu().numpy().astype(bool), attrs={"axis": ["baseline", "sample"]})
        return out


class DelaySpectrumFFT(DelaySpectrumBase):
    """Measure the delay spectrum of a general container by inverse FFT (``delay.py:960-979``).  Only a band of the
    complex time domain without cut channels can be transformed: anything else raises ``ValueError``."""


class DelaySpectrumWienerFilter(DelaySpectrumBase):
    """Measure the delay spectrum of a general container by Wiener filtering (``delay.py:982-1024``,
    https://arxiv.org/abs/2202.01242 Eq. A6): the signal covariance is a delay power spectrum, the noise covariance
    comes from the weights of the input.  A Wiener matrix that is not positive definite raises
    ``numpy.linalg.LinAlgError`` naming the baseline."""

    _wiener = True
    dps = None

    def setup(self, dps=None):
        """Set the delay power spectrum (a ``DelaySpectrum``) to use as the signal covariance."""
        self.dps = dps

    def _get_prior(self, nbase, ndelay, complex_td):
        if self.dps is None:
            raise ValueError(f"{type(self).__name__}: no delay power spectrum given")
        ps = np.asarray(self.dps.spectrum[:], dtype=np.float64)
        if ps.shape != (nbase, ndelay):
            raise ValueError(f"{type(self).__name__}: the delay power spectrum is {ps.shape}, the data need {(nbase, ndelay)}")
        return _shifted_inverse(ps, complex_td)


class DelaySpectrumWienerFilterIteratePS(DelaySpectrumWienerFilter):
    """:class:`DelaySpectrumWienerFilter` whose delay power spectrum comes with every ``process`` call
    (``delay.py:1027-1053``)."""

    def process(self, ss, dps):
        """Estimate the delay spectrum of ``ss`` with ``dps`` as the signal covariance."""
        self.dps = dps
        return super().process(ss)


def nrml_evaluators(ctx, data_v, weight_v, fold_n, nbase, nsample, channel_ind, ndelay, window, *, remove_mean, time_frac, freq_frac, weight_boost, workspace_mib=1024):
    """The NRML problem of ``nbase`` baselines in batches: yields ``(b0, evaluator)``, a
    :class:`~draco_amd.analysis.delayopt.DeviceEvaluator` over the baselines ``b0 ...`` whose model and starting spectrum
    ``S0`` come from the prepare pass (the cuts, the means, the averaged weights) on the device.  ``window``: a name or
    ``None``; it is evaluated at ``channel_ind / ndelay``."""
    from .delayopt import MAX_CHAN, MAX_DELAY, DeviceEvaluator, matern_prior

    nchan = int(len(channel_ind))
    if not (1 <= nchan <= MAX_CHAN and 1 <= ndelay <= MAX_DELAY):
        raise ValueError(f"NRML: {nchan} channels and {ndelay} delays, the kernels take at most {MAX_CHAN} and {MAX_DELAY}")
    if nsample > 65535:
        raise ValueError(f"NRML: {nsample} samples, the kernels take at most 65535")
    chan = np.ascontiguousarray(channel_ind, dtype=np.int32)
    chan_d = ctx.to_device(chan)
    ones_d = ctx.to_device(np.ones(nchan, dtype=np.float64))
    Ci_d = ctx.to_device(matern_prior(ndelay))  # one inversion and one upload for all batches
    win = _window_coef(np.asarray(channel_ind) / ndelay, window)
    fold = (C.c_int64 * max(1, len(fold_n)))(*[int(x) for x in fold_n])
    per = max(1, min(65535, (int(workspace_mib) << 20) // DeviceEvaluator.bytes_per_baseline(ndelay, nchan, nsample)))
    for b0 in range(0, nbase, per):
        nb = min(per, nbase - b0)
        Xp = ctx.empty((nb, nsample + 1, 2 * nchan), np.float64)
        nzt = ctx.empty((nb, nsample), np.uint8)
        status = ctx.empty((nb,), np.int32)
        Xd = ctx.empty((nb, nsample, 2 * nchan), np.float64)
        nzt_d, status_d = ctx.empty((nb, nsample), np.uint8), ctx.empty((nb,), np.int32)
        # (the complex time domain and a unit coefficient, twice: with wiener = 1 the last row of Xp is twice the averaged
        # weight and status is the skip word; with wiener = 0 the rows of Xd are the mean-removed data themselves, and
        # its status, which also reports cut channels, is not used)
        for wiener, X, t, st in ((1, Xp, nzt, status), (0, Xd, nzt_d, status_d)):
            _lib.check(
                _lib.lib.dmm_delay_prepare(
                    ctx.handle, ndelay, nchan, nsample, nb, b0, len(fold_n), fold, C.byref(data_v), C.byref(weight_v), 1, wiener, int(bool(remove_mean)), float(time_frac), float(freq_frac),
                    float(weight_boost), ptr(ones_d), ptr(chan_d), ptr(X), ptr(t), ptr(st),
                )
            )
        ev = DeviceEvaluator.from_prepared(ctx, ndelay, chan, win, Xp, Xd, nzt, status, Ci=Ci_d)
        ctx.uses(Xp, Xd, nzt, status, nzt_d, status_d)
        yield b0, ev
    ctx.uses(chan_d, ones_d, Ci_d)


class DelayPowerSpectrumBase(DelayTransformBase):
    """What the delay power spectrum estimators share (``delay.py:744-818``, ``1114-1215``): the output container, a
    :class:`~draco_amd.core.containers.DelaySpectrum`.

    Attributes
    ----------
    nsamp : int
        The number of samples to compute for each power spectrum.  Default 1.
    save_samples : bool
        Add ``spectrum_samples [sample, baseline, delay]``, every sample of the chain.  Default False.
    save_spectrum_mask : bool
        Add ``spectrum_mask [baseline]``, set where a baseline was skipped or the estimator did not succeed.
        Default False.
    """

    _config_names = DelayTransformBase._config_names + ("nsamp", "save_samples")
    nsamp = 1
    save_samples = False

    def _create_output(self, ss, delays, coord_axes):
        """The baseline axis is the folded axis's own index map when one axis is folded, otherwise a count."""
        if isinstance(coord_axes, np.ndarray):
            bl = coord_axes
        elif len(coord_axes) == 1:
            bl = ss.index_map[coord_axes[0]]
        else:
            bl = int(np.prod([len(ss.index_map[ax]) for ax in coord_axes]))
        out = containers.DelaySpectrum(baseline=bl, delay=delays, sample=self.nsamp, attrs_from=ss, allocate=False)
        if isinstance(coord_axes, list):
            for ax in coord_axes:
                out.create_index_map(ax, ss.index_map[ax])
            out.attrs["baseline_axes"] = coord_axes
        out.attrs["freq"] = np.asarray(ss.freq)
        return out


class DelayPowerSpectrumNRML(DelayPowerSpectrumBase):
    """Estimate the delay power spectrum by NRML (``delay.py:1270-1301``): per baseline the maximum a posteriori of a
    Gaussian likelihood in ``log S`` under a Matern Gaussian-process prior, found by scipy's Newton-CG algorithm run
    for all baselines of a batch in lock step with every evaluation on the GPU
    (:mod:`draco_amd.analysis.delayopt`).

    Attributes
    ----------
    nsamp : int
        The cap on the number of iterations (and the length of the ``sample`` axis).
    maxpost_tol : float
        The convergence tolerance of the optimiser (its ``xtol``).  Default 1e-3; below it the reference's own iterates
        are decided by rounding in the line search.

    ``spectrum [baseline, delay]`` (on the device) is ``fftshift`` of the last iterate; ``spectrum_samples[-k:, b]``
    holds the ``k`` iterates of baseline ``b``, the start first, not shifted, zeros before them; ``spectrum_mask[b]``
    is set where the baseline was skipped by the cuts or the optimiser did not succeed (a covariance that is not
    positive definite included: nothing is raised).  A baseline that runs to the cap has ``nsamp + 1`` iterates: the
    reference would assign them into ``nsamp`` slots and raise; here the last ``nsamp`` are kept.
    ``complex_timedomain`` acts through the delay grid only, as in the reference.
    """

    _config_names = DelayPowerSpectrumBase._config_names + ("maxpost_tol",)
    maxpost_tol = 1e-3

    def process(self, ss):
        from .delayopt import newton_cg

        self._check()
        delays, channel_ind = self._calculate_delays(ss)
        ndelay = len(delays)
        ss.redistribute("freq")
        name, axes, waxes, fold = self._resolve(ss)
        fold_n = [len(ss.index_map[ax]) for ax in fold]
        nbase = int(np.prod(fold_n)) if fold_n else 1
        nsample = len(ss.index_map[self.sample_axis])
        ctx = Context.get()
        data, weight, data_v, weight_v, fold_n = self._prepare_inputs(ss, ctx, name, axes, waxes, fold)
        out = self._create_output(ss, delays, fold)
        spectrum = np.zeros((nbase, ndelay))
        samples = np.zeros((self.nsamp, nbase, ndelay)) if self.save_samples else None
        mask = np.zeros(nbase, dtype=bool)
        batches = nrml_evaluators(ctx, data_v, weight_v, fold_n, nbase, nsample, channel_ind, ndelay, self.window if self.apply_window else None, remove_mean=self.remove_mean,
                                  time_frac=self.time_frac, freq_frac=self.freq_frac, weight_boost=self.weight_boost, workspace_mib=self.workspace_mib)
        for b0, ev in batches:
            live = ev.base == 0
            mask[b0 : b0 + ev.nb] = ~live
            if not live.any():
                continue
            with np.errstate(divide="ignore"):
                x0 = np.where(live[:, None], np.log(ev.S0.cpu().numpy()), 0.0)
            for i, r in enumerate(newton_cg(ev, x0, maxiter=self.nsamp, xtol=self.maxpost_tol, active=live)):
                if not live[i]:
                    continue
                its = np.exp(np.array(r["x"]))
                spectrum[b0 + i] = np.fft.fftshift(its[-1])
                mask[b0 + i] = not r["success"]
                if samples is not None:
                    keep = its[-self.nsamp :]
                    samples[-len(keep) :, b0 + i] = keep
        ctx.uses(data, weight)
        out.attach("spectrum", ctx.to_device(spectrum))
        if samples is not None:
            out.add_dataset("spectrum_samples", allocate=False)
            out.datasets["spectrum_samples"] = containers.Dataset(host=samples, attrs={"axis": ["sample", "baseline", "delay"]})
        if self.save_spectrum_mask:
            out.add_dataset("spectrum_mask", allocate=False)
            out.datasets["spectrum_mask"] = containers.Dataset(host=mask, attrs={"axis": ["baseline"]})
        return out


class DelaySpectrumToPowerSpectrum(ContainerTask):
    """Compute a delay power spectrum from a delay spectrum (``delay.py:1061-1106``): the variance over the sample
    axis, restricted to the unmasked samples.  A baseline with every sample masked gives zero and is flagged in the
    output's ``spectrum_mask``."""

    def process(self, dspec):
        dspec.redistribute("baseline")
        ctx = Context.get()
        pspec = containers.DelaySpectrum(attrs_from=dspec, axes_from=dspec, allocate=False)
        ds = _dev_dataset(dspec.spectrum, ctx, np.complex128)
        if "spectrum_mask" in dspec.datasets:
            w = ~ctx.to_device(np.asarray(dspec.datasets["spectrum_mask"][:]).astype(np.uint8)).bool()[:, :, None]
        else:
            w = torch.ones((ds.shape[0], ds.shape[1], 1), dtype=torch.bool, device=ctx.device)
        cnt = w.sum(dim=1).to(torch.float64)
        mean = (ds * w).sum(dim=1) / cnt
        ps = (((ds - mean[:, None, :]).abs() ** 2) * w).sum(dim=1) / cnt
        nans = torch.isnan(ps)
        ps = torch.where(nans, torch.zeros_like(ps), ps).contiguous()
        pspec.attach("spectrum", ps)
        if "spectrum_mask" in dspec.datasets:
            pspec.add_dataset("spectrum_mask", allocate=False)
            pspec.datasets["spectrum_mask"] = containers.Dataset(host=nans.any(dim=-1).cpu().numpy(), attrs={"axis": ["baseline"]})
        return pspec


__all__ = [
    "DelayPowerSpectrumBase",
    "DelayPowerSpectrumNRML",
    "DelaySpectrumFFT",
    "DelaySpectrumToPowerSpectrum",
    "DelaySpectrumWienerFilter",
    "DelaySpectrumWienerFilterIteratePS",
    "DelayTransformBase",
    "delay_spectrum_fft",
    "delay_spectrum_wiener_filter",
    "fourier_matrix",
    "fourier_matrix_c2c",
    "fourier_matrix_c2r",
    "fourier_matrix_r2c",
]


# ---- the delay null-space filter (``delay.py:29-339``)


def null_filter_plan(freq, cuts, flags):
    """Which filters a container needs: ``(cut [nuniq], num_modes [nuniq], mask [nuniq, nfreq], index [nitem])``.

    ``cuts [nitem]``: the delay cut of every item in micro-seconds, ``flags [nitem, nfreq]``: its frequency mask.
    ``num_modes = int(4 ptp(freq) cut + 0.5)``, as the DAYENU paper recommends and the reference uses.  Items with equal
    ``(cut, mask)`` share one filter, numbered in order of first use."""
    freq = np.asarray(freq, dtype=np.float64)
    bandwidth = np.ptp(freq)
    keys, cut_u, k_u, mask_u = {}, [], [], []
    index = np.empty(len(cuts), dtype=np.int64)
    for it, cut in enumerate(cuts):
        key = (float(cut), flags[it].tobytes())
        if key not in keys:
            keys[key] = len(cut_u)
            cut_u.append(float(cut))
            k_u.append(int(4.0 * bandwidth * float(cut) + 0.5))
            mask_u.append(flags[it])
        index[it] = keys[key]
    return np.asarray(cut_u), np.asarray(k_u, dtype=np.int64), np.asarray(mask_u, dtype=np.uint8).reshape(len(cut_u), freq.size), index


class _NullFilterTask(ContainerTask):
    """What the two tasks share: mask pass, filter sharing, batched build, apply."""

    _config_names = ("delay_cut", "window", "workspace_mib")
    delay_cut = 0.1
    window = False
    workspace_mib = 1024  # device memory the filters of one batch and their factors may take

    def _filter(self, ctx, dtype, wdtype, layout, freq, cuts, ninner, nouter, datas, weight, join=False):
        """``cuts [nouter * ninner]``: delay cut of every item.  ``datas``: one side per beam; ``weight``: the side the
        masks come from, multiplied by them in place; ``join``: the ``nouter`` items of one inner index are one item of the
        reference (one mask pair from the samples of all of them)."""
        from .dayenu import _GROUP, apply_filters

        freq = np.ascontiguousarray(freq, dtype=np.float64)
        nfreq, nitem = freq.size, ninner * nouter
        if not 1 <= nfreq <= filters.NULL_MAX_ORDER:
            raise ValueError(f"{type(self).__name__}: {nfreq} frequencies, the kernels take 1 ... {filters.NULL_MAX_ORDER}")
        flag_d = ctx.empty((nouter, ninner, nfreq), np.uint8)
        _lib.check(_lib.lib.dmm_nullfilter_mask(ctx.handle, wdtype, layout, nfreq, ninner, nouter, int(join), C.byref(weight), ptr(flag_d)))
        flags = flag_d.cpu().numpy().reshape(nitem, nfreq)
        ctx.uses(flag_d)
        cut_u, k_u, mask_u, imat = null_filter_plan(freq, cuts, flags)
        nuniq = len(cut_u)
        self.log.debug(f"{nitem} items, {nuniq} distinct filters.")
        if nuniq == 0:
            return
        window = filters.null_filter_window(freq, self.window)
        freq_d = ctx.to_device(freq)
        group = _GROUP[dtype]
        ngroup = (ninner + group - 1) // group
        per = max(1, min(65535, (int(self.workspace_mib) << 20) // (8 * nfreq * (nfreq + int(k_u.max())))))
        for m0 in range(0, nuniq, per):
            m1 = min(nuniq, m0 + per)
            nf, status, _, _ = filters.build_null_filters(ctx, freq_d, cut_u[m0:m1], k_u[m0:m1], mask_u[m0:m1], window, workspace_mib=self.workspace_mib)
            sel = np.flatnonzero((imat >= m0) & (imat < m1))
            if status.any():
                bad = sel[status[imat[sel] - m0] != 0][0]
                raise RuntimeError(f"Failed to converge while processing baseline {bad % ninner}")
            local = np.full(nitem, -1, dtype=np.int32)
            local[sel] = imat[sel] - m0
            if layout == _lib.DMM_DAYENU_COLS:
                units = sel.astype(np.int32)
            else:
                units = np.unique((sel // ninner) * ngroup + (sel % ninner) // group).astype(np.int32)
            units_d, local_d = ctx.to_device(units), ctx.to_device(local)
            for data in datas:
                apply_filters(ctx, dtype, layout, nfreq, ninner, nouter, nf, local_d, None, units_d, len(units), data, None)
            ctx.uses(nf, units_d, local_d)
        ctx.uses(freq_d)


def _real_code(t):
    return _lib.DMM_DAYENU_F64 if t.dtype in (torch.float64, torch.complex128) else _lib.DMM_DAYENU_F32


class DelayFilter(_NullFilterTask):
    """Remove delays less than a given threshold (``delay.py:29-153``).

    The data are projected onto the null space that is orthogonal to any mode at low delays.  For this to work best
    the zero entries of the weights should factorise in frequency and time for each baseline.

    Attributes
    ----------
    delay_cut : float
        Delay value to filter at, in micro-seconds.  Default 0.1.
    za_cut : float
        Sine of the maximum zenith angle included in baseline-dependent delay filtering.  Default 1.0 (the horizon);
        zero turns the baseline-dependent cut off.
    extra_cut : float
        Increase the delay threshold beyond the baseline-dependent term.  Default 0.
    weight_tol : float
        Unused, as in the reference.  Default 1e-4.
    telescope_orientation : one of ('NS', 'EW', 'none')
        Whether the baseline-dependent delay cut is based on the north-south component, the east-west component or the
        full baseline length.  Default 'NS'.
    window : bool
        Apply the window function to the data when applying the filter.  Default False.

    The delay cut applied is ``max(za_cut * baseline / c + extra_cut, delay_cut)``.  Works in place on a
    ``SiderealStream`` or ``TimeStream`` and returns it with device-resident ``vis`` (complex64, or complex128 if it
    came so) and ``vis_weight``.  Per stack entry the frequencies, and the samples, with the most positive weights stay
    (``f_mask``, ``t_mask``); the weights are multiplied by both masks.  Entries with the same cut and ``f_mask`` share
    one filter.  ``RuntimeError`` if the SVD of a filter does not converge.  The whole band must be in this process.
    """

    _config_names = ("za_cut", "extra_cut", "weight_tol", "telescope_orientation")
    za_cut = 1.0
    extra_cut = 0.0
    weight_tol = 1e-4
    telescope_orientation = "NS"

    def read_config(self, params):
        super().read_config(params)
        if self.telescope_orientation not in ("NS", "EW", "none"):
            raise ValueError(f"telescope_orientation must be 'NS', 'EW' or 'none', not {self.telescope_orientation!r}")

    def setup(self, telescope):
        """Set the telescope needed to obtain baselines."""
        self.telescope = io.get_telescope(telescope)

    def _cuts(self, prod):
        """The delay cut of every stack entry, in micro-seconds."""
        pos = self.telescope.feedpositions
        baselines = pos[np.asarray(prod["input_a"], dtype=np.int64)] - pos[np.asarray(prod["input_b"], dtype=np.int64)]
        if self.telescope_orientation == "NS":
            baselines = abs(baselines[:, 1])  # Y baseline
        elif self.telescope_orientation == "EW":
            baselines = abs(baselines[:, 0])  # X baseline
        else:
            baselines = np.linalg.norm(baselines, axis=-1)  # Norm
        return np.maximum(self.za_cut * baselines / scipy.constants.c * 1e6 + self.extra_cut, self.delay_cut)

    def process(self, ss):
        """Filter out delays from a SiderealStream or TimeStream, in place."""
        from .dayenu import _side

        ss.redistribute(["input", "prod", "stack"])
        ctx = Context.get()
        cuts = self._cuts(ss.prodstack)
        vis = _dev_dataset(ss.vis, ctx, np.complex128 if np.dtype(ss.vis.dtype) == np.complex128 else np.complex64)
        weight = _dev_dataset(ss.weight, ctx, np.float32)
        nfreq, nstack, nt = (int(s) for s in vis.shape)
        if len(cuts) != nstack:
            raise ValueError(f"{len(cuts)} products for {nstack} stack entries")
        data = _side(vis, 2 * nt, 2 * nstack * nt, 1, 2 * nt, 0)
        wside = _side(weight, nt, nstack * nt, 1, nt, 0)
        self._filter(ctx, _real_code(vis), _lib.DMM_DAYENU_F32, _lib.DMM_DAYENU_COLS, ss.freq[:], cuts, nstack, 1, [data], wside)
        ss.vis.set_device(vis)
        ss.weight.set_device(weight)
        return ss


class DelayFilterBase(_NullFilterTask):
    """Remove delays less than a given threshold (``delay.py:156-339``).

    Attributes
    ----------
    delay_cut : float
        Delay value to filter at, in micro-seconds.  Default 0.1.
    window : bool
        Apply the window function to the data when applying the filter.  Default False.
    axis : str
        The main axis to iterate over; the delay cut can be varied for each element of it (:meth:`_delay_cut`).  If not
        set, the default for the container type: ``stack`` for a ``SiderealStream``, ``el`` for a ``RingMap``.
    dataset : str
        Apply the delay filter to this dataset.  If not set, the default for the container type (``vis``, ``map``).

    Works in place and returns the input container with the dataset and the weights on the device.  A ``RingMap`` has
    one filter per ``el``, from the masks of the weights of both polarisations together (``f_samp`` counts the ``(pol,
    ra)`` samples), as the reference's reshaping makes it; the weights have no beam axis: every beam and polarisation
    is filtered with the same matrix and the weights are multiplied by the masks once.  ``TypeError`` for a container without a
    frequency axis; ``NotImplementedError`` for ``HybridVisMModes`` and ``GridBeam`` (the reference's other two
    defaults), for other containers, and for an ``axis`` or ``dataset`` other than the default: those layouts have no
    apply path.  ``RuntimeError`` if the SVD of a filter does not converge.  The whole band must be in this process.
    """

    _config_names = ("axis", "dataset")
    axis = None
    dataset = None

    _defaults = ((containers.SiderealStream, "stack", "vis"), (containers.HybridVisMModes, "m", "vis"), (containers.RingMap, "el", "map"), (containers.GridBeam, "theta", "beam"))

    def setup(self, telescope=None):
        """Set the telescope needed to obtain baselines (kept for subclasses that cut by baseline)."""
        self.telescope = io.get_telescope(telescope) if telescope is not None else None

    def _delay_cut(self, ss, axis, ind):
        """Return the delay cut to use for entry ``ind`` of ``axis`` of the container, in micro-seconds."""
        return self.delay_cut

    def process(self, ss):
        """Filter out delays from a SiderealStream or a RingMap, in place."""
        from .dayenu import _side

        if not isinstance(ss, containers._FreqMixin):
            raise TypeError(f"Can only process FreqContainer instances. Got {type(ss)}.")
        for cls, axis, dset in self._defaults:
            if isinstance(ss, cls):
                break
        else:
            raise NotImplementedError(f"DelayFilterBase: no default axis known for {type(ss).__name__} containers, and only the default layouts run on the GPU")
        if (self.axis is not None and self.axis != axis) or (self.dataset is not None and self.dataset != dset):
            raise NotImplementedError(f"DelayFilterBase: only axis {axis!r} and dataset {dset!r} of a {cls.__name__} have an apply path, not {self.axis!r} / {self.dataset!r}")
        if cls not in (containers.SiderealStream, containers.RingMap):
            raise NotImplementedError(f"DelayFilterBase: the {cls.__name__} layout (axis {axis!r}) has no apply path on the GPU")
        ss.redistribute(axis)
        ctx = Context.get()
        nax = len(ss.index_map[axis])
        cuts = np.array([float(self._delay_cut(ss, axis, ind)) for ind in range(nax)])
        if cls is containers.SiderealStream:
            vis = _dev_dataset(ss.vis, ctx, np.complex128 if np.dtype(ss.vis.dtype) == np.complex128 else np.complex64)
            weight = _dev_dataset(ss.weight, ctx, np.float32)
            nfreq, nstack, nt = (int(s) for s in vis.shape)
            data = _side(vis, 2 * nt, 2 * nstack * nt, 1, 2 * nt, 0)
            wside = _side(weight, nt, nstack * nt, 1, nt, 0)
            self._filter(ctx, _real_code(vis), _lib.DMM_DAYENU_F32, _lib.DMM_DAYENU_COLS, ss.freq[:], cuts, nstack, 1, [data], wside)
            ss.vis.set_device(vis)
            ss.weight.set_device(weight)
            return ss
        rmap = _dev_dataset(ss.map, ctx, np.float32 if np.dtype(ss.map.dtype) == np.float32 else np.float64)
        weight = _dev_dataset(ss.weight, ctx, np.float32 if np.dtype(ss.weight.dtype) == np.float32 else np.float64)
        nbeam, npol, nfreq, nra, nel = (int(s) for s in rmap.shape)
        plane = nfreq * nra * nel
        datas = [_side(rmap[b], nra, nra * nel, nel, 1, plane) for b in range(nbeam)]
        wside = _side(weight, nra, nra * nel, nel, 1, plane)
        self._filter(ctx, _real_code(rmap), _real_code(weight), _lib.DMM_DAYENU_ITEMS, ss.freq[:], np.tile(cuts, npol), nel, npol, datas, wside, join=True)
        ss.map.set_device(rmap)
        ss.weight.set_device(weight)
        return ss
