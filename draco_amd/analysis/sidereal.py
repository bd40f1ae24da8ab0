"""Sidereal regridding and day stacking on the GPU.

Drop-in for the two tasks of ``draco/analysis/sidereal.py`` that stand between time-ordered data and the m-mode path:

* :class:`SiderealRegridder`  ``sidereal.py:160-278``
* :class:`SiderealStacker`    ``sidereal.py:834-1080``
* :class:`SiderealRegridderGP`  ``sidereal.py:281-346`` (``csrc/gp.hip``)

and the second family of ways onto the RA grid (``csrc/rebin.hip``):

* :class:`SiderealRegridderNearest`, :class:`SiderealRegridderLinear`, :class:`SiderealRegridderCubic`  ``sidereal.py:349-547``
* :class:`SiderealRebinner`, :class:`RebinGradientCorrection`  ``sidereal.py:550-831``

Same class names, config attributes, ``setup`` / ``process`` / ``process_finish`` signatures and exceptions.  The
arithmetic runs in ``libdraco_amd.so`` (``csrc/regrid.hip``); outputs and the stacker's running state stay on the
device, so ``SiderealRegridder -> SiderealStacker -> MModeTransform -> DirtyMapMaker`` never crosses PCIe.
"""

from __future__ import annotations

import numpy as np
import scipy.constants
import torch

from .. import _lib
from ..core import containers
from ..core.task import ContainerTask
from ..device import Context, ptr
from .transform import LanczosRegridder, _dev_dataset


class SiderealRegridder(LanczosRegridder):
    """Take a sidereal day's worth of data, and put it onto a regular grid (``sidereal.py:160-278``).

    ``down_mix``: mix the visibilities down with the fringe rate of a source at zenith before the interpolation and
    back up after it; both products are fused into the regrid kernel's load and store.
    """

    _config_names = ("down_mix",)
    down_mix = False

    def process(self, data):
        self.log.info(f"Regridding LSD:{data.attrs['lsd']}")
        data.redistribute("freq")

        # Fetch which LSD this is to set bounds
        self.start = data.attrs["lsd"]
        self.end = self.start + 1

        if "time" in data.index_map:
            source_samples = self.observer.unix_to_lsd(data.time)
        elif "ra" in data.index_map:
            source_samples = self.start + data.ra / 360.0
        else:
            raise TypeError(f"Invalid input data container {data.__class__.__name__}. Expected container with a `time` or an `ra` axis.")

        for name in data.datasets.keys():
            if name not in {"vis", "vis_weight"}:
                self.log.info(f"Skipping dataset `{name}` - only `vis` and `vis_weight` are supported.")

        mix = None
        if self.down_mix:
            self.log.info("Downmixing before regridding.")
            ctx = Context.get()
            out_grid = self._mix_up_grid()
            omega, mask = self._get_fringe_rate(data.freq, data.prodstack)
            mix = (
                ctx.to_device(omega.reshape(-1), np.float64),
                ctx.to_device(np.broadcast_to(mask[np.newaxis, :], omega.shape).reshape(-1), np.float32),
                ctx.to_device(self._dphi(np.asarray(source_samples, dtype=np.float64)), np.float64),
                ctx.to_device(self._dphi(out_grid), np.float64),
            )

        new_grid, sts, ni = self._regrid(data.vis, data.weight, source_samples, mix=mix)

        sdata = containers.SiderealStream(attrs_from=data, axes_from=data, ra=self.samples, allocate=False)
        sdata.redistribute("freq")
        sdata.attach("vis", sts)
        sdata.attach("vis_weight", ni)
        sdata.attrs["lsd"] = self.start
        sdata.attrs["tag"] = f"lsd_{self.start:.0f}"
        return sdata

    def _mix_up_grid(self):
        """The output samples' LSDs as the mix-up sees them."""
        return self.start + np.arange(self.samples, dtype=np.float64) / self.samples * (self.end - self.start)

    @staticmethod
    def _dphi(lsd):
        """The local sidereal angle (``sidereal.py:270-271``)."""
        return 2.0 * np.pi * (lsd - np.floor(lsd))

    def _get_fringe_rate(self, freq, prod):
        """``(omega [nfreq, nstack], mask [nstack])``: the fringe rate of every row for ha = 0, dec = latitude, and
        the feed mask of its baseline (``sidereal.py:256-269``)."""
        aa, bb = prod["input_a"], prod["input_b"]
        mask = self.observer.feedmask[(aa, bb)].astype(np.float32)
        lmbda = scipy.constants.c / (np.asarray(freq, dtype=np.float64) * 1e6)
        u = self.observer.baselines[np.newaxis, :, 0] / lmbda[:, np.newaxis]
        omega = -2.0 * np.pi * u * np.cos(np.radians(self.observer.latitude))
        return omega, mask

    def _get_phase(self, freq, prod, lsd):
        """The mixing phase ``[nfreq, nstack, len(lsd)]`` as the reference forms it (``sidereal.py:256-278``); the
        kernel evaluates the same expression from :meth:`_get_fringe_rate` and :meth:`_dphi` -- host-side checks."""
        omega, mask = self._get_fringe_rate(freq, prod)
        dphi = self._dphi(np.asarray(lsd, dtype=np.float64))
        return mask[np.newaxis, :, np.newaxis] * np.exp(-1.0j * omega[:, :, np.newaxis] * dphi[np.newaxis, np.newaxis, :])


class SiderealRegridderGP(SiderealRegridder):
    r"""Regrid onto the sidereal day using Gaussian Process Regression (``sidereal.py:281-346``).

    A Matern-5/2 kernel of ``kernel_width`` grid cells with ``epsilon`` on the diagonal; per frequency the kernel matrix
    of the unflagged samples is truncated to a band, factored, and the projection applied to every stack
    (:mod:`draco_amd.util.gaussian_process`, ``csrc/gp.hip``).  Frequencies with the same flags share a factorisation.
    Raises ``scipy.linalg.LinAlgError`` if a truncated matrix is not positive definite.

    ``mask_cutoff``: distance (in input samples) from the `n`\th nearest unflagged input sample within which an output
    sample is kept.  ``mask_cutoff_partition``: that `n`, counted from zero.
    """

    _config_names = ("mask_cutoff", "mask_cutoff_partition")
    mask_cutoff = 1.7
    mask_cutoff_partition = 1

    def _mix_up_grid(self):
        # the grid this regridder returns carries no LSD offset, and the mix-up is formed from that grid
        return np.arange(self.samples, dtype=np.float64) / self.samples

    def _regrid(self, vis, weight, times, mix=None, timings=None):
        from ..util import gaussian_process

        ctx = Context.get()
        vis_d = _dev_dataset(vis, ctx, np.complex64)
        w_d = _dev_dataset(weight, ctx, np.float32)
        if len(vis_d.shape) != 3:
            raise NotImplementedError(f"SiderealRegridderGP regrids [freq, stack, time] streams; vis has shape {tuple(vis_d.shape)}.")
        # a regular grid, padded at either end to suppress interpolation issues
        pad = 5 * self.kernel_width
        grid = np.arange(-pad, self.samples + pad, dtype=np.float64) / self.samples
        # the kernels are normalised to a day that starts at zero
        times = np.asarray(times, dtype=np.float64) - self.start
        kernel_spec = {"name": "matern", "width": self.kernel_width, "alpha": 1.0, "nu": 2.5, "epsilon": self.epsilon}
        vout, wout = gaussian_process.resample_device(
            ctx, vis_d, w_d, times, grid, cutoff_dist=self.mask_cutoff, cutoff_partition=self.mask_cutoff_partition, kernel_spec=kernel_spec, pad=pad, samples=self.samples, mix=mix,
            timings=timings
        )
        return grid[pad:-pad].copy(), vout, wout


def _inz(x):
    """``invert_no_zero``: 1 / x, 0 where x is 0."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x == 0, 0.0, 1.0 / np.where(x == 0, 1.0, x))


def _search_nearest(x, xeval):
    """Index into the sorted ``x`` of the point nearest each ``xeval``; of two equally near, the later one
    (``sidereal.py:349-359``)."""
    nxt = np.searchsorted(x, xeval, side="left")
    prev = np.maximum(0, nxt - 1)
    nxt = np.minimum(x.size - 1, nxt)
    return np.where(np.abs(xeval - x[prev]) < np.abs(xeval - x[nxt]), prev, nxt)


class _DirectRegridder(SiderealRegridder):
    """Interpolators that read a few input samples per grid point: the host finds the taps, their coefficients and the
    grid points to flag, in float64 with the reference's expressions; ``dmm_regrid_interp`` gathers."""

    def _taps(self, lsd, grid):
        """``(tap [ntap, samples] int, coeff [ntap, samples] float64, bad [samples] bool)``."""
        raise NotImplementedError

    def _regrid(self, vis, weight, lsd, mix=None):
        from ..util import regrid

        ctx = Context.get()
        vis_d = _dev_dataset(vis, ctx, np.complex64)
        w_d = _dev_dataset(weight, ctx, np.float32)
        lsd = np.asarray(lsd, dtype=np.float64)
        # a regular grid
        interp_grid = np.arange(0, self.samples, dtype=np.float64) / self.samples
        interp_grid = interp_grid * (self.end - self.start) + self.start
        tap, coeff, bad = self._taps(lsd, interp_grid)
        lead, nt = tuple(vis_d.shape[:-1]), int(vis_d.shape[-1])
        sts, ni = regrid.regrid_interp(ctx, vis_d.reshape(-1, nt), w_d.reshape(-1, nt), tap.astype(np.int32), coeff, bad.astype(np.uint8), mix)
        return interp_grid, sts.reshape(*lead, self.samples), ni.reshape(*lead, self.samples)


class SiderealRegridderNearest(_DirectRegridder):
    """Regrid onto the sidereal day using nearest neighbour interpolation (``sidereal.py:362-383``)."""

    def _taps(self, lsd, grid):
        index = _search_nearest(lsd, grid)
        # flagged if the nearest sample is more than one sample spacing away: incomplete sidereal coverage
        delta = np.median(np.abs(np.diff(lsd)))
        bad = np.abs(lsd[index] - grid) > delta
        return index[np.newaxis, :], np.ones((1, grid.size)), bad


class SiderealRegridderLinear(_DirectRegridder):
    """Regrid onto the sidereal day using linear interpolation (``sidereal.py:386-461``)."""

    def _taps(self, lsd, grid):
        ind2 = np.searchsorted(lsd, grid, side="left")
        ind1 = ind2 - 1
        # outside the range the data cover: extrapolated from the two end samples, and flagged
        below = ind1 == -1
        above = ind2 == lsd.size
        ind1 = np.where(below, 0, np.where(above, lsd.size - 2, ind1))
        ind2 = np.where(below, 1, np.where(above, lsd.size - 1, ind2))
        delta = np.median(np.abs(np.diff(lsd)))
        distant = (np.abs(lsd[ind1] - grid) > delta) | (np.abs(lsd[ind2] - grid) > delta)
        dx1 = grid - lsd[ind1]
        dx2 = lsd[ind2] - grid
        norm = _inz(dx1 + dx2)
        return np.stack([ind1, ind2]), np.stack([dx2 * norm, dx1 * norm]), below | above | distant


class SiderealRegridderCubic(_DirectRegridder):
    """Regrid onto the sidereal day using cubic Hermite spline interpolation (``sidereal.py:464-547``)."""

    def _taps(self, lsd, grid):
        index = np.searchsorted(lsd, grid, side="left")
        index = np.stack([index + i for i in range(-2, 2)])  # the four samples around each grid point
        below = np.any(index < 0, axis=0)
        above = np.any(index >= lsd.size, axis=0)
        index = np.clip(index, 0, lsd.size - 1)
        delta = np.median(np.abs(np.diff(lsd)))
        distant = np.any(np.abs(grid - lsd[index]) > (2.0 * delta), axis=0)
        u = (grid - lsd[index[1]]) * _inz(lsd[index[2]] - lsd[index[1]])
        coeff = np.zeros((4, u.size), dtype=np.float64)
        coeff[0] = u * ((2 - u) * u - 1)
        coeff[1] = u**2 * (3 * u - 5) + 2
        coeff[2] = u * ((4 - 3 * u) * u + 1)
        coeff[3] = u**2 * (u - 1)
        coeff *= 0.5
        return index, coeff, below | above | distant


class SiderealRebinner(SiderealRegridder):
    """Regrid a sidereal day of data by binning (``sidereal.py:550-731``): every time sample gives each RA bin the
    fraction of its width that overlaps the bin.

    The output carries ``nsample`` and ``effective_ra``, the weighted centre of the samples of each bin, which
    :class:`RebinGradientCorrection` removes afterwards.  One pass of ``dmm_rebin`` over the input; all four output
    datasets stay on the device.  Input datasets beyond ``vis`` / ``vis_weight`` are refused, and the time stamps must
    not decrease (``NotImplementedError``).

    ``weight``: ``"uniform"`` or ``"inverse_variance"``.
    """

    _config_names = ("weight",)
    weight = "inverse_variance"

    def read_config(self, params):
        super().read_config(params)
        if self.weight not in ("uniform", "inverse_variance"):
            raise ValueError(f"weight must be 'uniform' or 'inverse_variance', not {self.weight!r}")

    def process(self, data):
        import inspect

        from ..util import regrid

        self.log.info(f"Rebinning LSD {data.attrs['lsd']:.0f} with {self.weight} weighting.")
        container_map = {
            containers.TimeStream: containers.SiderealStream,
            containers.SiderealStream: containers.SiderealStream,
            containers.HybridVisStream: containers.HybridVisStream,
        }
        OutputContainer = None
        for cls in inspect.getmro(data.__class__):  # subclasses of the mapped containers count
            OutputContainer = container_map.get(cls)
            if OutputContainer is not None:
                break
        if OutputContainer is None:
            raise TypeError(f"No valid container mapping.\nGot {data.__class__}.\nMappings exist for {list(container_map.keys())}.")
        extra = [name for name in data.datasets if name not in ("vis", "vis_weight")]
        if extra:
            raise NotImplementedError(f"SiderealRebinner rebins vis and vis_weight only; the input also holds {extra}.")
        data.redistribute("freq")

        self.start = data.attrs["lsd"]
        self.end = self.start + 1
        if "ra" in data.index_map:
            timestamp_lsd = self.start + data.ra / 360.0
        else:
            timestamp_lsd = self.observer.unix_to_lsd(data.time)
        timestamp_lsd = np.asarray(timestamp_lsd, dtype=np.float64)

        sdata = OutputContainer(ra=self.samples, axes_from=data, attrs_from=data, allocate=False)
        sdata.add_dataset("effective_ra", allocate=False)
        sdata.add_dataset("nsample", allocate=False)
        sdata.redistribute("freq")

        # the median width of a time sample, the regular grid of RA bins, the rebinning matrix
        width_t = np.median(np.abs(np.diff(timestamp_lsd)))
        target_lsd = np.linspace(self.start, self.end, self.samples, endpoint=False)
        ctx = Context.get()
        plan = regrid.RebinPlan(ctx, timestamp_lsd, target_lsd, width_t, self.start, sdata.index_map["ra"])
        vis_d = _dev_dataset(data.vis, ctx, np.complex64)
        w_d = _dev_dataset(data.weight, ctx, np.float32)
        nt = int(vis_d.shape[-1])
        mode = _lib.DMM_REBIN_UNIFORM if self.weight == "uniform" else _lib.DMM_REBIN_INVERSE_VARIANCE
        hybrid = OutputContainer is containers.HybridVisStream
        ssv, ssw, ssn, sera = regrid.rebin(ctx, plan, vis_d.reshape(-1, nt), w_d.reshape(-1, nt), mode, nsample_f32=hybrid)
        ctx.uses(plan.row_ptr_d, plan.sample_index_d, plan.value_d, plan.tile_span_d, plan.lsd_d, plan.ra_d)
        sdata.attach("vis", ssv.reshape(*vis_d.shape[:-1], self.samples))
        sdata.attach("vis_weight", ssw.reshape(*w_d.shape[:-1], self.samples))
        sdata.attach("nsample", ssn.reshape(*w_d.shape[:-1], self.samples))
        sdata.attach("effective_ra", sera.reshape(*w_d.shape[:-1], self.samples))
        return sdata


class RebinGradientCorrection(ContainerTask):
    """Apply a linear gradient correction to shift RA samples to bin centres (``sidereal.py:734-831``).

    ``setup`` takes the stream the local gradient is formed from -- it needs full sidereal coverage, and may be the
    rebinned stream itself; ``process`` corrects a stream in place on the device (``dmm_rebin_gradient``) and drops its
    ``effective_ra``.  A stream without ``effective_ra`` passes through untouched.
    """

    def setup(self, sstream_ref):
        self.sstream_ref = sstream_ref

    def process(self, sstream):
        from ..util import regrid

        self.sstream_ref.redistribute("freq")
        sstream.redistribute("freq")
        try:
            era = sstream.effective_ra
        except KeyError:
            self.log.info(f"Dataset of type ({type(sstream)}) does not have an effective ra dataset. No correction will be applied.")
            return sstream
        if len(sstream.vis.shape) != 3:
            raise NotImplementedError(f"RebinGradientCorrection corrects [freq, stack, ra] streams; vis has shape {sstream.vis.shape}.")
        ctx = Context.get()
        ref_era_d = ref_ra_d = None
        try:  # the reference's own effective RA if it has one (it may be the stream itself), else its regular RA axis
            ref_era_d = _dev_dataset(self.sstream_ref.effective_ra, ctx, np.float32)
        except KeyError:
            ref_ra_d = ctx.to_device(self.sstream_ref.ra, np.float64)
        nra = int(sstream.vis.shape[-1])
        vis_d = _dev_dataset(sstream.vis, ctx, np.complex64)
        w_d = _dev_dataset(sstream.weight, ctx, np.float32)
        era_d = _dev_dataset(era, ctx, np.float32)
        ra_d = ctx.to_device(sstream.ra, np.float64)
        ref_vis_d = _dev_dataset(self.sstream_ref.vis, ctx, np.complex64)
        ref_w_d = _dev_dataset(self.sstream_ref.weight, ctx, np.float32)
        if tuple(ref_vis_d.shape) != tuple(vis_d.shape):
            raise ValueError(f"reference stream of shape {tuple(ref_vis_d.shape)} does not match the stream's {tuple(vis_d.shape)}")
        regrid.rebin_gradient(
            ctx, vis_d.reshape(-1, nra), w_d.reshape(-1, nra), era_d.reshape(-1, nra), ra_d, ref_vis_d.reshape(-1, nra), ref_w_d.reshape(-1, nra),
            None if ref_era_d is None else ref_era_d.reshape(-1, nra), ref_ra_d
        )
        ctx.uses(ra_d, ref_ra_d)
        sstream.vis.set_device(vis_d)  # corrected in place: the device copy is the valid one
        sstream.weight.set_device(w_d)
        # the effective ra dataset is not needed anymore
        del sstream["effective_ra"]
        return sstream


def _ensure_list(x):
    if hasattr(x, "__iter__") and not isinstance(x, str):
        return list(x)
    return [x]


class SiderealStacker(ContainerTask):
    """Take in a set of sidereal days, and stack them up (``sidereal.py:834-1080``).

    Also computes the variance over sidereal days with West's update (1979).  One fused kernel per day; the running
    state (``vis``, ``vis_weight``, ``nsample``, ``sample_variance``, the sum of squared coefficients) lives on the
    device from the first day to ``process_finish``.  Datasets beyond those (``effective_ra``, ``*freq_cov*``) are
    refused with ``NotImplementedError``.
    """

    _config_names = ("tag", "weight", "with_sample_variance")
    tag = "stack"
    weight = "inverse_variance"
    with_sample_variance = False

    stack = None

    def read_config(self, params):
        super().read_config(params)
        if self.weight not in ("uniform", "inverse_variance"):
            raise ValueError(f"weight must be 'uniform' or 'inverse_variance', not {self.weight!r}")

    def process(self, sdata):
        if (self.stack is not None) and not isinstance(sdata, type(self.stack)):
            raise TypeError(f"type(sdata) (={type(sdata)}) does not match type(stack) (={type(self.stack)}).")
        extra = [name for name in sdata.datasets if name not in ("vis", "vis_weight", "nsample")]
        if extra:
            raise NotImplementedError(f"SiderealStacker stacks vis, vis_weight and nsample only; the input also holds {extra}.")

        sdata.redistribute("ra")
        if "lsd" in sdata.attrs:
            input_lsd = sdata.attrs["lsd"]
        elif "csd" in sdata.attrs:
            input_lsd = sdata.attrs["csd"]
        else:
            input_lsd = -1
        input_lsd = _ensure_list(input_lsd)

        ctx = Context.get()
        if self.stack is None:
            self.stack = type(sdata)(axes_from=sdata, attrs_from=sdata, allocate=False)
            self.stack.add_dataset("nsample", allocate=False)
            shape = self.stack.dataset_shape("vis")
            self._vis = ctx.zeros(shape, np.complex64)
            self._weight = ctx.zeros(shape, np.float32)
            self._nsample = ctx.zeros(shape, np.int16).view(torch.uint16)  # (allocated through int16: every torch build fills those)
            self._sum_coeff_sq = self._var = None
            if self.with_sample_variance:
                self.stack.add_dataset("sample_variance", allocate=False)
                self._var = ctx.zeros((3, *shape), np.float32)
                self._sum_coeff_sq = ctx.zeros(shape, np.float32)
            self.lsd_list = []
        elif tuple(sdata.vis.shape) != tuple(self._vis.shape):
            raise ValueError(f"day of shape {tuple(sdata.vis.shape)} does not match the stack's {tuple(self._vis.shape)}")

        self.log.info(f"Adding LSD {input_lsd} to stack with {self.weight} weighting.")
        self.lsd_list += input_lsd

        dvis = _dev_dataset(sdata.vis, ctx, np.complex64)
        dw = _dev_dataset(sdata.weight, ctx, np.float32)
        dns = ctx.to_device(np.ascontiguousarray(sdata.datasets["nsample"][:], dtype=np.uint16)) if "nsample" in sdata.datasets else None
        _lib.check(
            _lib.lib.dmm_sidereal_stack_add(
                ctx.handle, self._mode(), int(self.with_sample_variance), ptr(dvis), ptr(dw), ptr(dns), ptr(self._vis), ptr(self._weight), ptr(self._nsample), ptr(self._sum_coeff_sq), ptr(self._var), self._vis.numel()
            )
        )
        ctx.uses(dvis, dw, dns)

    def _mode(self):
        return _lib.DMM_STACK_UNIFORM if self.weight == "uniform" else _lib.DMM_STACK_INVERSE_VARIANCE

    def process_finish(self):
        ctx = Context.get()
        self.stack.attrs["tag"] = self.tag
        self.stack.attrs["lsd"] = np.array(self.lsd_list)
        _lib.check(
            _lib.lib.dmm_sidereal_stack_finish(ctx.handle, self._mode(), int(self.with_sample_variance), ptr(self._weight), ptr(self._nsample), ptr(self._sum_coeff_sq), ptr(self._var), self._vis.numel())
        )
        self.stack.attach("vis", self._vis)
        self.stack.attach("vis_weight", self._weight)
        self.stack.attach("nsample", self._nsample)
        if self.with_sample_variance:
            self.stack.attach("sample_variance", self._var)
        self.stack.redistribute("freq")
        return self.stack
