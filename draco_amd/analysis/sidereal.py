"""Sidereal regridding and day stacking on the GPU.

Drop-in for the two tasks of ``draco/analysis/sidereal.py`` that stand between time-ordered data and the m-mode path:

* :class:`SiderealRegridder`  ``sidereal.py:160-278``
* :class:`SiderealStacker`    ``sidereal.py:834-1080``

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
            out_grid = self.start + np.arange(self.samples, dtype=np.float64) / self.samples * (self.end - self.start)
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
