"""DPSS gap inpainting tasks on the GPU.

Drop-in for ``draco/analysis/interpolate.py``: :class:`DPSSFilter`, :class:`DPSSFilterBaseline`,
:class:`DPSSFilterDelay`, :class:`DPSSFilterMMode`, :class:`StokesIMixin`, :class:`DPSSFilterDelayStokesI`,
:class:`DPSSFilterMModeStokesI`, with the reference's config attributes, defaults and ``setup`` / ``process``
signatures.  The arithmetic is ``draco_amd.util.dpss`` (``csrc/dpss.hip``): every ``(stack, ra)`` column along
frequency, or ``(stack, freq)`` column along RA, is one symmetric positive definite system of the order of its basis,
solved in float64 on the device; ``vis`` and ``vis_weight`` of the output are device-resident (complex64 / float32).

Along ``freq`` a column's samples are ``nstack nra`` elements apart and adjacent RA samples are adjacent in memory;
along ``ra`` a column is contiguous.  Both are read where they lie: the stream is never transposed.

Differences from the reference, all stated where they apply: the bases are built on the host (``get_basis``) and cached
on the task, keyed by the samples and the cut (the reference recomputes them on every ``process``); a mask container
raises ``NotImplementedError``; a complex basis (non-zero ``centres``) raises ``NotImplementedError``; a column whose
matrix is not positive definite keeps its data, loses its weight and logs an error.  The independent axis must be
``stack`` (the only one of the default ``iter_axes`` that a stream has).
"""

from __future__ import annotations

import numpy as np
import scipy.constants

from ..core import io
from ..core.containers import Dataset
from ..core.task import ContainerTask
from ..device import Context
from ..util import dpss
from .transform import _dev_dataset

MAX_FREQ = 1024  # order along frequency
MAX_RA = 4096  # order along right ascension


class DPSSFilter(ContainerTask):
    """Fill data gaps using DPSS inpainting (``interpolate.py:13-190``), with one constant cutoff.

    Attributes
    ----------
    inpaint : bool
        If True, inpaint flagged values; otherwise return the filtered dataset.  Default True.
    axis : str
        The axis over which to inpaint, "freq" or "ra".  Default "freq".
    iter_axes : list[str]
        Independent axes over which to iterate; may name axes the dataset lacks, at least one must be present.
        Default ["stack", "el"].
    centres : list
        Top-hat window centres.  Anything but zeros makes the basis complex (``NotImplementedError``).
    halfwidths : list
        Window half-widths, as many as ``centres``.
    epsilon : float
        Wiener filter inverse signal covariance.  Default 1.0e-3.
    cutoff_frac : float
        Gaps wider than ``cutoff_frac * fs / max(halfwidths)`` samples are flagged again.  Default 1.0.
    copy : bool
        If True, return a new container and leave the input alone; otherwise work in place.  Default True.
    workspace_mib : int
        Device memory the matrices and right-hand sides of one batch of columns may take.  Default 1024.
    """

    _config_names = ("inpaint", "axis", "iter_axes", "centres", "halfwidths", "epsilon", "cutoff_frac", "copy", "workspace_mib")
    _axis_choices = ("freq", "ra")
    inpaint = True
    axis = "freq"
    iter_axes = ["stack", "el"]
    centres = None
    halfwidths = None
    epsilon = 1.0e-3
    cutoff_frac = 1.0
    copy = True
    workspace_mib = 1024

    def read_config(self, params):
        super().read_config(params)
        if self.axis not in self._axis_choices:
            raise ValueError(f"axis must be one of {self._axis_choices}, not {self.axis!r}")

    def setup(self, mask=None):
        """Use an optional mask dataset.

        The reference hands the whole mask array to every slice of the iteration axis (``interpolate.py:152``), which
        cannot broadcast for more than one slice; a mask container therefore raises ``NotImplementedError`` here and
        the samples to inpaint are those whose weight is zero.
        """
        if mask is not None:
            raise NotImplementedError(f"{type(self).__name__}: a mask container is not supported; samples with zero weight are inpainted")
        self.mask = None
        self._basis_cache = {}

    def process(self, data):
        """Inpaint visibility data of a ``SiderealStream`` or ``TimeStream``; returns a copy (``copy=True``) or the
        input container, with device-resident ``vis`` and ``vis_weight``."""
        try:
            samples = np.asarray(getattr(data, self.axis), dtype=np.float64)
        except AttributeError as exc:
            raise ValueError(f"Could not get axis `{self.axis}`.") from exc
        if not hasattr(self, "_basis_cache"):
            self._basis_cache = {}
        axes = list(data.vis.attrs["axis"])
        present = [a for a in self.iter_axes if a in axes]
        if not present:
            raise ValueError(f"No matching axes. Dataset has axes {axes}, but axes {tuple(self.iter_axes)} were requested.")
        if present != ["stack"] or len(axes) != 3 or axes[1] != "stack" or self.axis not in (axes[0], axes[2]):
            raise NotImplementedError(f"{type(self).__name__}: the GPU path iterates over `stack` of a [freq, stack, ra/time] dataset, got {axes} with iter_axes {self.iter_axes}")
        data.redistribute(self.iter_axes)
        n = samples.size
        limit = MAX_FREQ if self.axis == "freq" else MAX_RA
        if not 1 <= n <= limit:
            raise ValueError(f"{type(self).__name__}: {n} samples along {self.axis}, the kernels take 1 ... {limit}")
        ctx = Context.get()
        vis = _dev_dataset(data.vis, ctx, np.complex64)
        weight = _dev_dataset(data.weight, ctx, np.float32)
        n0, nstack, n2 = (int(s) for s in vis.shape)
        if n != (n0 if self.axis == axes[0] else n2):
            raise ValueError(f"{n} samples along {self.axis} for a dataset of shape {(n0, nstack, n2)}")
        self._nlocal = nstack
        self._set_sel(data)

        modes, amap, cutoff = self._get_basis(samples)
        amap = np.asarray(amap, dtype=np.int64).reshape(-1)
        if amap.size != nstack:
            raise ValueError(f"{amap.size} baselines for {nstack} stack entries")
        if self.copy:
            vout, wout = ctx.empty(vis.shape, np.complex64), ctx.empty(weight.shape, np.float32)
        else:
            vout, wout = vis, weight
        if self.axis == axes[0]:  # column (s, r) = s n2 + r, samples n1 n2 apart
            layout, ncs = (nstack * n2, 0, 1, nstack * n2), n2
        else:  # column (s, f) = s n0 + f starts at f nstack n2 + s n2, samples contiguous
            layout, ncs = (n0, n2, nstack * n2, 1), n0
        for u, basis in enumerate(modes):
            entries = np.flatnonzero(amap == u)
            if entries.size == 0:
                continue
            cols = (entries[:, np.newaxis] * ncs + np.arange(ncs)[np.newaxis, :]).reshape(-1)
            failed = dpss.run_columns(ctx, basis, self.epsilon, layout, cols, vis, weight, None, vout, wout, self.inpaint, cutoff, self.workspace_mib,
                                      getattr(self, "_timings", None))
            for s in np.unique(failed // ncs):
                self.log.error(f"Failed to factorise the covariance of {int((failed // ncs == s).sum())} of {ncs} columns while processing stack entry {int(s)} "
                               f"[{basis.k} modes, epsilon {self.epsilon:g}]; their data is unchanged and their weight zero.")
        ctx.uses(vis, weight)

        if self.copy:
            import copy as _copy

            out = data.copy(shared=("vis", "vis_weight"))
            for name, t in (("vis", vout), ("vis_weight", wout)):
                out.datasets[name] = Dataset(dev=t, attrs=_copy.deepcopy(data.datasets[name].attrs))
        else:
            out = data
            out.vis.set_device(vout)
            out.weight.set_device(wout)
        return out

    def _set_sel(self, data):
        """Extract selection along local axis (a single process holds every stack entry)."""
        self._local_sel = slice(0, self._nlocal)

    def _device_basis(self, samples, halfwidths, centres):
        """The basis of one cut on the device, cached on the task by (samples, cut)."""
        key = (samples.tobytes(), tuple(np.atleast_1d(np.asarray(halfwidths, dtype=np.float64)).tolist()), tuple(np.atleast_1d(np.asarray(centres, dtype=np.float64)).tolist()))
        if key not in self._basis_cache:
            cov = dpss.make_covariance(samples, halfwidths, centres)
            self._basis_cache[key] = dpss.DeviceBasis(Context.get(), dpss.get_basis(cov), type(self).__name__)
        return self._basis_cache[key]

    def _get_basis(self, samples):
        """The bases (one here), the map from stack entry to basis, and the flagging cutoff in samples."""
        modes = self._device_basis(samples, self.halfwidths, self.centres)
        amap = [0] * (self._local_sel.stop - self._local_sel.start)
        fs = 1 / np.median(abs(np.diff(samples)))
        cutoff = self.cutoff_frac * fs / np.max(self.halfwidths)
        return [modes], amap, cutoff


class DPSSFilterBaseline(DPSSFilter):
    """Inpaint with a baseline-dependent cut (``interpolate.py:193-269``): the base class that selects the baselines
    and builds one basis per unique cut; subclasses give ``_get_baseline_cuts``.

    Attributes
    ----------
    telescope_orientation : one of ('NS', 'EW', 'none')
        Whether the baseline-dependent cut is based on the north-south component, the east-west component or the full
        baseline length.  Default 'NS'.
    """

    _config_names = ("telescope_orientation",)
    telescope_orientation = "NS"

    def read_config(self, params):
        super().read_config(params)
        if self.telescope_orientation not in ("NS", "EW", "none"):
            raise ValueError(f"telescope_orientation must be 'NS', 'EW' or 'none', not {self.telescope_orientation!r}")

    def setup(self, telescope, mask=None):
        """Load a telescope object with baseline information; ``mask`` as for :class:`DPSSFilter`."""
        self.telescope = io.get_telescope(telescope)
        super().setup(mask)

    def _set_sel(self, data):
        """Set the local baselines."""
        prod = data.prodstack
        sel = self.telescope.feedmap[(prod["input_a"], prod["input_b"])]
        self._baselines = np.asarray(self.telescope.baselines)[sel]

    def _get_basis(self, samples):
        """One basis per unique cut, the map from stack entry to basis, and the flagging cutoff of the widest cut."""
        cuts = self._get_baseline_cuts()
        cuts, amap = np.unique(cuts, return_inverse=True)
        modes = []
        for ii, cut in enumerate(cuts):
            self.log.debug(f"Making unique covariance {ii + 1}/{len(cuts)} with cut={cut}.")
            modes.append(self._device_basis(samples, cut, 0.0))
        fs = 1 / np.median(abs(np.diff(samples)))
        cutoff = self.cutoff_frac * fs / np.max(cuts)  # (a single process: the reference's MIN all-reduce is the identity)
        return modes, amap, cutoff

    def _get_baseline_cuts(self):
        """Get an array of cutoffs for each baseline."""
        raise NotImplementedError()


class DPSSFilterDelay(DPSSFilterBaseline):
    """Inpaint along frequency with a baseline-dependent delay cut (``interpolate.py:272-312``).

    Attributes
    ----------
    axis : str
        "freq" is the only accepted value.
    za_cut : float
        Sine of the maximum zenith angle included in the baseline-dependent delay cut.  Default 1 (the horizon); zero
        turns the baseline-dependent term off.
    extra_cut : float
        Increase the delay threshold beyond the baseline-dependent term.  Default 0.
    """

    _config_names = ("za_cut", "extra_cut")
    _axis_choices = ("freq",)
    axis = "freq"
    za_cut = 1.0
    extra_cut = 0.0

    def _get_baseline_cuts(self):
        """Delay cut of every baseline in micro-seconds, rounded to three decimals."""
        if self.telescope_orientation == "NS":
            blen = abs(self._baselines[:, 1])
        elif self.telescope_orientation == "EW":
            blen = abs(self._baselines[:, 0])
        else:
            blen = np.linalg.norm(self._baselines, axis=1)
        delay_cut = self.za_cut * blen / scipy.constants.c * 1.0e6 + self.extra_cut
        delay_cut = np.maximum(delay_cut, self.halfwidths[0])
        return np.round(delay_cut, decimals=3)


class DPSSFilterMMode(DPSSFilterBaseline):
    """Inpaint along right ascension with a baseline-dependent m cut (``interpolate.py:315-351``); ``axis`` is "ra".
    The telescope must give ``freq_start`` (the highest frequency in MHz) and ``latitude``."""

    _axis_choices = ("ra",)
    axis = "ra"

    def _get_baseline_cuts(self):
        """The maximum m expected for every baseline, per degree of RA, rounded to two decimals."""
        if self.telescope_orientation == "NS":
            blen = abs(self._baselines[:, 0])
        elif self.telescope_orientation == "EW":
            blen = abs(self._baselines[:, 1])
        else:
            blen = np.linalg.norm(self._baselines, axis=1)
        freq = self.telescope.freq_start
        dec = np.deg2rad(self.telescope.latitude)
        mcut = (np.pi / 180) * freq * 1e6 * blen / (scipy.constants.c * np.cos(dec))
        mcut = np.maximum(mcut, self.halfwidths[0])
        return np.round(mcut, decimals=2)


class StokesIMixin:
    """Change baseline selection assuming Stokes I only: the stack axis holds the baseline vectors."""

    def _set_sel(self, data):
        """Set the local baselines."""
        self._baselines = np.asarray(data.index_map["stack"])[slice(0, self._nlocal)]


class DPSSFilterDelayStokesI(StokesIMixin, DPSSFilterDelay):
    """Inpaint Stokes I with baseline-dependent delay cut."""


class DPSSFilterMModeStokesI(StokesIMixin, DPSSFilterMMode):
    """Inpaint Stokes I with baseline-dependent m-mode cut."""


__all__ = ["DPSSFilter", "DPSSFilterBaseline", "DPSSFilterDelay", "DPSSFilterDelayStokesI", "DPSSFilterMMode", "DPSSFilterMModeStokesI", "StokesIMixin"]
