"""Beamform visibilities to the location of known sources, on the GPU.

Drop-in for the catalogue part of ``draco/analysis/beamform.py``: :class:`BeamFormBase`, :class:`BeamForm`,
:class:`BeamFormCat`, :class:`BeamFormExternalMixin`, :class:`BeamFormExternal`, :class:`BeamFormExternalCat` and
:func:`icrs_to_cirs`, with the reference's config attributes, defaults and ``setup`` / ``process`` /
``process_finish`` signatures.  A sidereal stream or time stream is fringestopped to every source of a catalogue, summed
over baselines and (``collapse_ha``) hour angle; ``beam`` and ``weight`` of the returned :class:`FormedBeam` /
:class:`FormedBeamHA` are device resident (float64).

The arithmetic is ``draco_amd.util._fast_tools`` (``csrc/srcbeam.hip``).  ``_process_data`` gathers every processed
polarisation once (``prepare``); ``process`` walks the catalogue in chunks sized for ``workspace_mib`` of device tables
(primary beam and the uncollapsed sums ``F``, both ``[pol, source, freq, ha]`` float64, and the hour-angle tables): per
chunk the host computes the windows and ``cos`` / ``sin`` of hour angle and declination in float64 (NumPy, as the
reference), the primary beam table, and the device forms and collapses the beams.  The frequency axis of the container
is the rank's own (frequencies shard across ranks as in the other tasks); no collective is needed.

Two deliberate differences from the reference:

* Catalogues must carry ``attrs["coordinates"] == "CIRS"``.  The ICRS conversion needs an ephemeris package (skyfield)
  that is not available here: :func:`icrs_to_cirs`, and a catalogue that is not marked CIRS, raise
  ``NotImplementedError``.
* A window longer than the RA axis (``2 int(ha_side) + 1 > nra``) raises ``ValueError``; the reference wraps indices once
  in each direction only and then indexes from the wrong end.
"""

from __future__ import annotations

import numpy as np
import scipy.constants
import scipy.interpolate
import torch

from ..core import containers, io
from ..core.task import ContainerTask
from ..device import Context
from ..util import _fast_tools
from ..util.tools import baseline_vector, calculate_redundancy, polarization_map
from .transform import _dev_dataset

NU21 = 1420.40575177  # MHz
C = scipy.constants.c
SIDEREAL_S = 1.0 / (1.0 + 1.0 / 365.259636)  # sidereal second in SI seconds

_FULLPOL = ["XX", "XY", "YX", "YY"]


def icrs_to_cirs(ra, dec, epoch, apparent=True):
    """Convert positions from ICRS to CIRS at a given epoch (``beamform.py:1773-1804``).

    Not available: the conversion needs an ephemeris package (skyfield and its ephemeris files).  Convert the catalogue
    beforehand and mark it with ``attrs["coordinates"] = "CIRS"``."""
    raise NotImplementedError("icrs_to_cirs needs an ephemeris package (skyfield) that is not available; pass a catalogue in CIRS coordinates (attrs['coordinates'] = 'CIRS')")


class BeamFormBase(ContainerTask):
    """Base class for beam forming tasks (``beamform.py:32-665``).  Not to be used directly.

    Attributes
    ----------
    collapse_ha : bool
        Sum over hour angle / time to complete the beamforming.  Default True.
    polarization : str
        'I' (Stokes I only), 'full' ('XX', 'XY', 'YX', 'YY'; default), 'copol' ('XX', 'YY'), 'stokes' (not implemented).
    weight : str
        How to weight the redundant baselines when adding: 'natural' (by redundancy; default), 'uniform' or
        'inverse_variance' (by the weight dataset).
    no_beam_model : bool
        Do not include a primary beam factor in the weights.
    timetrack : float
        How long (seconds) to track sources at each side of transit.  Default 900.
    variable_timetrack : bool
        Scale the tracking time by the secant of the declination.  Default False.
    freqside : int
        Number of frequencies to process at each side of the source.  Default (None) processes all.
    workspace_mib : int
        Device memory the per-chunk tables (primary beam, uncollapsed sums, hour-angle tables) may take.  Default 1024.
    """

    _config_names = ("collapse_ha", "polarization", "weight", "no_beam_model", "timetrack", "variable_timetrack", "freqside", "workspace_mib")
    collapse_ha = True
    polarization = "full"
    weight = "natural"
    no_beam_model = False
    timetrack = 900.0
    variable_timetrack = False
    freqside = None
    workspace_mib = 1024
    data_available = True

    def read_config(self, params):
        super().read_config(params)
        if self.polarization not in ("I", "full", "copol", "stokes"):
            raise ValueError(f"Invalid polarization parameter: {self.polarization}")
        if self.weight not in ("natural", "uniform", "inverse_variance"):
            raise ValueError(f"Invalid weight parameter: {self.weight}")
        if self.freqside is not None:
            self.freqside = int(self.freqside)

    def setup(self, manager):
        """Generic setup: ``manager`` holds the telescope (``ProductManager``, ``BeamTransfer`` or a telescope)."""
        self.telescope = io.get_telescope(manager)
        self.latitude = np.deg2rad(self.telescope.latitude)

        if self.polarization == "I":
            self.process_pol = ["XX", "YY"]
            self.return_pol = ["I"]
        elif self.polarization == "full":
            self.process_pol = list(_FULLPOL)
            self.return_pol = self.process_pol
        elif self.polarization == "copol":
            self.process_pol = ["XX", "YY"]
            self.return_pol = self.process_pol
        else:
            raise RuntimeError("Stokes parameters are not implemented")
        self.npol = len(self.process_pol)
        self.map_pol_feed = {pstr: list(self.telescope.polarisation).index(pstr) for pstr in ["X", "Y"]}

        if self.variable_timetrack and not self.collapse_ha:
            raise NotImplementedError("Must collapse over hour angle if tracking sources for declination dependent amount of time.")

    # ---- the catalogue on the host: windows, hour angles, frequency masks
    def _windows(self):
        """Per source: ``ra_index [nsource, W]`` (sample of every slot of the window, -1: no such slot), ``ha [nsource,
        W]`` (radians, zero where there is no slot), ``fmask [nsource, nfreq]`` (frequencies the source processes) and
        ``skipped [nsource]`` -- ``beamform.py:205-258, 399-454``."""
        nra = len(self.ra)
        nsrc = self.nsource
        dec = np.radians(self.sdec)
        if self.variable_timetrack:
            ha_side = np.array([int(self.ha_side / np.cos(d)) for d in dec], dtype=np.int64)
        else:
            ha_side = np.full(nsrc, int(self.ha_side), dtype=np.int64)
        if nsrc and 2 * int(ha_side.max()) + 1 > nra:
            raise ValueError(f"a window of {2 * int(ha_side.max()) + 1} samples is longer than the RA axis ({nra})")
        W = 2 * int(ha_side.max()) + 1 if nsrc else self.nha
        ra_index = np.full((nsrc, W), -1, dtype=np.int32)
        ha = np.zeros((nsrc, W), dtype=np.float64)
        skipped = np.zeros(nsrc, dtype=bool)
        fmask = np.ones((nsrc, self.nfreq), dtype=bool)
        for src in range(nsrc):
            if self.freqside is not None:
                sfreq_index = np.argmin(abs(self.freq["centre"] - self.sfreq[src]))
                fmask[src] = False
                fmask[src, max(0, sfreq_index - self.freqside) : min(self.nfreq, sfreq_index + self.freqside + 1)] = True
                if not fmask[src].any():
                    skipped[src] = True
                    continue
            if self.is_sstream:
                sra_index = np.searchsorted(self.ra, self.sra[src])  # the insertion point, may be nra
            else:
                transit_diff = abs(self.ra - self.sra[src])
                sra_index = np.argmin(transit_diff)
                if transit_diff[sra_index] > 1.5 * (self.ra[1] - self.ra[0]):
                    skipped[src] = True  # does not transit in the data
                    continue
            hs = int(ha_side[src])
            idx = np.arange(sra_index - hs, sra_index + hs + 1, dtype=np.int32)
            if self.is_sstream:
                idx[idx < 0] += nra
                idx[idx >= nra] -= nra
                mask = np.ones(idx.size, dtype=bool)
            else:
                mask = (idx >= 0) & (idx < nra)
            good = idx[mask]
            h = np.deg2rad(self.ra[good] - self.sra[src])
            h = (h + np.pi) % (2.0 * np.pi) - np.pi
            slots = np.flatnonzero(mask)
            ra_index[src, slots] = good
            ha[src, slots] = h
        fmask[skipped] = False
        return ra_index, ha, fmask, skipped

    def process(self):
        """Perform the beamforming for the parsed data and catalogue; returns a ``FormedBeam`` (``collapse_ha``) or a
        ``FormedBeamHA`` whose ``beam`` and ``weight`` are device tensors."""
        self._initialize_beam_with_data()
        ctx = Context.get()
        object_id = self.source_cat.index_map["object_id"]
        pol = np.array(self.return_pol)
        if self.collapse_ha:
            formed_beam = containers.FormedBeam(freq=self.freq, object_id=object_id, pol=pol, distributed=True)
        else:
            formed_beam = containers.FormedBeamHA(freq=self.freq, ha=np.arange(self.nha, dtype=np.int64), object_id=object_id, pol=pol, distributed=True)
        formed_beam.attrs["tag"] = "_".join([tag for tag in [self.tag_data, self.tag_catalog] if tag is not None])
        formed_beam["position"][:] = self.source_cat["position"][:]
        if "redshift" in self.source_cat:
            formed_beam.add_dataset("redshift")
            formed_beam["redshift"][:] = self.source_cat["redshift"][:]

        ra_index, ha, fmask, skipped = self._windows()
        W = ra_index.shape[1]
        shape = (self.nsource, len(self.return_pol), self.nfreq) + (() if self.collapse_ha else (W,))
        fbb, fbw = ctx.zeros(shape, np.float64), ctx.zeros(shape, np.float64)
        if not self.collapse_ha:
            formed_beam.ha[:] = ha

        # the device tables of a chunk, per source: F and the primary beam [pol, freq, W] float64, ut / vt [W]
        per_source = 8 * W * (self.npol * self.nfreq * (1 if self.no_beam_model else 2) + 2) + 4 * W + self.nfreq
        chunk = max(1, int((int(self.workspace_mib) << 20) // per_source))
        live = np.flatnonzero(~skipped)
        dec = np.radians(self.sdec)
        stokes_i = self.polarization == "I"
        for c0 in range(0, live.size, chunk):
            rows = live[c0 : c0 + chunk]
            ut, vt = _fast_tools.phase_tables(dec[rows, np.newaxis], self.latitude, np.cos(ha[rows]), np.sin(ha[rows]))
            fm = fmask[rows] if self.freqside is not None else None
            F = ctx.empty((self.npol, rows.size, self.nfreq, W), np.float64)
            for p in range(self.npol):
                _fast_tools.form(ctx, self.vis[p], self.sumweight[p], self.bvec[p][0], self.bvec[p][1], ut, vt, ra_index[rows], fm, out=F[p])
            pb = None
            if self.collapse_ha and not self.no_beam_model:  # (the uncollapsed output does not use the primary beam)
                pb = ctx.to_device(self._beam_table(dec[rows], ha[rows]), np.float64)
            _fast_tools.collapse(ctx, F, pb, self.SW, self.SW2, ra_index[rows], fm, rows, fbb, fbw, self.collapse_ha, self.weight == "inverse_variance", stokes_i)
        formed_beam.attach("beam", fbb)
        formed_beam.attach("weight", fbw)
        return formed_beam

    def process_finish(self):
        """Drop the copies of the data."""
        for attr in ["vis", "visweight", "bvec", "sumweight", "SW", "SW2"]:
            try:
                delattr(self, attr)
            except AttributeError:
                pass

    def _initialize_beam_with_data(self):
        """Index of the data's frequencies in the telescope's frequency axis (``beamform.py:456-471``)."""
        if not self.no_beam_model:
            self.freq_local_telescope_index = np.array([np.argmin(np.abs(nu - self.telescope.frequencies)) for nu in self.freq_local])

    def _beam_table(self, dec, ha):
        """Primary beam power ``[pol, source, freq, W]`` float64 of a chunk (``dec [n]``, ``ha [n, W]``, radians)."""
        return np.stack([self._beamfunc(pol, dec, ha) for pol in self.process_pol])

    def _beamfunc(self, pol, dec, ha):
        """``telescope.beam(feed, freq, angpos)`` once per (feed, frequency) for the whole chunk: ``angpos`` has the
        reference's shape ``(n, 2)`` with ``n = sources x W`` and the call returns ``(n, 2)`` complex; the power is the
        real part of ``sum bii conj(bjj)`` over the last axis, as the reference's assignment into a float64 array
        (``beamform.py:473-513``)."""
        nsrc, W = ha.shape
        angpos = np.stack([np.repeat(0.5 * np.pi - dec, W), ha.ravel()], axis=1)
        out = np.zeros((nsrc, self.nfreq, W), dtype=np.float64)
        for ff, freq in enumerate(self.freq_local_telescope_index):
            bii = self.telescope.beam(self.map_pol_feed[pol[0]], freq, angpos)
            bjj = self.telescope.beam(self.map_pol_feed[pol[1]], freq, angpos) if pol[0] != pol[1] else bii
            out[:, ff, :] = np.real(np.sum(bii * bjj.conjugate(), axis=1)).reshape(nsrc, W)
        return out

    def _process_data(self, data):
        """Parse the data and stage every processed polarisation on the device (``beamform.py:515-630``)."""
        self.tag_data = data.attrs["tag"] if "tag" in data.attrs else None
        if "ra" in data.index_map:
            self.is_sstream = True
            self.ra = np.asarray(data.index_map["ra"], dtype=np.float64)
            if "lsd" not in data.attrs:
                raise ValueError("SiderealStream must have an LSD attribute to calculate the epoch.")
            self.epoch = self.telescope.lsd_to_unix(np.mean(data.attrs["lsd"]))
            dt = 240.0 * SIDEREAL_S * np.median(np.abs(np.diff(self.ra)))
        else:
            self.is_sstream = False
            self.ra = np.asarray(self.telescope.unix_to_lsa(data.time), dtype=np.float64)
            self.epoch = data.time.mean()
            dt = np.median(np.abs(np.diff(data.time)))
        self.freq = data.index_map["freq"]
        self.nfreq = len(self.freq)
        self.freq_local = self.freq["centre"]
        self.ha_side = self.timetrack / dt
        self.nha = 2 * int(self.ha_side) + 1
        if self.nha > len(self.ra):
            raise ValueError(f"a window of {self.nha} samples is longer than the RA axis ({len(self.ra)})")

        needs_redundancy = self.weight != "inverse_variance"
        if needs_redundancy and "input_flags" not in data.datasets:
            raise ValueError(f"weight={self.weight!r} needs the input_flags dataset of the data to count the redundancy.")

        ctx = Context.get()
        polmap = polarization_map(data.index_map, self.telescope)
        bvec_m = baseline_vector(data.index_map, self.telescope)
        vis = _dev_dataset(data.vis, ctx, np.complex64)
        weight = _dev_dataset(data.weight, ctx, np.float32)
        redundancy = None
        if needs_redundancy:  # counted on the host, uploaded once for all polarisations
            count = calculate_redundancy(data.datasets["input_flags"][:], data.index_map["prod"][:], data.reverse_map["stack"]["stack"][:], int(vis.shape[1]))
            redundancy = ctx.to_device(count, np.float32)
        self.vis, self.sumweight, self.bvec, SW, SW2 = [], [], [], [], []
        for pol in self.process_pol:
            polmask = polmap == _FULLPOL.index(pol)
            visT, ws, sw, sw2 = _fast_tools.prepare(ctx, vis, weight, np.flatnonzero(polmask), self.weight, redundancy)
            self.vis.append(visT)
            self.sumweight.append(ws)
            SW.append(sw)
            SW2.append(sw2)
            # baselines in wavelengths per frequency, float64 on the host: (2, nfreq, nvis)
            bvec = bvec_m[:, np.newaxis, polmask] * self.freq_local[np.newaxis, :, np.newaxis] * 1e6 / C
            self.bvec.append(ctx.to_device(np.copy(bvec, order="C"), np.float64))
        self.SW, self.SW2 = torch.stack(SW), torch.stack(SW2)

    def _process_catalog(self, catalog):
        """Take positions, line frequencies and tag from a catalogue (``_process_data`` must have run: without an
        epoch the data was not available, and ``process`` returns None)."""
        if "position" not in catalog:
            raise ValueError("Input is missing a position table.")
        self.data_available = hasattr(self, "epoch")
        if not self.data_available:
            self.log.warning("Epoch not set. Was the requested data not available?")
            return
        position = catalog["position"]
        if catalog.attrs.get("coordinates") != "CIRS":
            icrs_to_cirs(position["ra"], position["dec"], self.epoch)  # (raises: see the module's docstring)
        self.sra, self.sdec = (np.array(position[col], dtype=np.float64) for col in ("ra", "dec"))
        self.nsource = self.sra.size
        if self.freqside is not None:
            if "redshift" not in catalog:
                raise ValueError("Input is missing a required redshift table.")
            self.sfreq = NU21 / (1.0 + np.asarray(catalog["redshift"]["z"], dtype=np.float64))  # MHz
        self.source_cat = catalog
        self.tag_catalog = catalog.attrs.get("tag")

    def _form(self, catalog, data=None):
        """Parse ``data`` (unless ``setup`` already has), then the catalogue, and form the beams."""
        if data is not None:
            self._process_data(data)
        self._process_catalog(catalog)
        return BeamFormBase.process(self) if self.data_available else None


class BeamForm(BeamFormBase):
    """One source catalogue, given to ``setup(manager, source_cat)``; ``process(data)`` forms its beams on every
    dataset that comes by."""

    def setup(self, manager, source_cat):
        super().setup(manager)
        self.catalog = source_cat

    def process(self, data):
        """``data``: ``SiderealStream`` or ``TimeStream``.  Returns the ``FormedBeam`` / ``FormedBeamHA``."""
        return self._form(self.catalog, data=data)


class BeamFormCat(BeamFormBase):
    """One dataset, given to ``setup(manager, data)`` and staged on the device there; ``process(source_cat)`` forms
    the beams of every catalogue that comes by."""

    def setup(self, manager, data):
        super().setup(manager)
        self._process_data(data)

    def process(self, source_cat):
        """``source_cat``: ``SourceCatalog`` or ``SpectroscopicCatalog``.  Returns the ``FormedBeam`` / ``FormedBeamHA``."""
        return self._form(source_cat)


class _GridBeamModel:
    """Bivariate splines through a ``GridBeam`` in celestial coordinates, on (declination, hour angle) in radians: for
    every frequency and wanted polarisation one through the power beam (real part, zero where the weight is not
    positive) and one through the 0 / 1 map of where the weight is positive."""

    def __init__(self, gbeam, pols):
        self.freq = np.asarray(gbeam.freq)
        self.pols = list(pols)
        grid_pols = [str(p) for p in gbeam.pol]
        hour = (np.asarray(gbeam.phi, dtype=np.float64) + 180.0) % 360.0 - 180.0  # into -180 ... 180, then ascending
        order = np.argsort(hour)
        x, y = np.radians(np.asarray(gbeam.theta, dtype=np.float64)), np.radians(hour[order])
        beam, weight = gbeam.beam[:][:, :, 0], gbeam.weight[:][:, :, 0]  # the one input: [freq, pol, theta, phi]
        self.power, self.valid = {}, {}
        for pol in self.pols:
            ip = grid_pols.index(pol)
            for ff in range(self.freq.size):
                seen = weight[ff, ip][:, order] > 0.0
                self.power[ff, pol] = scipy.interpolate.RectBivariateSpline(x, y, np.where(seen, beam[ff, ip][:, order].real, 0.0))
                self.valid[ff, pol] = scipy.interpolate.RectBivariateSpline(x, y, seen.astype(np.float32))

    def __call__(self, pol, dec, ha):
        """``[n, freq, W]`` for ``dec [n]`` and ``ha [n, W]``, evaluated point by point; zero where the interpolated
        validity is 0.01 or more away from one (some of the grid under the point was masked)."""
        decs, has = np.repeat(dec, ha.shape[1]), ha.ravel()
        out = np.empty((ha.shape[0], self.freq.size, ha.shape[1]), dtype=np.float64)
        for ff in range(self.freq.size):
            ok = np.abs(self.valid[ff, pol](decs, has, grid=False) - 1.0) < 0.01
            out[:, ff, :] = np.where(ok, self.power[ff, pol](decs, has, grid=False), 0.0).reshape(ha.shape)
        return out


class BeamFormExternalMixin:
    """Beamform with an external model of the primary beam, the first argument of ``setup``; the others go to the
    task it is mixed into.  Use :class:`BeamFormExternal` and :class:`BeamFormExternalCat`."""

    def setup(self, beam, *args):
        super().setup(*args)
        self._initialize_beam(beam)

    def _initialize_beam(self, beam):
        """Only ``GridBeam`` containers are understood."""
        if not isinstance(beam, containers.GridBeam):
            raise ValueError(f"Do not recognize beam container: {beam.__class__}")
        self._initialize_grid_beam(beam)

    def _initialize_grid_beam(self, gbeam):
        """``gbeam``: power beam on (theta, phi) = (declination, hour angle) in degrees with a single input, which
        serves every baseline of a polarisation."""
        if gbeam.coords != "celestial":
            raise RuntimeError("GridBeam must be converted to celestial coordinates for beamforming.")
        if len(gbeam.input) > 1:
            raise NotImplementedError("Do not support input-dependent beams at the moment.")
        self._grid_model = _GridBeamModel(gbeam, getattr(self, "process_pol", [str(p) for p in gbeam.pol]))
        self._beamfunc = self._grid_beam
        self.log.info("Grid beam initialized.")

    def _initialize_beam_with_data(self):
        """The beam must come on the data's frequencies."""
        if not np.array_equal(self.freq_local, self._grid_model.freq):
            raise RuntimeError("Beam and visibility frequency axes do not match.")

    def _grid_beam(self, pol, dec, ha):
        """The grid beam's power for a chunk: ``[n, freq, W]`` for ``dec [n]`` and ``ha [n, W]`` in radians."""
        return self._grid_model(pol, dec, ha)


class BeamFormExternal(BeamFormExternalMixin, BeamForm):
    """:class:`BeamForm` with an external beam model: ``setup(beam, manager, source_cat)``."""


class BeamFormExternalCat(BeamFormExternalMixin, BeamFormCat):
    """:class:`BeamFormCat` with an external beam model: ``setup(beam, manager, data)``."""
