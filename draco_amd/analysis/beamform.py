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

The ring-map half of the reference's module is here too: :class:`RingMapBeamForm` extracts the pixel containing each
source from a ``RingMap`` (``dmm_ringmap_extract``) and :class:`RingMapStack2D` stacks the patches around the sources into a
``Stack3D`` (``dmm_ringmap_stack3d``, both ``csrc/sourcestack.hip``).  The CIRS rule holds for them whenever the ring map
carries an ``lsd`` attribute; a ring map without one takes the catalogue's coordinates as they are.
"""

from __future__ import annotations

import numpy as np
import scipy.constants
import scipy.interpolate
import torch

from .. import _lib
from ..core import containers, io
from ..core.task import ContainerTask
from ..device import Context, ptr
from ..util import _fast_tools
from ..util.tools import baseline_vector, calculate_redundancy, polarization_map
from .sidereal import _search_nearest
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


class RingMapBeamForm(ContainerTask):
    """Beamform by extracting the pixel containing each source from a ``RingMap`` (``beamform.py:915-1094``).

    Much faster than :class:`BeamForm`, at the mercy of what was done to produce the ring map.  A ring map without an
    ``lsd`` attribute is taken to be in the epoch of the catalogue, whose coordinates are used as they are; with ``lsd``
    the catalogue must be marked ``attrs["coordinates"] == "CIRS"`` (see the module's docstring).

    The host finds the pixels in float64 exactly as the reference (``_source_ind``); ``dmm_ringmap_extract`` copies, so
    ``beam`` and ``weight`` (device resident) are bit-equal to the reference's.
    """

    def setup(self, telescope, ringmap):
        """``telescope``: anything ``io.get_telescope`` understands; ``ringmap``: the ``RingMap`` to extract from."""
        self.telescope = io.get_telescope(telescope)
        self.ringmap = ringmap

    def _map_tensors(self, ctx):
        """``(map [pol, freq, ra, el], weight source, rms?)`` on the device; the first beam of the map only."""
        rmm = _dev_dataset(self.ringmap.map, ctx, np.float64)[0].contiguous()
        if "weight" in self.ringmap.datasets:
            return rmm, _dev_dataset(self.ringmap.weight, ctx, np.float64).contiguous(), False
        return rmm, _dev_dataset(self.ringmap.rms, ctx, np.float64).contiguous(), True

    def process(self, catalog):
        """``catalog``: a ``SourceCatalog``.  Returns the ``FormedBeam`` of the sources inside the map."""
        ringmap = self.ringmap
        src_ra, src_dec = self._process_catalog(catalog)
        ra_ind, el_ind, src_ind = self._source_ind(src_ra, src_dec)
        nsrc = int(src_ind.size)

        formed_beam = containers.FormedBeam(object_id=catalog.index_map["object_id"][src_ind], axes_from=ringmap, attrs_from=catalog, distributed=True, allocate=False)
        formed_beam.datasets["position"] = containers.Dataset(host=np.array(catalog["position"][:][src_ind]), attrs={"axis": ["object_id"]})
        if "redshift" in catalog:
            formed_beam.add_dataset("redshift")
            formed_beam["redshift"][:] = catalog["redshift"][:][src_ind]

        npol, nfreq = len(ringmap.index_map["pol"]), len(ringmap.index_map["freq"])
        nra, nel = len(ringmap.index_map["ra"]), len(ringmap.index_map["el"])
        ctx = Context.get()
        fbb, fbw = ctx.empty((nsrc, npol, nfreq), np.float64), ctx.empty((nsrc, npol, nfreq), np.float64)
        if nsrc:
            rmm, rmw, rms = self._map_tensors(ctx)
            order = np.argsort(ra_ind.astype(np.int64) * nel + el_ind, kind="stable").astype(np.int32)
            ri_d, ei_d, or_d = (ctx.to_device(np.ascontiguousarray(x, dtype=np.int32)) for x in (ra_ind, el_ind, order))
            _lib.check(_lib.lib.dmm_ringmap_extract(ctx.handle, npol, nfreq, nra, nel, ptr(rmm), ptr(rmw), int(rms), nsrc, ptr(ri_d), ptr(ei_d), ptr(or_d), ptr(fbb), ptr(fbw)))
        formed_beam.attach("beam", fbb)
        formed_beam.attach("weight", fbw)
        return formed_beam

    def _process_catalog(self, catalog):
        """The catalogue's coordinates in the epoch of the map (``beamform.py:1000-1028``)."""
        if "position" not in catalog:
            raise ValueError("Input is missing a position table.")
        position = catalog["position"]
        if "lsd" not in self.ringmap.attrs:
            self.log.info("Input map has no epoch set, assuming that it matches the catalog.")
        elif catalog.attrs.get("coordinates") != "CIRS":
            lsd = self.ringmap.attrs["lsd"][0] if isinstance(self.ringmap.attrs["lsd"], np.ndarray) else self.ringmap.attrs["lsd"]
            icrs_to_cirs(position["ra"], position["dec"], self.telescope.lsd_to_unix(lsd))  # (raises: see the module's docstring)
        return np.array(position["ra"], dtype=np.float64), np.array(position["dec"], dtype=np.float64)

    def _source_ind(self, src_ra, src_dec):
        """Indices ``(ra_ind, el_ind, src_ind)`` of the pixels nearest to the sources that fall inside the map
        (``beamform.py:1030-1094``), in float64 NumPy."""
        src_el = np.sin(np.radians(src_dec - self.telescope.latitude))
        ra = np.asarray(self.ringmap.index_map["ra"], dtype=np.float64)
        el = np.asarray(self.ringmap.index_map["el"], dtype=np.float64)
        delta_ra = np.median(np.abs(np.diff(ra)))
        delta_el = np.median(np.abs(np.diff(el)))
        # (sources just below 360 deg may be closest to the first sample)
        ra_ind = _search_nearest(np.append(ra, 360.0 + ra[0]), src_ra) % ra.size
        ra_sep = src_ra - ra[ra_ind]
        ra_sep = (ra_sep + 180.0) % 360.0 - 180.0
        el_ind = _search_nearest(el, src_el)
        el_sep = src_el - el[el_ind]
        src_flag = (np.abs(ra_sep) > (0.5 * delta_ra)) | (np.abs(el_sep) > (0.5 * delta_el))
        if np.any(src_flag):
            self.log.info(f"There are {np.sum(src_flag)} (of {src_flag.size}) sources outside of the RA and Declination range covered by the map.")
        src_ind = np.flatnonzero(~src_flag)
        return ra_ind[src_ind], el_ind[src_ind], src_ind


class RingMapStack2D(RingMapBeamForm):
    """Stack ring maps on sources directly (``beamform.py:1097-1302``): the patch of ``(2 num_ra + 1) x (2 num_dec + 1)``
    pixels around every source, binned in frequency offset from the source's line, into a ``Stack3D``.

    Attributes
    ----------
    num_ra, num_dec : int
        The number of RA and DEC pixels to stack either side of the source.  Default 10.
    num_freq : int
        Number of final frequency channels either side of the source redshift to stack.  Default 256.
    freq_width : float
        Length of the frequency interval either side of the source in MHz; zero: the ring map's own resolution.
    weight : {"patch", "dec", "input"}
        ``"input"``: pixel by pixel as the map's weights (default); ``"patch"``: the inverse variance of the extracted
        patch; ``"dec"``: the inverse variance over RA of each declination strip.
    workspace_mib : int
        Device memory the partial sums of a pass may take.  The result does not depend on it.  Default 1024.

    The frequency axis of the map must be strictly monotonic.  A patch longer than the RA axis, or ``2 num_dec + 1 >
    nel``, raises ``ValueError`` (the reference indexes from the wrong end there).
    """

    _config_names = ("num_ra", "num_dec", "num_freq", "freq_width", "weight", "workspace_mib")
    num_ra = 10
    num_dec = 10
    num_freq = 256
    freq_width = 0.0
    weight = "input"
    workspace_mib = 1024

    def read_config(self, params):
        super().read_config(params)
        if self.weight not in ("patch", "dec", "input"):
            raise ValueError(f"Invalid weight parameter: {self.weight}")

    def process(self, catalog):
        """``catalog``: a ``SpectroscopicCatalog``.  Returns the ``Stack3D``."""
        from .sourcestack import _monotonic, stack_partials

        ringmap = self.ringmap
        src_ra, src_dec = self._process_catalog(catalog)
        if "redshift" not in catalog:
            raise ValueError("Input is missing a required redshift table.")
        src_z = np.asarray(catalog["redshift"]["z"], dtype=np.float64)
        ra_ind, el_ind, src_ind = self._source_ind(src_ra, src_dec)
        src_z = src_z[src_ind]

        freq = np.asarray(ringmap.freq, dtype=np.float64)
        ra = np.asarray(ringmap.index_map["ra"], dtype=np.float64)
        el = np.asarray(ringmap.index_map["el"], dtype=np.float64)
        dra = np.median(np.abs(np.diff(ra)))
        dell = np.median(np.abs(np.diff(el)))
        nra, nel, nfreq, npol = ra.size, el.size, freq.size, len(ringmap.index_map["pol"])
        if 2 * self.num_ra + 1 > nra or self.num_ra < 0:
            raise ValueError(f"a patch of {2 * self.num_ra + 1} pixels is longer than the RA axis ({nra})")
        if 2 * self.num_dec + 1 > nel or self.num_dec < 0:
            raise ValueError(f"a patch of {2 * self.num_dec + 1} pixels is longer than the el axis ({nel})")
        fdir = _monotonic(freq)
        if fdir == 0:
            raise ValueError("the frequency axis is not strictly monotonic")
        if nfreq > _lib.DMM_STACK_MAX_FREQ:
            raise ValueError(f"{nfreq} channels: at most {_lib.DMM_STACK_MAX_FREQ}")

        # does the RA axis wrap around from 360 to 0 deg?
        tol = dra / 100.0
        ra_wraps = bool(np.isclose(ra[-1] + dra, 360.0, atol=tol) and np.isclose(ra[0], 0.0, atol=tol))

        nbins = 2 * self.num_freq + 1
        if self.freq_width > 0:
            bin_edges = np.linspace(-self.freq_width, self.freq_width, nbins + 1, endpoint=True)
        else:
            df = np.median(np.abs(np.diff(freq)))
            bin_edges = (np.arange(-self.num_freq, self.num_freq + 2) - 0.5) * df
        if _monotonic(bin_edges) != 1:
            raise ValueError("bins must be monotonically increasing")

        # sources outside the band are dropped
        source_freq = NU21 / (1 + src_z)
        keep = ~((source_freq > freq.max()) | (source_freq < freq.min()))
        ra_ind, el_ind, source_freq = ra_ind[keep], el_ind[keep], source_freq[keep]
        nsrc = int(source_freq.size)

        ctx = Context.get()
        nrp, ndp = 2 * self.num_ra + 1, 2 * self.num_dec + 1
        n = npol * nbins * nrp * ndp
        partial, chunks, running = stack_partials(ctx, n, nsrc, self.workspace_mib)
        out_s, out_w = ctx.empty((npol, nrp, ndp, nbins), np.float64), ctx.empty((npol, nrp, ndp, nbins), np.float64)
        rmm = rmw = wdec = ri_d = ei_d = sf_d = None
        rms = False
        mode = {"input": _lib.DMM_STACK3D_INPUT, "dec": _lib.DMM_STACK3D_DEC, "patch": _lib.DMM_STACK3D_PATCH}[self.weight]
        if nsrc or self.weight == "dec":
            rmm, rmw, rms = self._map_tensors(ctx)
        if self.weight == "dec":
            rmvar = rmm.var(dim=2, unbiased=False)
            wdec = torch.where(rmvar < 3e-7, torch.zeros_like(rmvar), rmvar)
            wdec = torch.where(wdec == 0, torch.zeros_like(wdec), 1.0 / torch.where(wdec == 0, torch.ones_like(wdec), wdec)).contiguous()
        if nsrc:
            ri_d, ei_d = (ctx.to_device(np.ascontiguousarray(x, dtype=np.int32)) for x in (ra_ind, el_ind))
            sf_d = ctx.to_device(np.ascontiguousarray(source_freq))
        freq_d, edges_d = ctx.to_device(freq), ctx.to_device(np.ascontiguousarray(bin_edges, dtype=np.float64))
        _lib.check(_lib.lib.dmm_ringmap_stack3d(ctx.handle, npol, nfreq, nra, nel, ptr(rmm), ptr(rmw), int(rms), int(mode), ptr(wdec), nsrc, ptr(ri_d), ptr(ei_d), ptr(sf_d),
                                                ptr(freq_d), int(fdir < 0), nbins, ptr(edges_d), int(self.num_ra), int(self.num_dec), int(ra_wraps), ptr(partial), chunks,
                                                ptr(running), ptr(out_s), ptr(out_w)))

        delta_f = np.zeros(nbins, dtype=[("centre", float), ("width", float)])
        delta_f["centre"] = 0.5 * (bin_edges[1:] + bin_edges[:-1])
        delta_f["width"] = bin_edges[1:] - bin_edges[:-1]
        delta_ra = np.arange(-self.num_ra, self.num_ra + 1) * dra
        delta_dec = np.degrees(np.arcsin(np.arange(-self.num_dec, self.num_dec + 1) * dell))
        stack = containers.Stack3D(freq=delta_f, delta_ra=delta_ra, delta_dec=delta_dec, axes_from=ringmap, attrs_from=ringmap, allocate=False)
        stack.attrs["tag"] = catalog.attrs["tag"]
        stack.attach("stack", out_s)
        stack.attach("weight", out_w)
        return stack
