"""Instrumental-noise tasks for simulated streams.

Drop-in for ``GaussianNoise`` (``draco/synthesis/noise.py:178-284``) and ``SampleNoise``
(``:287-374``): same config attributes and ``setup``/``process`` signatures, in-place
modification of the input container like the reference.  These are input generation for
BASELINE config 5: random numbers come from a host ``np.random.Generator``
(the reference's ``RandomTask.rng`` [3P]); nothing here is on the timed hot path.

``GaussianNoiseDataset`` / ``MultipleGaussianNoiseDatasets`` (``:48-175``) are host side as well.
``FreqCorrelatedNoise`` / ``MultipleFreqCorrelatedNoise`` (``:377-474``) draw on the host, so that a seed gives the
reference's realisation, and colour the draw on the GPU (``csrc/noisemodel.hip``).
"""

from __future__ import annotations

import numpy as np

from ..core import containers, io
from ..core.task import CaputConfigError, ContainerTask, PipelineStopIteration
from ..util import random, tools

STELLAR_S = 1.0 / 1.002737909350795  # length of a sidereal second in SI seconds (caput.astro.constants [3P])


def _cmap(i, j, n):
    """Upper-triangle product index of the feed pair (i <= j) (``tools.py:21-39``)."""
    if i > j:
        i, j = j, i
    return (n * (n + 1) // 2) - ((n - i) * (n - i + 1) // 2) + (j - i)


def _prodstack(data):
    """Representative input pair per stacked product, conjugation applied (``containers.py:211-229``)."""
    prod = data.index_map["prod"]
    stack = data.index_map.get("stack")
    if stack is None or stack.dtype.names is None or "prod" not in stack.dtype.names:
        return prod
    t = prod[stack["prod"]].copy()
    conj = stack["conjugate"].astype(bool)
    t["input_a"] = np.where(conj, prod[stack["prod"]]["input_b"], prod[stack["prod"]]["input_a"])
    t["input_b"] = np.where(conj, prod[stack["prod"]]["input_a"], prod[stack["prod"]]["input_b"])
    return t


class _RandomTask(ContainerTask):
    seed = None
    _config_names = ("seed",)
    _rng = None

    @property
    def rng(self):
        if self._rng is None:
            self._rng = np.random.default_rng(self.seed)
        return self._rng

    @rng.setter
    def rng(self, value):
        self._rng = value


class ReceiverTemperature(ContainerTask):
    """Add a basic receiver temperature term into the data (``noise.py:21-45``).

    An uncorrelated, frequency and time independent offset: it only reaches the auto-correlations.  The random
    fluctuations that go with it come from :class:`SampleNoise` afterwards.

    Attributes
    ----------
    recv_temp : float
        The receiver temperature in Kelvin.
    """

    recv_temp = 0.0
    _config_names = ("recv_temp",)

    def process(self, data):
        pairs = _prodstack(data)
        autos = np.flatnonzero(pairs["input_a"] == pairs["input_b"])
        vis = data.vis[:]
        vis[:, autos] += self.recv_temp
        data.vis[:] = vis
        return data


class GaussianNoise(_RandomTask):
    """Add Gaussian distributed noise to a visibility dataset (``noise.py:178-284``).

    Attributes
    ----------
    recv_temp : float
        The temperature of the noise to add.
    ndays : float
        Multiplies the number of samples in each measurement.
    set_weights : bool
        Set the weights to ``1/sigma**2``.
    add_noise : bool
        Add the noise (False: only set the weights).
    """

    recv_temp = 50.0
    ndays = 733.0
    set_weights = True
    add_noise = True
    _config_names = ("recv_temp", "ndays", "set_weights", "add_noise")
    telescope = None

    def setup(self, manager=None):
        self.telescope = io.get_telescope(manager) if manager is not None else None

    def _samples_per_product(self, data, nprod):
        """Independent samples behind each (stacked) product of ``data``: ``int(ndays * dt * df) * redundancy``.

        The radiometer count uses the first channel's width for the whole band, as the reference does
        (``noise.py:243-244``).  A stream that matches the telescope's unique baselines is taken to be redundancy
        stacked; the full triangle of its inputs counts every product once; anything else is refused (``:250-256``).
        """
        cadence = _sample_interval(data)
        bandwidth = data.index_map["freq"]["width"][0] * 1e6
        ninput = len(data.index_map["input"])
        tel = self.telescope
        if tel is not None and nprod == getattr(tel, "nbase", -1):
            copies = np.asarray(tel.redundancy, dtype=np.float64)
        elif 2 * nprod == ninput * (ninput + 1):
            copies = np.ones(nprod)
        else:
            raise ValueError("Unexpected number of products")
        return int(self.ndays * cadence * bandwidth) * copies

    def process(self, data):
        """Add the noise to ``data`` in place and/or set its weights to ``1 / sigma^2`` (``noise.py:219-284``)."""
        data.redistribute("freq")
        pairs = _prodstack(data)
        sigma = self.recv_temp / np.sqrt(self._samples_per_product(data, len(pairs)))  # [nprod]

        if self.add_noise:
            vis = data.vis[:]
            nfreq, nprod, ntime = vis.shape
            # one draw for the whole stream, standard deviation per product (the reference's single call, :261-265)
            draw = random.complex_normal(size=(nfreq, nprod, ntime), scale=sigma[None, :, None], rng=self.rng)
            is_auto = np.asarray(pairs["input_a"]) == np.asarray(pairs["input_b"])
            # an auto-correlation is real: all of sigma^2 goes into its real part (sqrt(2) x the real half, :270-273)
            draw[:, is_auto] = np.sqrt(2) * draw[:, is_auto].real
            np.add(vis, draw, out=vis, casting="same_kind")  # summed in float64, rounded once to the stream's dtype
            data.vis[:] = vis
        if self.set_weights:
            data.weight[:] = np.broadcast_to((1.0 / sigma**2)[None, :, None], data.weight.shape)
        return data


def _sample_interval(data):
    """Seconds between samples: 240 s of sidereal time per degree of RA for a sidereal stream, else the time step."""
    if isinstance(data, containers.SiderealStream):
        return 240 * (data.ra[1] - data.ra[0]) * STELLAR_S
    return data.time[1] - data.time[0]


class SampleNoise(_RandomTask):
    """Draw complex-Wishart distributed samples around the expected visibilities (``noise.py:287-374``).

    The input must be the full triangle of products.

    Attributes
    ----------
    sample_frac : float
        Multiplies the number of samples in each measurement.
    set_weights : bool
        Set the weights to the appropriate values.
    """

    sample_frac = 1.0
    set_weights = True
    _config_names = ("sample_frac", "set_weights")

    def process(self, data_exp):
        data_exp.redistribute("freq")
        nfeed = len(data_exp.index_map["input"])
        vis_data = data_exp.vis[:]
        weight = data_exp.weight[:]
        if vis_data.shape[1] != nfeed * (nfeed + 1) // 2:
            raise ValueError("SampleNoise needs the full triangle of products")
        dt = _sample_interval(data_exp)
        iu = np.triu_indices(nfeed)
        diag = np.array([_cmap(i, i, nfeed) for i in range(nfeed)])
        pa, pb = iu
        for fi in range(vis_data.shape[0]):
            df = data_exp.index_map["freq"]["width"][fi] * 1e6
            nsamp = int(self.sample_frac * dt * df)
            for ti in range(vis_data.shape[2]):
                mat = np.zeros((nfeed, nfeed), dtype=vis_data.dtype)
                mat[iu] = vis_data[fi, :, ti]  # upper triangle in product order, noise.py:350-357
                mat = mat + np.triu(mat, 1).T.conj()
                samp = random.complex_wishart(mat, nsamp, rng=self.rng) / nsamp
                vis_data[fi, :, ti] = samp[iu]
            if self.set_weights:
                autos = vis_data[fi][diag].real  # [nfeed, ntime]
                fac = nsamp**0.5 / autos
                weight[fi] = weight[fi] * (fac[pa] * fac[pb])  # apply_gain on the weights, noise.py:366-372
        data_exp.vis[:] = vis_data
        data_exp.weight[:] = weight
        return data_exp


# the data dataset of every container here that has a data / weight pair (the reference's
# ``DataWeightContainer._data_dset_name``, ``containers.py``)
_DATA_DSET = ((containers._VisMixin, "vis"), (containers.RingMap, "map"), (containers.FormedBeam, "beam"), (containers.GridBeam, "beam"),
              (containers.FrequencyStack, "stack"), (containers.Stack3D, "stack"))


def _default_dataset(data):
    name = getattr(data, "_data_dset_name", None)
    if name is None:
        name = next((n for cls, n in _DATA_DSET if isinstance(data, cls)), None)
    if name is None:
        raise ValueError(f"No default dataset known for {type(data)} container.")
    return name


class GaussianNoiseDataset(_RandomTask):
    """Replace a dataset by Gaussian noise whose variance is the inverse of the container's weights (``noise.py:48-124``).

    Attributes
    ----------
    dataset : str
        The dataset to fill.  ``"vis"`` gets real auto-correlations (all of the variance in the real part).  Default
        (None): the data dataset of a container that has a data / weight pair.
    in_place : bool
        Work on the input (default) or on a copy.
    """

    dataset = None
    in_place = True
    _config_names = ("dataset", "in_place")

    def process(self, data):
        name = _default_dataset(data) if self.dataset is None else self.dataset
        if name not in data:
            raise CaputConfigError(f"Dataset '{name}' does not exist in container {type(data)}.")
        data.redistribute("freq")
        out = data if self.in_place else data.copy()
        dset = out[name].host()
        weight = np.asarray(data.weight[:])
        if np.iscomplexobj(dset):
            random.complex_normal(scale=tools.invert_no_zero(weight) ** 0.5, out=dset, rng=self.rng)
        else:
            self.rng.standard_normal(dtype=dset.dtype, out=dset)
            dset *= tools.invert_no_zero(weight) ** 0.5
        if name == "vis":  # an auto-correlation is real and carries the whole variance
            pairs = _prodstack(data)
            for si in np.flatnonzero(np.asarray(pairs["input_a"]) == np.asarray(pairs["input_b"])):
                dset[:, si].real *= 2**0.5
                dset[:, si].imag = 0.0
        out[name][:] = dset  # (the host copy is the valid one)
        return out


class MultipleNoiseRealizationsMixin:
    """Several realisations with the same statistics (``noise.py:127-169``): combine with a task whose ``process(data)``
    makes one.  ``setup(data1, data2=None)`` keeps the inputs; ``process()`` alternates between them and raises
    :class:`~draco_amd.core.task.PipelineStopIteration` after ``niter`` calls.

    Attributes
    ----------
    niter : int
        Number of realisations.  Default 1.
    """

    niter = 1
    in_place = False
    _config_names = ("niter",)
    _count = 0

    def setup(self, data1, data2=None):
        self.data = [data1]
        if data2 is not None:
            self.data.append(data2)
        self._count = 0

    def process(self):
        if self._count == self.niter:
            raise PipelineStopIteration
        out = super().process(self.data[self._count % len(self.data)])
        self._count += 1
        return out


class MultipleGaussianNoiseDatasets(MultipleNoiseRealizationsMixin, GaussianNoiseDataset):
    """Several Gaussian noise datasets (``noise.py:172-175``)."""


class FreqCorrelatedNoise(_RandomTask):
    """A noise realisation on the baseline grid with the frequency correlation of a ``FreqNoiseModel``
    (``noise.py:377-470``): per ``(pol, ew)`` a unit complex normal draw ``z [ra, freq, ns]`` on the host, in the
    reference's order and from the same stream, then on the device ``vis[f, ns, ra] = (L[ra] z[ra])[f, ns] / sqrt(redundancy[ns])``
    with the sums in float64, rounded once to complex64, and ``vis_weight = weight redundancy``.  The intra-cylinder
    baselines (``ew = 0``) are made Hermitian afterwards, which needs an odd number of north-south separations.  The
    draw of one slab runs on the host while the device colours the slab before it; ``vis`` and ``vis_weight`` of the
    returned ``VisGridStream`` are device resident.

    Attributes
    ----------
    save_redundancy : bool
        Save the redundancy of each visibility.  Default False.
    """

    save_redundancy = False
    _config_names = ("save_redundancy",)

    def process(self, noise_model):
        import torch

        from .. import _lib
        from ..analysis.transform import _dev_dataset
        from ..device import Context, ptr

        if "complex_freq_cov" in noise_model.datasets:
            raise NotImplementedError("FreqCorrelatedNoise: the dataset 'complex_freq_cov' is not supported (complex covariances)")
        noise_model.redistribute("ra")
        redundancy = np.ascontiguousarray(noise_model.redundancy[:], dtype=np.int32)
        npol, new, nns = redundancy.shape
        if nns % 2 == 0:
            raise ValueError(f"FreqCorrelatedNoise needs an odd number of north-south separations to make ew = 0 Hermitian, got {nns}")
        out = containers.VisGridStream(axes_from=noise_model, attrs_from=noise_model, comm=noise_model.comm, allocate=False)
        if self.save_redundancy:
            out.add_dataset("redundancy", allocate=True)
            out.redundancy[:] = redundancy[..., np.newaxis]
        ctx = Context.get()
        L = _dev_dataset(noise_model.freq_cov, ctx, np.float64).contiguous()
        weight = _dev_dataset(noise_model.weight, ctx, np.float32).contiguous()
        nfreq, nra = int(weight.shape[1]), int(weight.shape[3])
        if tuple(L.shape) != (npol, new, nra, nfreq, nfreq) or tuple(weight.shape) != (npol, nfreq, new, nra):
            raise ValueError(f"freq_cov {tuple(L.shape)} and weight {tuple(weight.shape)} do not match redundancy {redundancy.shape}")
        pol = [str(p) for p in out.index_map["pol"]]
        pconjmap = np.unique([p[1] + p[0] for p in pol], return_inverse=True)[1].astype(np.int32)
        red_d = ctx.to_device(redundancy)
        isr_d = ctx.to_device(tools.invert_no_zero(np.sqrt(redundancy)))
        pc_d = ctx.to_device(pconjmap)
        ovis = ctx.empty((npol, nfreq, new, nns, nra), np.complex64)
        oweight = ctx.empty((npol, nfreq, new, nns, nra), np.float32)
        zp = torch.empty((nra, nfreq, nns), dtype=torch.complex64, pin_memory=True)
        z = zp.numpy()
        zd = ctx.empty((nra, nfreq, nns), np.complex64)
        copied = torch.cuda.Event()
        lib = _lib.lib
        for pp in range(npol):
            for ee in range(new):
                random.complex_normal(scale=1.0, out=z, rng=self.rng)
                zd.copy_(zp, non_blocking=True)  # (behind the colouring of the slab before, which reads zd)
                copied.record()
                _lib.check(lib.dmm_noise_colour(ctx.handle, npol, nfreq, new, nns, nra, pp, ee, ptr(L), ptr(zd), ptr(weight), ptr(red_d), ptr(isr_d), ptr(ovis), ptr(oweight)))
                copied.synchronize()  # the host buffer is free for the next draw; the kernel runs on
        _lib.check(lib.dmm_noise_hermitian(ctx.handle, npol, nfreq, new, nns, nra, ptr(pc_d), ptr(ovis)))
        ctx.uses(red_d, isr_d, pc_d, zd)
        out.attach("vis", ovis)
        out.attach("vis_weight", oweight)
        return out


class MultipleFreqCorrelatedNoise(MultipleNoiseRealizationsMixin, FreqCorrelatedNoise):
    """Several realisations of frequency-correlated noise (``noise.py:473-474``)."""
