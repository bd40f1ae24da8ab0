"""Power spectrum estimation from ring-map delay cubes on the GPU.

Drop-in for the part of ``draco/analysis/powerspec.py`` that turns the delay transform of a ring map into power spectra:

* :class:`TransformJyPerBeamToKelvin`                                   ``powerspec.py:25-115``
* :class:`ConstructWienerDelayTransform`, :class:`ApplyWienerDelayTransform`   ``powerspec.py:118-458``
* :class:`SpatialTransformDelayMap`                                     ``powerspec.py:539-705``
* :class:`CrossPowerSpectrum3D`, :class:`AutoPowerSpectrum3D`           ``powerspec.py:708-834``
* :class:`CylindricalPowerSpectrum2D`                                   ``powerspec.py:837-1017``
* :class:`SphericalPowerSpectrum2Dto1D`                                 ``powerspec.py:1020-1113``
* the unit conversions, ``image_to_uv``, ``get_3D_ps``, ``get_2d_ps``, ``get_1d_ps`` and the rest of the module's
  functions                                                             ``powerspec.py:1295-2004``

Same names, config attributes, defaults, ``setup`` / ``process`` signatures and exception types.  The cube-sized stages
run in ``libdraco_amd.so`` (``csrc/powerspec.hip``) on device-resident containers: the batched 2-D transform
``dmm_uv_fft2``, the cross product ``dmm_ps3d_cross`` and the binned reduction ``dmm_ps_cyl_bin``; their outputs stay on
the device.  Everything that is a few thousand numbers (the Fourier axes, the masks, the bin map of the cylindrical
average, the spherical average) is computed on the host with the reference's own float64 expressions.  The functions
are host NumPy.

One cosmology is used throughout -- that of :func:`get_cosmo`, or of the container a task is given; the reference's
``get_fourier_modes`` hands none to ``kperp_to_u`` and ``delays_to_kpara`` and so silently uses the default there.  The
cosmology is :class:`draco_amd.util.cosmology.Cosmology` (cora [3P] is not available; its defaults are not checked
against cora's), the constants below are caput's [3P] values.

The Wiener delay transform of a filtered ring map (``csrc/wienerdelay.hip``) builds, per pixel, the operator that takes
the map from frequency to delay given the masked channels, the foreground filter already applied and the noise
covariance between frequencies (``dmm_wienerdelay_build``), and applies it with propagated weights
(``dmm_wienerdelay_apply``); the operator, the spectrum and its weight stay on the device.  The ring map's ``filter``
and ``freq_cov`` datasets are real: complex filters (off-centre stop bands) raise ``NotImplementedError`` as in
``dayenu.py``.  The tasks that put these two datasets on a ring map (``DayenuDelayFilterHybridVis(save_filter,
calculate_cov)``, ``RADependentWeights``) are not provided yet, nor is a host-resident operator or a distribution of
the elevations over processes: an operator that does not fit the device is built from ``el`` slices of the map.

Not provided: ``ReduceExcessScatter``, ``ScaleDelayTransform`` and ``SphericalPowerSpectrum3Dto1D``.
"""

from __future__ import annotations

import ctypes
import types
from functools import cache

import numpy as np

from .. import _lib
from ..core import containers, io
from ..core.task import ContainerTask
from ..device import Context, ptr
from ..util import tools
from ..util.cosmology import Cosmology
from .ringmapmaker import find_grid_indices, window_generalised_full
from .transform import _dev_dataset

# caput.astro.constants [3P]: the speed of light (m / s), the 21 cm line (MHz), the Boltzmann constant (J / K)
constants = types.SimpleNamespace(c=299792458.0, nu21=1420.40575177, k_B=1.380649e-23)

_SPATIAL_WINDOWS = ("uniform", "hann", "hanning", "hamming", "blackman", "nuttall", "blackman_nuttall", "blackman_harris", "tukey-0.5")


@cache
def get_cosmo(*args, **kwargs):
    """The default cosmology (one object per set of arguments)."""
    return Cosmology(*args, **kwargs)


def _window(x, window):
    # the reference's tools.window_generalised term by term (the Chebyshev form of draco_amd.util.tools differs from it
    # in the last bit, and the noise-equivalent bandwidths below go into ps_norm)
    return window_generalised_full(np.asarray(x, dtype=np.float64), window)


# ---- unit conversions


def f2z(freq):
    """Redshift of the 21 cm line observed at ``freq`` MHz."""
    return constants.nu21 / freq - 1


def z2f(z):
    """Frequency in MHz at which the 21 cm line of redshift ``z`` is observed."""
    return constants.nu21 / (z + 1)


def dRperp_dtheta(z, cosmo=None):
    """Transverse comoving distance per radian at redshift ``z``, h^-1 Mpc / rad."""
    cosmo = get_cosmo() if cosmo is None else cosmo
    return cosmo.comoving_distance(z)


def dRpara_df(z, cosmo=None):
    """Radial comoving distance per unit of frequency at redshift ``z``, h^-1 Mpc / Hz (Liu et al. 2014, Eq. A9)."""
    cosmo = get_cosmo() if cosmo is None else cosmo
    hz = cosmo.H(z) * (cosmo._unit_distance / 1000.0)  # km h / (Mpc s)
    return (1 + z) ** 2.0 / hz * (constants.c / 1e3) / (constants.nu21 * 1e6)


def delays_to_kpara(delay, z, cosmo=None):
    """k_parallel in h / Mpc probed by a delay in seconds (Eq. A10)."""
    return (delay * 2 * np.pi) / dRpara_df(z, cosmo=cosmo)


def kpara_to_delay(kpara, z, cosmo=None):
    """The delay in seconds that probes ``kpara`` h / Mpc."""
    return kpara * dRpara_df(z, cosmo=cosmo) / (2 * np.pi)


def u_to_kperp(u, z, cosmo=None):
    """k_perp in h / Mpc probed by a baseline of ``u`` wavelengths (Eq. A10)."""
    return 2 * np.pi * u / dRperp_dtheta(z, cosmo=cosmo)


def kperp_to_u(kperp, z, cosmo=None):
    """The baseline length in wavelengths that probes ``kperp`` h / Mpc."""
    return kperp * dRperp_dtheta(z, cosmo=cosmo) / (2 * np.pi)


def jy_per_beam_to_kelvin(freq, bl_length):
    """Conversion factor from Jy / beam to kelvin per frequency (MHz): ``1e-26 lambda^2 / (2 k_B Omega)`` with
    ``Omega`` the solid angle of a Gaussian beam of FWHM ``1.22 lambda / bl_length``."""
    jy = 1.0e-26
    wl = constants.c / (freq * 1e6)
    fwhm = np.degrees(1.22 * wl / bl_length)
    omega = (np.pi * fwhm**2) / (4 * np.log(2))
    omega_sr = omega * (np.pi / 180.0) ** 2
    return wl**2 * jy / (2 * constants.k_B * omega_sr)


def noise_equivalent_bandwidth(N, window):
    """Relative noise-equivalent bandwidth of ``window`` sampled at ``arange(N) / N``."""
    w = _window(np.arange(N) / N, window)
    return np.sum(w) ** 2 / (np.sum(w**2) * len(w))


def _transverse_steps(ra, dec, redshift, cosmo):
    res_ra = np.deg2rad(np.mean(np.diff(ra)))
    res_dec = np.deg2rad(np.mean(np.diff(dec)))
    dm = dRperp_dtheta(redshift, cosmo=cosmo)
    return dm * res_ra * np.mean(np.cos(np.deg2rad(dec))), dm * res_dec


def get_fourier_modes(ra, dec, delays, redshift, cosmo=None):
    """``(kx [nra], ky [ndec], u [nra], v [ndec], kpara [ndelay])``: the Fourier modes conjugate to RA, Dec (degrees) and
    delay (seconds) in h / Mpc, ascending through zero, and the gridded (u, v) in wavelengths."""
    cosmo = get_cosmo() if cosmo is None else cosmo
    dx, dy = _transverse_steps(ra, dec, redshift, cosmo)
    kx = 2 * np.pi * np.fft.fftshift(np.fft.fftfreq(ra.size, d=dx))
    ky = 2 * np.pi * np.fft.fftshift(np.fft.fftfreq(dec.size, d=dy))
    return kx, ky, kperp_to_u(kx, redshift, cosmo=cosmo), kperp_to_u(ky, redshift, cosmo=cosmo), delays_to_kpara(delays, redshift, cosmo=cosmo)


def _taper(ra, dec, window):
    w_ra = _window((ra - ra[0]) / (ra[-1] - ra[0]), window)
    w_dec = _window((dec - dec[0]) / (dec[-1] - dec[0]), window)
    return w_ra, w_dec


def image_to_uv(data, ra, dec, window="tukey-0.5"):
    """``(fftshift(fft2(data * taper)) / data.size, NEB_ra, NEB_dec)`` of one ``[ra, el]`` plane on the host; as in the
    reference ``data`` is tapered in place.  The device form of this is ``dmm_uv_fft2``."""
    norm = 1 / float(np.prod(np.array(data.shape)))
    neb_ra = neb_dec = 1.0
    if window:
        w_ra, w_dec = _taper(ra, dec, window)
        neb_ra = noise_equivalent_bandwidth(ra.size, window)
        neb_dec = noise_equivalent_bandwidth(dec.size, window)
        data *= np.outer(w_ra[:, np.newaxis], w_dec[np.newaxis, :])
    return np.fft.fftshift(np.fft.fft2(data)) * norm, neb_ra, neb_dec


def vol_normalization(ra, dec, freq, redshift, cosmo=None):
    """Comoving volume of the cube in h^-3 Mpc^3."""
    cosmo = get_cosmo() if cosmo is None else cosmo
    dx, dy = _transverse_steps(ra, dec, redshift, cosmo)
    lx = ra.size * dx
    ly = dec.size * dy
    chan_width = np.abs(np.diff(freq)).mean() * 1e6
    lz = dRpara_df(redshift, cosmo=cosmo) * chan_width * freq.size
    return lx * ly * lz


def spatial_mask(k_x, k_y, ew_min, ew_max, ns_bl, wl_min, wl_max, redshift, cosmo=None):
    """``[u, v]`` bool: the modes the east-west baselines ``ew_min ... ew_max`` and the north-south baselines up to
    ``ns_bl`` (metres) measure anywhere in the band of wavelengths ``wl_min ... wl_max``."""
    cosmo = get_cosmo() if cosmo is None else cosmo
    vy_min = -ns_bl / wl_max
    kx_min = u_to_kperp(ew_min / wl_max, redshift, cosmo=cosmo)
    kx_max = u_to_kperp(ew_max / wl_min, redshift, cosmo=cosmo)
    ky_min = u_to_kperp(vy_min, redshift, cosmo=cosmo)
    ky_max = u_to_kperp(abs(vy_min), redshift, cosmo=cosmo)
    zone_x = ((k_x >= kx_min) & (k_x <= kx_max)) | ((k_x >= -kx_max) & (k_x <= -kx_min))
    zone_y = ((k_y >= ky_min) & (k_y <= ky_max)) | ((k_y >= -ky_max) & (k_y <= -ky_min))
    return zone_x[:, None] * zone_y[None, :]


def get_3D_ps(data_cube_1, data_cube_2, vol_norm_factor):
    """Real part of the cross spectrum of two cubes (the auto spectrum of the first if the second is None) times
    ``vol_norm_factor``."""
    if data_cube_1 is None and data_cube_2 is None:
        raise NameError("Atleast one data cube must be provided")
    second = data_cube_1 if data_cube_2 is None else data_cube_2
    return (data_cube_1 * np.conj(second)).real * vol_norm_factor


def _baseline_grid(u, v):
    g_uu, g_vv = np.meshgrid(v, u)
    return g_uu, g_vv, np.sqrt(g_uu**2 + g_vv**2)


def reshape_data_cube(data_cube, u, v, bl_min, bl_max):
    """``(cells, uu, vv)``: the cells of a ``[u, v]`` plane whose baseline length lies in ``[bl_min, bl_max]``
    wavelengths, flattened, with their coordinates."""
    g_uu, g_vv, g_ru = _baseline_grid(u, v)
    keep = (g_ru >= bl_min) & (g_ru <= bl_max)
    return data_cube[keep], g_uu[keep], g_vv[keep]


def _kperp_bin_index(uu, vv, kperp_bins, redshift, cosmo):
    ku = u_to_kperp(uu, redshift, cosmo=cosmo)
    kv = u_to_kperp(vv, redshift, cosmo=cosmo)
    return np.digitize(np.sqrt(ku**2 + kv**2), bins=kperp_bins)


def get_2d_ps(ps_cube, weight, kperp_bins, uu, vv, redshift, cosmo=None):
    """``(sum w p / sum w, sum w, (sum w)^2 / sum w^2)`` per k_perp bin of the flattened cells (host NumPy)."""
    cosmo = get_cosmo() if cosmo is None else cosmo
    idx = _kperp_bin_index(uu, vv, kperp_bins, redshift, cosmo)
    ps, wsum, neff = [], [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(1, len(kperp_bins)):
            w = weight[idx == i]
            ps.append(np.sum(w * ps_cube[idx == i]) / np.sum(w))
            wsum.append(np.sum(w))
            neff.append(np.sum(w) ** 2 / np.sum(w**2))
    return np.array(ps), np.array(wsum), np.array(neff)


def cyl_bin_map(u, v, uv_mask, bl_min, bl_max, kperp_bins, redshift, cosmo=None):
    """``[u, v]`` int16: the k_perp bin (0 based) every cell of a plane falls into in the cylindrical average, -1 for
    a cell that :func:`reshape_data_cube`, ``uv_mask`` or the range of ``kperp_bins`` excludes.  The same float64
    expressions as the reference, element by element, so membership is the reference's bit for bit."""
    cosmo = get_cosmo() if cosmo is None else cosmo
    if len(kperp_bins) - 1 > _lib.DMM_PS_MAX_BINS:
        raise ValueError(f"{len(kperp_bins) - 1} bins, at most {_lib.DMM_PS_MAX_BINS}")
    g_uu, g_vv, g_ru = _baseline_grid(u, v)
    keep = (g_ru >= bl_min) & (g_ru <= bl_max) & np.asarray(uv_mask, dtype=bool)
    idx = _kperp_bin_index(g_uu, g_vv, kperp_bins, redshift, cosmo)
    keep &= (idx >= 1) & (idx <= len(kperp_bins) - 1)
    return np.where(keep, idx - 1, -1).astype(np.int16)


def get_1d_ps(ps_2D, kperp, kpara, weight_cube, signal_window=None, kbins=None, Nbins_3D=10, logbins_3D=True):
    """Spherical average of a ``[kpara, kperp]`` spectrum: ``(k, spectrum, sample error, variance, neff)`` per bin.
    ``kbins`` (the edges) overrides ``Nbins_3D`` and ``logbins_3D``; a cell at the last edge (``k.max()`` with the
    default edges) lies outside the last bin."""
    kpp, kll = np.meshgrid(kperp, kpara)
    k = np.sqrt(kpp**2 + kll**2)
    w = weight_cube
    if signal_window is not None:
        k, ps_2D, w = k[signal_window], ps_2D[signal_window], weight_cube[signal_window]
    if kbins is None:
        kmin, kmax = k[k > 0].min(), k.max()
        kbins = np.logspace(np.log10(kmin), np.log10(kmax), Nbins_3D) if logbins_3D else np.linspace(kmin, kmax, Nbins_3D)
    p1d, w1d, k1d = ps_2D.flatten(), w.flatten(), k.flatten()
    idx = np.digitize(k1d, kbins)
    out = [[] for _ in range(5)]
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(1, len(kbins)):
            wb = w1d[idx == i]
            p = np.sum(wb * p1d[idx == i]) / np.sum(wb)
            out[0].append(np.average(k1d[idx == i], weights=wb))
            out[1].append(p)
            out[2].append(np.sqrt(np.sum(wb**2 * np.abs(p) ** 2) / np.sum(wb) ** 2))
            out[3].append(1 / np.sum(wb))
            out[4].append(np.sum(wb) ** 2 / np.sum(wb**2))
    return tuple(np.array(o) for o in out)


# ---- tasks


class TransformJyPerBeamToKelvin(ContainerTask):
    """Convert a ring map from Jy / beam to kelvin (``powerspec.py:25-115``): per frequency the map is multiplied by
    :func:`jy_per_beam_to_kelvin` of the longest baseline within ``ncyl`` cylinder separations, the weight by the
    inverse square of it.  One elementwise scale on the device.

    in_place : bool
        Modify and return the input container.  Default True.
    ncyl : int
        Cylinder separations included in the longest baseline; 0: intra-cylinder baselines only.  Default 3.
    """

    _config_names = ("in_place", "ncyl")
    in_place = True
    ncyl = 3

    def setup(self, telescope):
        self.telescope = io.get_telescope(telescope)
        self.bl_max = self._get_max_baseline()

    def _get_max_baseline(self):
        prod = self.telescope.prodstack
        pos = np.asarray(self.telescope.feedpositions)
        baselines = pos[np.asarray(prod["input_a"]).astype(int), :] - pos[np.asarray(prod["input_b"]).astype(int), :]
        xind = find_grid_indices(baselines)[0]
        return np.sqrt(np.sum(baselines[xind <= self.ncyl] ** 2, axis=-1)).max()

    def process(self, rm):
        rm.redistribute("freq")
        if not isinstance(rm, containers.RingMap):
            raise ValueError(f"Input container must be instance of RingMap (received {rm.__class__})")
        ctx = Context.get()
        factor = jy_per_beam_to_kelvin(np.asarray(rm.freq), self.bl_max)
        f_d = ctx.to_device(np.ascontiguousarray(factor, dtype=np.float64))
        g_d = ctx.to_device(np.ascontiguousarray(tools.invert_no_zero(factor) ** 2, dtype=np.float64))
        m = _dev_dataset(rm.map, ctx, np.float64)
        w = _dev_dataset(rm.weight, ctx, np.float64)
        if self.in_place:
            out = rm
            m.mul_(f_d[None, None, :, None, None])
            w.mul_(g_d[None, :, None, None])
        else:
            out = rm.copy(shared=tuple(rm.datasets))  # (its own dataset table; the two entries are replaced below)
            m = m * f_d[None, None, :, None, None]
            w = w * g_d[None, :, None, None]
        for name, t in (("map", m), ("weight", w)):
            ds = containers.Dataset(dev=t, attrs=dict(rm.datasets[name].attrs))
            out.datasets[name] = ds
        ctx.uses(f_d, g_d)
        return out


_LOS_WINDOWS = ("uniform", "hann", "hanning", "hamming", "blackman", "nuttall", "blackman_nuttall", "blackman_harris", "tukey-0.5", "None")


def _free_device_bytes(ctx):
    """Device memory a new tensor can take: what the driver reports free and what torch's allocator holds unused."""
    import torch

    free, _ = torch.cuda.mem_get_info(ctx.device)
    return int(free) + int(torch.cuda.memory_reserved(ctx.device)) - int(torch.cuda.memory_allocated(ctx.device))


class ConstructWienerDelayTransform(ContainerTask):
    """Construct the Wiener filter that takes a filtered ring map from frequency to delay (``powerspec.py:118-369``).

    Per pixel, with ``K`` the foreground filter and ``C`` the noise covariance of its RA, ``w`` the weights, ``b`` the
    root of the dirty beam power, ``F`` the Fourier matrix from delay to frequency and ``S`` the prior:
    ``D = diag(S) F^H H^T (H (F S F^H o b b^T) H^T + C o r r^T)^-1 window``, ``H = diag(M) K``, ``M`` the channels
    inside the window with a weight, ``r = sqrt(inv0(w diag C))`` inside the window; the inverse is that of the block
    of the channels of ``M``.  ``tau``, ``F``, ``S``, ``F S F^H`` and the window are formed once on the host as the
    reference forms them; everything per pixel runs on the device in float64, slab by slab, and the output's ``filter``
    (complex64) stays there.

    prior_amp : float
        Amplitude of the signal prior in delay space.  Default 2.8e-5.
    prior_scale : float
        Inverse coherence scale in MHz of the exponential decay of the prior with delay; 0: constant.  Default 0.
    window : str
        Apodisation along frequency, a window of ``tools.window_generalised``.  Default 'uniform'.
    window_lower_freq, window_upper_freq : float, optional
        The band in MHz the window spans (default: that of the data); channels outside weigh zero.
    workspace_mib : int
        Library scratch the pixels of one slab may take.  Default 1024.  The result does not depend on it.

    ``1 <= nfreq <= 1024``.  A pixel without a valid channel gets a zero operator; one whose covariance is not positive
    definite raises ``numpy.linalg.LinAlgError``, as the reference's ``cho_factor`` does.  An operator larger than the
    free device memory raises ``ValueError`` before anything is launched: build it from ``el`` slices of the map.
    """

    _config_names = ("prior_amp", "prior_scale", "window", "window_lower_freq", "window_upper_freq", "workspace_mib")
    prior_amp = 2.8e-5
    prior_scale = 0.0
    window = "uniform"
    window_lower_freq = None
    window_upper_freq = None
    workspace_mib = 1024

    def read_config(self, params):
        super().read_config(params)
        if self.window not in _LOS_WINDOWS:
            raise ValueError(f"window must be one of {_LOS_WINDOWS}, not {self.window!r}")
        for k in ("window_lower_freq", "window_upper_freq"):
            if getattr(self, k) is not None:
                setattr(self, k, float(getattr(self, k)))
        if self.workspace_mib < 1:
            raise ValueError(f"workspace_mib must be at least 1, not {self.workspace_mib}")

    def _get_prior(self, delay):
        """``prior_amp exp(-2 pi prior_scale |delay|)``, delay in micro-seconds."""
        return self.prior_amp * np.exp(-2.0 * np.pi * self.prior_scale * np.abs(delay))

    def _get_window(self, freq):
        """The window at the frequencies ``freq`` (MHz)."""
        frng = np.percentile(freq, [0, 100])
        if self.window_lower_freq is not None:
            frng[0] = self.window_lower_freq
        if self.window_upper_freq is not None:
            frng[1] = self.window_upper_freq
        self.log.info(f"Applying a {self.window} window spanning {frng[0]:0.2f} - {frng[1]:0.2f} MHz.")
        x = (freq - frng[0]) / (frng[1] - frng[0])
        return _window(x, self.window)

    def _constants(self, freq):
        """``(tau, F [freq, delay], Sdiag, F S F^H, window)`` as the reference forms them."""
        dfreq = np.median(np.abs(np.diff(freq)))
        window = self._get_window(freq)
        win_mask = window > 0
        ntau = np.sum(win_mask, dtype=int)
        tau = np.fft.fftshift(np.fft.fftfreq(ntau, d=dfreq))
        tau = tau[tau >= 0.0]
        F = np.exp(2.0j * np.pi * np.outer(freq, tau)) / np.sqrt(ntau)
        FT = F.T.conj()
        Sdiag = self._get_prior(tau)
        FSFT = (F * Sdiag[np.newaxis, :]) @ FT
        return tau, F, Sdiag, FSFT, window

    def _build(self, data, dtype=np.complex64):
        """``(tau, operator)``: the device tensor ``[pol, ra, el, delay, freq]`` of ``dtype`` (complex64 or complex128:
        one computation, cast at the store)."""
        for name in ("complex_filter", "complex_freq_cov"):
            if name in data.datasets:
                raise NotImplementedError(f"{type(self).__name__}: the ring map carries {name!r}; complex filters are not supported")
        npol, nfreq, nra, nel = (int(n) for n in data.weight.shape)
        if not 1 <= nfreq <= _lib.DMM_WD_MAX_FREQ:
            raise ValueError(f"{type(self).__name__}: {nfreq} frequencies; the transform takes 1 to {_lib.DMM_WD_MAX_FREQ}")
        freq = np.asarray(data.freq, dtype=np.float64)
        tau, F, Sdiag, FSFT, window = self._constants(freq)
        ndelay = int(tau.size)
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)):
            raise ValueError(f"{type(self).__name__}: the operator is complex64 or complex128, not {dtype}")
        ctx = Context.get()
        size = npol * nra * nel * ndelay * nfreq * dtype.itemsize
        free = _free_device_bytes(ctx)
        if size > free:
            raise ValueError(f"{type(self).__name__}: the operator [{npol}, {nra}, {nel}, {ndelay}, {nfreq}] takes {size / 2**30:.2f} GiB, the device has {free / 2**30:.2f} GiB free: "
                             "pass an el slice of the ring map (nothing couples elevations)")
        prior_d = ctx.to_device(np.ascontiguousarray(np.hstack([FSFT.real, FSFT.imag]), dtype=np.float64))
        four_d = ctx.to_device(np.ascontiguousarray(np.stack([F.real, F.imag]), dtype=np.float64))
        s_d = ctx.to_device(np.ascontiguousarray(Sdiag, dtype=np.float64))
        win_d = ctx.to_device(np.ascontiguousarray(window, dtype=np.float64))
        K = _dev_dataset(data.filter, ctx, np.float64).contiguous()
        Cv = _dev_dataset(data.freq_cov, ctx, np.float64).contiguous()
        w = _dev_dataset(data.weight, ctx, np.float64).contiguous()
        beam = _dev_dataset(data.dirty_beam_power, ctx, np.float64).contiguous()[0]
        for name, t, shape in (("filter", K, (npol, nfreq, nfreq, nra)), ("freq_cov", Cv, (npol, nfreq, nfreq, nra)), ("dirty_beam_power", beam, (npol, nfreq, nel))):
            if tuple(t.shape) != shape:
                raise ValueError(f"{type(self).__name__}: {name} is {tuple(t.shape)}, the weights need {shape}")
        out = ctx.empty((npol, nra, nel, ndelay, nfreq), dtype)
        bad = ctypes.c_int64(-1)
        _lib.check(_lib.lib.dmm_wienerdelay_build(ctx.handle, npol, nfreq, nra, nel, ndelay, ptr(K), ptr(Cv), ptr(w), ptr(beam), ptr(prior_d), ptr(four_d), ptr(s_d), ptr(win_d), ptr(out),
                                                  _lib.DMM_C64 if dtype == np.dtype(np.complex64) else _lib.DMM_C128, int(self.workspace_mib), ctypes.byref(bad)))
        ctx.uses(K, Cv, w, beam, prior_d, four_d, s_d, win_d)
        if bad.value >= 0:
            pp, rr, ee = np.unravel_index(bad.value, (npol, nra, nel))
            raise np.linalg.LinAlgError(f"{type(self).__name__}: the covariance of pixel (pol, ra, el) = ({pp}, {rr}, {ee}) is not positive definite")
        return tau, out

    def process(self, data):
        data.redistribute("el")
        tau, op = self._build(data, np.complex64)
        out = containers.DelayTransformOperator(delay=tau, axes_from=data, attrs_from=data, allocate=False)
        out.redistribute("el")
        for attr in ["window", "window_lower_freq", "window_upper_freq"]:
            out.attrs[attr] = getattr(self, attr)
        out.attach("filter", op)
        return out


class ApplyWienerDelayTransform(ContainerTask):
    """Apply the operator of :class:`ConstructWienerDelayTransform` to a ring map (``powerspec.py:372-458``): per pixel
    ``spectrum = D map`` (complex128) and ``weight = inv0(|D|^2 inv0(w))`` (float32), into a ``DelayTransform`` with
    ``baseline = (pol, el)`` and ``sample = ra`` whose datasets stay on the device.  The operator is read once."""

    def process(self, data, operator):
        data.redistribute("ra")
        operator.redistribute("ra")
        npol, nfreq, nra, nel = (int(n) for n in data.weight.shape)
        delay = operator.index_map["delay"]
        ndelay = int(len(delay))
        out = containers.DelayTransform(baseline=npol * nel, sample=data.index_map["ra"], delay=delay, attrs_from=data, allocate=False)
        out.add_dataset("weight", allocate=False)
        out.redistribute("sample")
        bl_axes = np.array(["pol", "el"])
        for ax in bl_axes:
            out.create_index_map(ax, data.index_map[ax])
        out.attrs["baseline_axes"] = bl_axes
        out.attrs["freq"] = data.freq
        for attr in ["window", "window_lower_freq", "window_upper_freq"]:
            out.attrs[attr.replace("window", "window_los")] = operator.attrs[attr]

        ctx = Context.get()
        op = operator.filter.device(ctx).contiguous()
        if tuple(op.shape) != (npol, nra, nel, ndelay, nfreq):
            raise ValueError(f"{type(self).__name__}: the operator is {tuple(op.shape)}, the map needs {(npol, nra, nel, ndelay, nfreq)}")
        if operator.filter.dtype not in (np.dtype(np.complex64), np.dtype(np.complex128)):
            raise ValueError(f"{type(self).__name__}: the operator is {operator.filter.dtype}, not complex64 or complex128")
        m = _dev_dataset(data.map, ctx, np.float64).contiguous()[0]
        w = _dev_dataset(data.weight, ctx, np.float64).contiguous()
        spec = ctx.empty((npol * nel, nra, ndelay), np.complex128)
        sweight = ctx.empty((npol * nel, nra, ndelay), np.float32)
        _lib.check(_lib.lib.dmm_wienerdelay_apply(ctx.handle, npol, nfreq, nra, nel, ndelay, ptr(op), _lib.DMM_C64 if operator.filter.dtype == np.dtype(np.complex64) else _lib.DMM_C128,
                                                  ptr(m), ptr(w), ptr(spec), ptr(sweight)))
        ctx.uses(op, m, w)
        out.attach("spectrum", spec)
        out.attach("weight", sweight)
        return out


class SpatialTransformDelayMap(ContainerTask):
    """Transform a delay map from (RA, Dec) to the (u, v) domain (``powerspec.py:539-705``): per (pol, delay) plane the
    2-D FFT over (RA, el) of the tapered map, shifted and normalised by the number of pixels, into a
    :class:`~draco_amd.core.containers.SpatialDelayCube` whose ``vis`` stays on the device.

    apply_spatial_window : bool
        Taper the RA and Dec axes before the transform.  Default True.
    spatial_window : str
        A window of :func:`draco_amd.util.tools.window_generalised`.  Default 'tukey-0.5'.
    ew_min, ew_max, ns_bl : float
        Shortest and longest east-west baseline and the longest north-south baseline in metres: the extent of
        ``uv_mask``.  Defaults 14, 76, 60.
    workspace_mib : int
        The transform runs in slabs of delays of about this much of the output, so that its second pass reads what
        the first wrote from the last-level cache.  Default 128.

    The input is a ``DelayTransform`` of a ring map with ``sample_axis="ra"``: ``baseline_axes`` are ``[pol, el]``,
    or those with a ``beam`` axis, of which beam 0 is taken.  An axis longer than the in-LDS transform takes (powers
    of two to 8192, other lengths to 4096) raises ``NotImplementedError``.  The input is not modified.
    """

    _config_names = ("apply_spatial_window", "spatial_window", "ew_min", "ew_max", "ns_bl", "workspace_mib")
    apply_spatial_window = True
    spatial_window = "tukey-0.5"
    ew_min = 14.0
    ew_max = 76.0
    ns_bl = 60.0
    workspace_mib = 128

    def read_config(self, params):
        super().read_config(params)
        if self.spatial_window not in _SPATIAL_WINDOWS:
            raise ValueError(f"spatial_window must be one of {_SPATIAL_WINDOWS}, not {self.spatial_window!r}")

    def setup(self, telescope):
        self.tel = io.get_telescope(telescope)
        self.cosmology = get_cosmo()

    def process(self, ds):
        if not isinstance(ds, containers.DelayTransform):
            raise ValueError(f"Input container must be instance of DelayTransform (received {ds.__class__})")
        ds.redistribute("delay")
        delay = ds.index_map["delay"]  # micro-seconds
        el = ds.index_map["el"]
        pol = ds.index_map["pol"]
        ra = ds.index_map["sample"]  # degrees
        dec = self.tel.latitude + np.degrees(np.arcsin(el))
        freq = np.asarray(ds.attrs["freq"])
        wl = constants.c / (freq * 1e6)
        axes = list(ds.attrs["baseline_axes"])
        if [ax for ax in axes if ax != "beam"] != ["pol", "el"]:
            raise ValueError(f"{type(self).__name__}: the baseline axes {axes} are not [pol, el] (with or without beam)")
        nra, nel, npol, ndelay = ra.size, el.size, pol.size, delay.size
        for name, n in (("ra", nra), ("el", nel)):
            if not _lib.lib.dmm_uv_fft2_supported(int(n)):
                raise NotImplementedError(f"{type(self).__name__}: the {name} axis has length {n}; the transform takes powers of two up to 8192 and other lengths up to 4096")

        nu_c = freq[int(freq.size / 2.0)]
        redshift = constants.nu21 / nu_c - 1
        cosmo = self.cosmology
        kx, ky, u, v, kpara = get_fourier_modes(ra, dec, delay * 1e-6, redshift, cosmo)
        uv_mask = spatial_mask(kx, ky, self.ew_min, self.ew_max, self.ns_bl, wl.min(), wl.max(), redshift, cosmo)
        out = containers.SpatialDelayCube(u=u, v=v, attrs_from=ds, axes_from=ds, cosmology=cosmo, allocate=False)
        out.set_host("kx", kx)
        out.set_host("ky", ky)
        out.set_host("uv_mask", uv_mask)
        out.set_host("kpara", kpara)
        out.attrs["freq_center"] = nu_c
        out.attrs["redshift"] = redshift
        out.attrs["volume"] = vol_normalization(ra, dec, freq, redshift, cosmo)
        window = self.spatial_window if self.apply_spatial_window else None
        out.attrs["window_spatial"] = window if window else "None"
        out.attrs["effective_ra"] = noise_equivalent_bandwidth(nra, window) if window else 1.0
        out.attrs["effective_dec"] = noise_equivalent_bandwidth(nel, window) if window else 1.0

        ctx = Context.get()
        spec = _dev_dataset(ds.spectrum, ctx, np.complex128)
        shp = tuple(len(ds.index_map[ax]) for ax in axes)
        cube = spec.reshape(*shp, nra, ndelay)
        if "beam" in axes:
            cube = cube.select(axes.index("beam"), 0)
        cube = cube.contiguous()  # [pol, el, ra, delay]: a view of the dataset itself when beam comes first
        w_ra = w_el = None
        if window:
            w_ra, w_el = (ctx.to_device(np.ascontiguousarray(w, dtype=np.float64)) for w in _taper(ra, dec, window))
        vis = ctx.empty((npol, ndelay, nra, nel), np.complex128)
        _lib.check(_lib.lib.dmm_uv_fft2(ctx.handle, ptr(cube), int(npol), int(nel), int(nra), int(ndelay), ptr(w_ra) if window else None, ptr(w_el) if window else None, ptr(vis),
                                        int(self.workspace_mib)))
        ctx.uses(spec, cube, *([w_ra, w_el] if window else []))
        out.attach("vis", vis)
        return out


class CrossPowerSpectrum3D(ContainerTask):
    """The 3-D cross power spectrum of two :class:`~draco_amd.core.containers.SpatialDelayCube` s
    (``powerspec.py:708-815``): ``spectrum[p1-p2] = ps_norm vis_1[p1] conj(vis_2[p2])`` for every pair of polarisations,
    ``ps_norm`` the volume of the cube over the noise-equivalent bandwidths of the three tapers, K^2 h^-3 Mpc^3.  As in
    the reference ``vis_1.attrs["effective_bandwidth"]`` is set when both cubes carry a line-of-sight window."""

    def process(self, vis_1, vis_2):
        if vis_1.vis.shape != vis_2.vis.shape:
            raise ValueError(f"Size of data_1 ({vis_1.vis.shape}) must match data_2 ({vis_2.vis.shape})")
        if type(vis_1) is not type(vis_2):
            raise TypeError(f"type(vis_1) (={type(vis_1)}) must match type(vis_2) (={type(vis_2)})")
        vis_1.redistribute("delay")
        vis_2.redistribute("delay")
        pol_1 = list(vis_1.index_map["pol"])
        pol_2 = list(vis_2.index_map["pol"])
        pol = np.array(["-".join([p1, p2]) for p1 in pol_1 for p2 in pol_2])

        volume = vis_1.attrs["volume"]
        if vis_1.attrs["window_los"] != "None" and vis_2.attrs["window_los"] != "None":
            if vis_1.attrs["window_los"] != vis_2.attrs["window_los"]:
                raise ValueError("The windows applied to both data sets are different")
            neb_freq = noise_equivalent_bandwidth(vis_1.index_map["delay"].size, vis_1.attrs["window_los"])
            vis_1.attrs["effective_bandwidth"] = neb_freq
        else:
            neb_freq = 1
        neb = 1 / (neb_freq * vis_1.attrs["effective_ra"] * vis_1.attrs["effective_dec"])
        ps_norm = volume * neb

        out = containers.PowerSpectrum3D(pol=pol, axes_from=vis_1, attrs_from=vis_1, cosmology=vis_1.cosmology, allocate=False)
        for name in ("kx", "ky", "kpara", "uv_mask"):
            out.set_host(name, vis_1.datasets[name][:].copy())
        out.attrs["ps_norm"] = ps_norm
        if "lsd" in vis_1.attrs and "lsd" in vis_2.attrs:
            out.attrs["lsd_p0"] = vis_1.attrs["lsd"]
            out.attrs["lsd_p1"] = vis_2.attrs["lsd"]
        if "tag" in vis_1.attrs and "tag" in vis_2.attrs:
            out.attrs["tag"] = "_x_".join([vis_1.attrs["tag"], vis_2.attrs["tag"]])

        ctx = Context.get()
        v1 = _dev_dataset(vis_1.vis, ctx, np.complex128).contiguous()
        v2 = v1 if vis_2 is vis_1 else _dev_dataset(vis_2.vis, ctx, np.complex128).contiguous()
        ncell = int(np.prod(v1.shape[1:]))
        spectrum = ctx.empty((len(pol),) + tuple(v1.shape[1:]), np.complex128)
        _lib.check(_lib.lib.dmm_ps3d_cross(ctx.handle, ptr(v1), ptr(v2), len(pol_1), len(pol_2), ncell, float(ps_norm), ptr(spectrum)))
        ctx.uses(v1, v2)
        out.attach("spectrum", spectrum)
        return out


class AutoPowerSpectrum3D(CrossPowerSpectrum3D):
    """The 3-D auto power spectrum of one cube (``powerspec.py:818-834``); its imaginary part is exactly zero."""

    def process(self, data):
        return super().process(data, data)


class CylindricalPowerSpectrum2D(ContainerTask):
    """The cylindrically averaged 2-D power spectrum of a :class:`~draco_amd.core.containers.PowerSpectrum3D`
    (``powerspec.py:837-1017``): per (pol, delay) plane the weighted mean of the cells of every k_perp bin, the sum of
    the weights and the effective number of modes.  The bin of a cell is the same in every plane: it is computed once
    on the host (:func:`cyl_bin_map`), the sums run on the device in a fixed order.  An empty bin gives NaN.

    bl_min, bl_max : float
        The baseline lengths in metres between which cells are binned.  Defaults 20, 66.
    Nbins_2D : int
        The number of bin edges.  Default 35.
    logbins_2D : bool
        Logarithmic bins.  Default False.
    delay_cut : float
        ``mask`` is False below the k_parallel of this delay (seconds).  Default 300e-9.

    ``setup(weight)``: a ``PowerSpectrum3D`` of sigma; the weights are ``1 / |sigma|^2`` (0 where sigma is 0), formed on
    the fly.  Without it every cell weighs 1.
    """

    _config_names = ("bl_min", "bl_max", "Nbins_2D", "logbins_2D", "delay_cut")
    bl_min = 20.0
    bl_max = 66.0
    Nbins_2D = 35
    logbins_2D = False
    delay_cut = 300.0e-9
    weight = None

    def setup(self, weight=None):
        self.weight = weight

    def _bins(self, ps):
        redshift = ps.attrs["redshift"]
        wl = constants.c / (ps.attrs["freq_center"] * 1e6)
        u_min, u_max = self.bl_min / wl, self.bl_max / wl
        k_min = u_to_kperp(u_min, redshift, ps.cosmology)
        k_max = u_to_kperp(u_max, redshift, ps.cosmology)
        if self.logbins_2D:
            kperp = np.logspace(np.log10(k_min), np.log10(k_max), self.Nbins_2D)
        else:
            kperp = np.linspace(k_min, k_max, self.Nbins_2D)
        return u_min, u_max, kperp

    def process(self, ps):
        if not isinstance(ps, containers.PowerSpectrum3D):
            raise ValueError(f"Input container must be instance of PowerSpectrum3D (received {ps.__class__})")
        ps.redistribute("delay")
        pol = ps.index_map["pol"]
        kpara = ps.kpara[:]
        redshift = ps.attrs["redshift"]
        u_min, u_max, kperp = self._bins(ps)
        kperp_cent = 0.5 * (kperp[1:] + kperp[:-1])
        uv_dist = kperp_to_u(kperp_cent, redshift, ps.cosmology)
        binmap = np.ascontiguousarray(cyl_bin_map(ps.index_map["u"], ps.index_map["v"], ps.uv_mask[:], u_min, u_max, kperp, redshift, ps.cosmology))

        out = containers.PowerSpectrum2D(pol=pol, delay=ps.delay[:], uv_dist=uv_dist, attrs_from=ps, cosmology=ps.cosmology, allocate=False)
        out.set_host("kpara", kpara)
        out.set_host("kperp", kperp_cent)
        out.attrs["delay_cut"] = self.delay_cut

        ctx = Context.get()
        spec = _dev_dataset(ps.spectrum, ctx, np.complex128).contiguous()
        npol, ndelay, nu, nv = (int(n) for n in spec.shape)
        sigma = None
        if self.weight is not None:
            self.weight.redistribute("delay")
            sigma = _dev_dataset(self.weight.spectrum, ctx, np.complex128).contiguous()
            if tuple(sigma.shape) != tuple(spec.shape):
                raise ValueError(f"The weight cube is {tuple(sigma.shape)}, the power spectrum {tuple(spec.shape)}")
        nbins = len(kperp) - 1
        o_spec = ctx.empty((npol, ndelay, nbins), np.complex128)
        o_w = ctx.empty((npol, ndelay, nbins), np.float64)
        o_n = ctx.empty((npol, ndelay, nbins), np.float64)
        _lib.check(_lib.lib.dmm_ps_cyl_bin(ctx.handle, ptr(spec), ptr(sigma) if sigma is not None else None, binmap.ctypes.data, npol * ndelay, nu, nv, nbins, ptr(o_spec), ptr(o_w),
                                           ptr(o_n)))
        ctx.uses(spec, *([sigma] if sigma is not None else []))
        out.attach("spectrum", o_spec)
        out.attach("weight", o_w)
        out.attach("neff", o_n)

        mask = np.ones((npol, ndelay, nbins), dtype=bool)
        if self.delay_cut > 0.0:
            # (the negative k_parallel modes, conjugates of the positive ones, go too)
            mask[:, np.where(kpara < delays_to_kpara(self.delay_cut, redshift, ps.cosmology))[0], :] = False
        out.set_host("mask", mask)
        return out


class SphericalPowerSpectrum2Dto1D(ContainerTask):
    """The spherically averaged 1-D power spectrum of a :class:`~draco_amd.core.containers.PowerSpectrum2D`
    (``powerspec.py:1020-1113``), on the host: the input is a few thousand numbers.

    Nbins_3D : int
        The number of bin edges.  Default 8.
    logbins_3D : bool
        Logarithmic bins.  Default True.
    bin_edges : list of float, optional
        The bin edges; they override ``Nbins_3D`` and ``logbins_3D``.
    """

    _config_names = ("Nbins_3D", "logbins_3D", "bin_edges")
    Nbins_3D = 8
    logbins_3D = True
    bin_edges = None

    def process(self, ps2D):
        if not isinstance(ps2D, containers.PowerSpectrum2D):
            raise ValueError(f"Input container must be instance of PowerSpectrum2D (received {ps2D.__class__})")
        ps2D.redistribute("pol")
        kbins = None
        if self.bin_edges is not None:
            if self.Nbins_3D is not None:
                self.log.warning("Both 'bin_edges' and 'Nbins_3D' are specified. Using 'bin_edges' and ignoring 'Nbins_3D'.")
            self.Nbins_3D = len(self.bin_edges)
            kbins = np.array(self.bin_edges)
        pol = ps2D.index_map["pol"]
        kpara, kperp = ps2D.kpara[:], ps2D.kperp[:]
        spec, mask, weight = ps2D.spectrum[:], ps2D.mask[:], ps2D.weight[:]
        out = containers.PowerSpectrum1D(pol=pol, k=self.Nbins_3D - 1, attrs_from=ps2D, cosmology=ps2D.cosmology)
        for pp in range(len(pol)):
            k1d, p, err, var, neff = get_1d_ps(spec[pp], kperp, kpara, weight[pp], signal_window=mask[pp], kbins=kbins, Nbins_3D=self.Nbins_3D, logbins_3D=self.logbins_3D)
            out.k1D[pp], out.spectrum[pp], out.samp_var[pp], out.var[pp], out.neff[pp] = k1d, p, err, var, neff
        return out


__all__ = [
    "ApplyWienerDelayTransform",
    "AutoPowerSpectrum3D",
    "ConstructWienerDelayTransform",
    "CrossPowerSpectrum3D",
    "CylindricalPowerSpectrum2D",
    "SpatialTransformDelayMap",
    "SphericalPowerSpectrum2Dto1D",
    "TransformJyPerBeamToKelvin",
    "cyl_bin_map",
    "dRpara_df",
    "dRperp_dtheta",
    "delays_to_kpara",
    "f2z",
    "get_1d_ps",
    "get_2d_ps",
    "get_3D_ps",
    "get_cosmo",
    "get_fourier_modes",
    "image_to_uv",
    "jy_per_beam_to_kelvin",
    "kpara_to_delay",
    "kperp_to_u",
    "noise_equivalent_bandwidth",
    "reshape_data_cube",
    "spatial_mask",
    "u_to_kperp",
    "vol_normalization",
    "z2f",
]
