"""Host side of the power-spectrum chain (`draco_amd/analysis/powerspec.py`, `draco_amd/util/cosmology.py`) against
vectors produced by executing the reference (`tests/gen_golden_powerspec.py` -> tests/golden/powerspec.npz): the twin
against the stored truths, the functions against the reference's values, the cosmology's own properties, the
containers, every exception, and the host-computed bin map of the cylindrical average against the reference's
membership.  No GPU is needed: everything here stops before the first launch.
"""

import os

import numpy as np
import pytest

import powerspec_twin as twin
from conftest import GOLDEN

SPATIAL = ("A", "B", "C", "D", "E")
WINDOWS = {"A": "tukey-0.5", "B": "nuttall", "C": None, "D": "uniform", "E": "uniform"}
CYL = {
    "CYL_B": ("AUTO_B", False, dict(bl_min=20.0, bl_max=110.0, Nbins_2D=7)),
    "CYL_Bs": ("AUTO_B", True, dict(bl_min=20.0, bl_max=110.0, Nbins_2D=7)),
    "CYL_S": ("S", False, dict(bl_min=15.0, bl_max=140.0, Nbins_2D=9, logbins_2D=True, delay_cut=0.0)),
    "CYL_Ss": ("S", True, dict(bl_min=15.0, bl_max=140.0, Nbins_2D=9, logbins_2D=True, delay_cut=0.0)),
}


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "powerspec.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ps():
    from draco_amd.analysis import powerspec

    return powerspec


def cyl_input(g, name):
    """``(spectrum, sigma or None, u, v, uv_mask, redshift, freq_center, delay, pol, kx, ky, kpara)`` of a cylindrical case."""
    src, with_sigma, _ = CYL[name]
    sigma = twin.from_q64(g[f"{src}/sigma_q64"]) if with_sigma else None
    if src == "S":
        return (twin.from_q64(g["S/spectrum_q64"]), sigma, g["S/u"], g["S/v"], g["S/uv_mask"], float(g["S/redshift"]), float(g["S/freq_center"]), g["S/delay"], g["S/pol"], g["S/kx"],
                g["S/ky"], g["S/kpara_in"])
    return (g["AUTO_B/ref"], sigma, g["B/u"], g["B/v"], g["B/uv_mask"], float(g["B/attr_redshift"]), float(g["B/attr_freq_center"]), g["B/delay"], g["AUTO_B/pol"], g["B/kx"], g["B/ky"],
            g["B/kpara"])


# ---- the twin against the stored truths


@pytest.mark.parametrize("name", SPATIAL)
def test_twin_spatial(gold, name):
    g = gold
    axes = [str(a) for a in g[f"{name}/axes"]]
    spectrum = twin.from_q64(g[f"{name}/spectrum_q64"])
    shape = {"pol": len(g[f"{name}/pol"]), "el": len(g[f"{name}/el"])}
    shape["beam"] = spectrum.shape[0] // (shape["pol"] * shape["el"])
    cube = twin.spectrum_to_cube(spectrum, tuple(shape[a] for a in axes), axes)
    w_ra, w_el = (g[f"{name}/w_ra"], g[f"{name}/w_el"]) if WINDOWS[name] else (None, None)
    truth = twin.uv_full(cube, w_ra, w_el).astype(np.complex128)
    stored = twin.from_bits(g[f"{name}/ref"], g[f"{name}/truth_bits"])
    assert np.array_equal(truth, stored)
    assert twin.rel_err(g[f"{name}/ref"], truth) == float(g[f"{name}/e_ref"]) <= 4e-16
    # the sampled evaluation is the full one at those cells (another order of the long-double sums: 2^-64 a term)
    iu, iv = twin.sample_cells(cube.shape[2], cube.shape[3], 7)
    assert (cube.shape[2] // 2, cube.shape[3] // 2) in set(zip(iu.tolist(), iv.tolist())) and len(iu) == min(64, cube.shape[2] * cube.shape[3])
    assert twin.rel_err(twin.uv_at(cube, iu, iv, w_ra, w_el), twin.uv_full(cube, w_ra, w_el)[:, :, iu, iv]) <= 2.0**-58


def test_twin_cross(gold):
    g = gold
    t = twin.cross(g["D/ref"], g["E/ref"], float(g["XDE/ps_norm"])).astype(np.complex128)
    assert np.array_equal(t, twin.from_bits(g["XDE/ref"], g["XDE/truth_bits"]))
    assert twin.rel_err(g["XDE/ref"], t) == float(g["XDE/e_ref"])
    t = twin.cross(g["B/ref"], g["B/ref"], float(g["AUTO_B/ps_norm"])).astype(np.complex128)
    assert np.array_equal(t, twin.from_bits(g["AUTO_B/ref"], g["AUTO_B/truth_bits"])) and not t.imag.any()


@pytest.mark.parametrize("name", list(CYL))
def test_twin_cyl(gold, name):
    g = gold
    spec, sigma = cyl_input(g, name)[:2]
    w = None if sigma is None else twin.inverse_variance(sigma)
    nbins = len(g[f"{name}/kperp_edges"]) - 1
    t_s, t_w, t_n, count, t_a = twin.cyl_bin(spec, w, g[f"{name}/binmap"], nbins)
    assert np.array_equal(t_s, g[f"{name}/truth"], equal_nan=True) and np.array_equal(t_w, g[f"{name}/truth_weight"])
    assert np.array_equal(t_n, g[f"{name}/truth_neff"], equal_nan=True) and np.array_equal(count, g[f"{name}/count"])
    assert (count == 0).any()
    # the reference against the truth: NaN in the same places, and within the summation bound of each bin
    ref = g[f"{name}/ref"]
    assert np.array_equal(np.isnan(ref), np.isnan(t_s))
    ok = ~np.isnan(t_s)
    assert (np.abs(ref - t_s)[ok] <= (np.maximum(count - 1, 0) * 2.0**-53 * t_a + 2.0**-52 * np.abs(t_s))[ok]).all()


# ---- the functions against the reference's values


def test_unit_conversions(gold, ps):
    g = gold
    z = g["FN/z"]
    assert np.array_equal(ps.f2z(np.array([400.0, 600.0, 800.0])), g["FN/f2z"]) and np.array_equal(ps.z2f(z), g["FN/z2f"])
    assert np.array_equal([ps.dRperp_dtheta(x) for x in z], g["FN/dRperp"]) and np.array_equal([ps.dRpara_df(x) for x in z], g["FN/dRpara"])
    assert np.array_equal(ps.delays_to_kpara(np.array([-1e-7, 0.0, 3e-7]), 1.3), g["FN/kpara"])
    assert np.array_equal(ps.kpara_to_delay(np.array([0.05, 0.3]), 1.3), g["FN/delay"])
    assert np.array_equal(ps.u_to_kperp(np.array([10.0, 150.0]), 1.3), g["FN/kperp"]) and np.array_equal(ps.kperp_to_u(np.array([0.01, 0.2]), 1.3), g["FN/u"])
    neb = [ps.noise_equivalent_bandwidth(n, w) for n in (7, 64) for w in ("tukey-0.5", "nuttall", "uniform", "blackman_harris")]
    assert np.array_equal(neb, g["FN/neb"])
    assert ps.constants.c == 299792458.0 and ps.constants.nu21 == 1420.40575177 and ps.constants.k_B == 1.380649e-23
    assert ps.get_cosmo() is ps.get_cosmo()


@pytest.mark.parametrize("name", SPATIAL)
def test_spatial_host_functions(gold, ps, name):
    """get_fourier_modes, spatial_mask, vol_normalization, the windows and image_to_uv: the reference's values."""
    g = gold
    ra, el, delay, freq = (g[f"{name}/{k}"] for k in ("ra", "el", "delay", "freq"))
    dec = twin.LATITUDE + np.degrees(np.arcsin(el))
    redshift = ps.f2z(freq[int(freq.size / 2.0)])
    assert redshift == float(g[f"{name}/attr_redshift"])
    kx, ky, u, v, kpara = ps.get_fourier_modes(ra, dec, delay * 1e-6, redshift)
    for got, key in ((kx, "kx"), (ky, "ky"), (u, "u"), (v, "v"), (kpara, "kpara")):
        assert np.array_equal(got, g[f"{name}/{key}"]), key
    wl = ps.constants.c / (freq * 1e6)
    assert np.array_equal(ps.spatial_mask(kx, ky, 14.0, 76.0, 60.0, wl.min(), wl.max(), redshift), g[f"{name}/uv_mask"])
    assert ps.vol_normalization(ra, dec, freq, redshift) == float(g[f"{name}/attr_volume"])
    window = WINDOWS[name]
    if window:
        w_ra, w_el = ps._taper(ra, dec, window)
        assert np.array_equal(w_ra, g[f"{name}/w_ra"]) and np.array_equal(w_el, g[f"{name}/w_el"])
    axes = [str(a) for a in g[f"{name}/axes"]]
    spectrum = twin.from_q64(g[f"{name}/spectrum_q64"])
    shape = {"pol": len(g[f"{name}/pol"]), "el": len(el)}
    shape["beam"] = spectrum.shape[0] // (shape["pol"] * shape["el"])
    cube = twin.spectrum_to_cube(spectrum, tuple(shape[a] for a in axes), axes)
    plane = np.ascontiguousarray(cube[-1, 1])
    keep = plane.copy()
    got, neb_ra, neb_el = ps.image_to_uv(plane, ra, dec, window=window)
    assert np.array_equal(got, g[f"{name}/ref"][-1, 1])
    assert neb_ra == float(g[f"{name}/attr_effective_ra"]) and neb_el == float(g[f"{name}/attr_effective_dec"])
    assert np.array_equal(plane, keep) == (window in (None, "uniform"))  # (tapered in place, as the reference's)


def test_get_3d_ps(gold, ps):
    g = gold
    a, b = g["D/ref"], g["E/ref"]
    assert np.array_equal(ps.get_3D_ps(a[0], b[1], 2.5), (a[0] * np.conj(b[1])).real * 2.5)
    assert np.array_equal(ps.get_3D_ps(a[0], None, 2.5), (np.conj(a[0]) * a[0]).real * 2.5)
    with pytest.raises(NameError):
        ps.get_3D_ps(None, None, 1.0)


@pytest.mark.parametrize("name", list(CYL))
def test_bin_map_and_host_average(gold, ps, name):
    """The bin map is the reference's membership exactly; get_2d_ps on the host gives the reference's numbers."""
    g = gold
    spec, sigma, u, v, uv_mask, redshift, freq_center = cyl_input(g, name)[:7]
    cfg = CYL[name][2]
    task = ps.CylindricalPowerSpectrum2D(**cfg)
    holder = type("P", (), {"attrs": {"redshift": redshift, "freq_center": freq_center}, "cosmology": ps.get_cosmo()})()
    u_min, u_max, kperp = task._bins(holder)
    assert np.array_equal(kperp, g[f"{name}/kperp_edges"])
    bm = ps.cyl_bin_map(u, v, uv_mask, u_min, u_max, kperp, redshift)
    assert bm.dtype == np.int16 and np.array_equal(bm, g[f"{name}/binmap"])
    w = np.ones(spec.shape) if sigma is None else twin.inverse_variance(sigma)
    p, d = 0, spec.shape[1] - 1
    flat, uu, vv = ps.reshape_data_cube(spec[p, d], u, v, u_min, u_max)
    mflat = ps.reshape_data_cube(uv_mask, u, v, u_min, u_max)[0]
    wflat = ps.reshape_data_cube(w[p, d], u, v, u_min, u_max)[0]
    got = ps.get_2d_ps(flat[mflat], wflat[mflat], kperp, uu[mflat], vv[mflat], redshift)
    for x, key in zip(got, ("ref", "ref_weight", "ref_neff")):
        assert np.array_equal(x, g[f"{name}/{key}"][p, d], equal_nan=True), key


def _ps2d(g, ps, name, containers):
    p2 = containers.PowerSpectrum2D(pol=np.arange(g[f"{name}/ref"].shape[0]).astype(str), delay=np.arange(g[f"{name}/ref"].shape[1]), uv_dist=g[f"{name}/uv_dist"], cosmology=ps.get_cosmo())
    for key, src in (("spectrum", "ref"), ("weight", "ref_weight"), ("neff", "ref_neff"), ("mask", "ref_mask"), ("kpara", "kpara"), ("kperp", "kperp")):
        p2.datasets[key][:] = g[f"{name}/{src}"]
    return p2


@pytest.mark.parametrize("name,src,cfg", [("P1_B", "CYL_B", dict(Nbins_3D=5, logbins_3D=True)), ("P1_Bl", "CYL_B", dict(Nbins_3D=4, logbins_3D=False)), ("P1_Se", "CYL_Ss", dict(Nbins_3D=8))])
def test_spherical(gold, ps, name, src, cfg):
    from draco_amd.core import containers

    g = gold
    if name == "P1_Se":
        cfg = dict(cfg, bin_edges=[float(x) for x in g["P1_Se/bin_edges"]])
    task = ps.SphericalPowerSpectrum2Dto1D(**cfg)
    with np.errstate(divide="ignore", invalid="ignore"):
        p1 = task.process(_ps2d(g, ps, src, containers))
    assert isinstance(p1, containers.PowerSpectrum1D) and p1.spectrum.dtype == np.complex128
    for key in ("spectrum", "samp_var", "var", "neff", "k1D"):
        assert np.array_equal(p1.datasets[key][:], g[f"{name}/{key}"], equal_nan=True), key
    if name == "P1_Se":  # the edges override Nbins_3D; the cell at the last edge, k.max(), is in no bin
        assert task.Nbins_3D == 5 and len(p1.index_map["k"]) == 4
        p2 = _ps2d(g, ps, src, containers)
        k = np.sqrt(np.add.outer(p2.kpara[:] ** 2, p2.kperp[:] ** 2))
        assert k.max() == cfg["bin_edges"][-1]
        idx = np.digitize(k.flatten(), np.array(cfg["bin_edges"]))
        assert idx[np.argmax(k)] == len(cfg["bin_edges"])


def test_jy_to_kelvin_factor(gold, ps):
    g = gold
    for ncyl in (0, 1):
        assert np.array_equal(ps.jy_per_beam_to_kelvin(g["JY/freq"], float(g[f"JY/bl_max{ncyl}"])), g[f"JY/factor{ncyl}"])


# ---- the cosmology


def test_cosmology():
    from draco_amd.analysis import powerspec as ps
    from draco_amd.util.cosmology import C_LIGHT, Cosmology

    c = Cosmology()
    assert (c.H0, c.omega_b, c.omega_c, c.omega_l, c.omega_k) == (67.66, 0.04897, 0.26067, 0.69036, 0.0)
    assert Cosmology(omega_l=0.6).omega_k == pytest.approx(0.09036, abs=1e-15)
    assert c.comoving_distance(0.0) == 0.0
    z = np.linspace(0.0, 6.0, 241)
    d = c.comoving_distance(z)
    assert d.shape == z.shape and (np.diff(d) > 0).all()
    assert c.comoving_distance(1.0) == d[40]
    # d D / d z = c / H: a central difference of step h carries h^2 D''' / 6 (below 1e-8 relative here) plus rounding
    h = 1e-4
    for zz in (0.3, 1.0, 1.3672, 2.5, 5.0):
        deriv = (c.comoving_distance(zz + h) - c.comoving_distance(zz - h)) / (2 * h)
        assert deriv == pytest.approx(C_LIGHT / c.H(zz) / c._unit_distance, rel=1e-8)
    # Einstein-de Sitter has a closed form: D = 2 (c / H0) (1 - 1 / sqrt(1 + z))
    eds = Cosmology(omega_b=0.0, omega_c=1.0, omega_l=0.0)
    assert eds.comoving_distance(3.0) == pytest.approx(2 * C_LIGHT / 1e5 * 0.5, rel=1e-13)
    # H(z) * _unit_distance / 1000 is 100 E(z) km h / (Mpc s)
    assert c.H(0.0) * c._unit_distance / 1000.0 == pytest.approx(100.0, rel=1e-15)
    # the round trip of the delay conversion: one ulp
    x = np.array([-3.1e-7, 1e-9, 2.7e-7, 1.9e-6])
    back = ps.kpara_to_delay(ps.delays_to_kpara(x, 1.3), 1.3)
    assert (np.abs(back - x) <= np.spacing(np.abs(x))).all()
    with pytest.raises(TypeError):
        Cosmology(omega_k=0.1)


# ---- containers


def test_containers():
    from draco_amd.core import containers as c
    from draco_amd.util.cosmology import Cosmology

    cosmo = Cosmology()
    cube = c.SpatialDelayCube(pol=np.array(["XX", "YY"]), delay=np.arange(3.0), u=np.arange(4.0), v=np.arange(5.0), cosmology=cosmo)
    assert isinstance(cube, c.Fourier3DContainer) and isinstance(cube, c.DelayContainer) and cube.cosmology is cosmo
    assert cube.vis.shape == (2, 3, 4, 5) and cube.vis.dtype == np.complex128 and cube.vis.attrs["axis"] == ["pol", "delay", "u", "v"]
    assert cube.kx.shape == (4,) and cube.ky.shape == (5,) and cube.kpara.shape == (3,) and cube.kx.dtype == cube.kpara.dtype == np.float64
    assert cube.uv_mask.shape == (4, 5) and cube.uv_mask.dtype == np.bool_
    cube.attrs.update(redshift=1.2, freq_center=640.0)
    assert cube.redshift == 1.2 and cube.freq_center == 640.0
    p3 = c.PowerSpectrum3D(pol=np.array(["XX-XX"]), axes_from=cube, attrs_from=cube)
    assert p3.spectrum.shape == (1, 3, 4, 5) and p3.spectrum.dtype == np.complex128 and p3.cosmology is cosmo and p3.redshift == 1.2
    p3.attrs["ps_norm"] = 2.0
    assert p3.ps_norm == 2.0 and set(p3.datasets) == {"kx", "ky", "kpara", "uv_mask", "spectrum"}
    p2 = c.PowerSpectrum2D(pol=np.array(["XX-XX"]), delay=np.arange(3.0), uv_dist=np.arange(6.0), attrs_from=p3, cosmology=cosmo)
    assert {k: (d.shape, d.dtype) for k, d in p2.datasets.items()} == {
        "spectrum": ((1, 3, 6), np.complex128), "weight": ((1, 3, 6), np.float64), "neff": ((1, 3, 6), np.float64), "mask": ((1, 3, 6), np.bool_), "kpara": ((3,), np.float64),
        "kperp": ((6,), np.float64)}
    p1 = c.PowerSpectrum1D(pol=np.array(["XX-XX"]), k=7, attrs_from=p2, cosmology=cosmo)
    assert {k: (d.shape, d.dtype) for k, d in p1.datasets.items()} == {
        "spectrum": ((1, 7), np.complex128), "samp_var": ((1, 7), np.float64), "var": ((1, 7), np.float64), "neff": ((1, 7), np.float64), "k1D": ((1, 7), np.float64)}
    with pytest.raises(ValueError):
        cube.set_host("kx", np.zeros(3))


# ---- exceptions (all raised before anything touches a device)


def _cube(containers, cosmo, pol=("XX", "YY"), shape=(3, 4, 5), cls=None, **attrs):
    cube = (cls or containers.SpatialDelayCube)(pol=np.array(pol), delay=np.arange(float(shape[0])), u=np.arange(float(shape[1])), v=np.arange(float(shape[2])), cosmology=cosmo)
    cube.attrs.update(dict(volume=1.0, window_los="nuttall", effective_ra=1.0, effective_dec=1.0, tag="t"), **attrs)
    return cube


def test_exceptions(gold, ps):
    from draco_amd.core import containers

    g, cosmo = gold, ps.get_cosmo()
    tel = type("T", (), {"latitude": twin.LATITUDE, "lmax": 1, "mmax": 1, "frequencies": np.array([600.0])})()
    st = ps.SpatialTransformDelayMap()
    st.setup(tel)
    with pytest.raises(ValueError, match="instance of DelayTransform"):
        st.process(containers.DelaySpectrum(baseline=2, delay=np.arange(3.0)))
    ds = twin.golden_delay_transform(g, "D")
    ds.attrs["baseline_axes"] = ["el", "pol"]
    with pytest.raises(ValueError, match="baseline axes"):
        st.process(ds)
    for n_ra, n_el, axis, n in ((8193, 2, "ra", 8193), (4097, 2, "ra", 4097), (4, 8193, "el", 8193), (4, 4097, "el", 4097)):
        ra, el = 10.0 + 0.01 * np.arange(n_ra), np.sin(np.radians(0.001 * np.arange(n_el)))
        big = twin.delay_transform(np.zeros((n_el, n_ra, 1), dtype=np.complex128), ra, el, np.zeros(1), np.array([600.0]), ["XX"], ["pol", "el"], "None")
        with pytest.raises(NotImplementedError, match=f"{axis} axis has length {n}"):
            st.process(big)
    with pytest.raises(ValueError, match="spatial_window"):
        ps.SpatialTransformDelayMap(spatial_window="boxcar")

    x = ps.CrossPowerSpectrum3D()
    with pytest.raises(ValueError, match="must match"):
        x.process(_cube(containers, cosmo), _cube(containers, cosmo, shape=(3, 4, 6)))

    class Other(containers.SpatialDelayCube):
        pass

    with pytest.raises(TypeError, match="must match"):
        x.process(_cube(containers, cosmo), _cube(containers, cosmo, cls=Other))
    with pytest.raises(ValueError, match="windows applied to both data sets are different"):
        x.process(_cube(containers, cosmo), _cube(containers, cosmo, window_los="blackman"))

    with pytest.raises(ValueError, match="instance of PowerSpectrum3D"):
        ps.CylindricalPowerSpectrum2D().process(_cube(containers, cosmo))
    with pytest.raises(ValueError, match="instance of PowerSpectrum2D"):
        ps.SphericalPowerSpectrum2Dto1D().process(_cube(containers, cosmo))
    jy = ps.TransformJyPerBeamToKelvin()
    jy.bl_max = 20.0
    with pytest.raises(ValueError, match="instance of RingMap"):
        jy.process(_cube(containers, cosmo))
    with pytest.raises(ValueError, match="at most"):
        ps.cyl_bin_map(np.arange(3.0), np.arange(3.0), np.ones((3, 3), bool), 0.0, 5.0, np.linspace(0.1, 1.0, 4098), 1.0)


def test_jy_max_baseline(gold, ps):
    from draco_amd.core.products import TransitTelescope

    g = gold
    tel = TransitTelescope(g["JY/freq"], lmax=12, ncyl=2, nfeed_cyl=3)
    for ncyl in (0, 1):
        task = ps.TransformJyPerBeamToKelvin(ncyl=ncyl, in_place=False)
        task.setup(tel)
        assert task.bl_max == float(g[f"JY/bl_max{ncyl}"])
