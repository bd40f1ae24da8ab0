"""GPU power-spectrum chain (`csrc/powerspec.hip`, `draco_amd/analysis/powerspec.py`) against a long-double truth and
against vectors produced by executing the reference (`tests/gen_golden_powerspec.py` -> tests/golden/powerspec.npz).

Spatial transform.  Per case `e_gpu = max |gpu - truth| / max |truth|` with the truth (`tests/powerspec_twin.py`, a
direct long-double DFT) rounded once; required `e_gpu <= max(K e_ref, 2**-51)` and, against the reference's vectors,
`<= (K + 1) e_ref + 2**-51`.  `e_ref` is the same measure of the reference's own output (stored by the generator; on
the seeded cases `numpy.fft.fft2`'s, computed here).  K = 2 where both lengths are powers of two (the margin for
another rounding order, as in `test_gpu_delay.py`), K = 8 where either axis goes through Bluestein's algorithm (three
transforms of at least twice the length and two chirp products in place of one transform; the margin of the SHT
sweep).  Axes longer than 256 are checked at 64 cells per plane: the zero mode, the cells beside it and beside the
Nyquist position, the corners and seeded cells.

Cross / auto: `e_gpu <= max(2 e_ref, 2**-51)`; the imaginary part of a polarisation with itself is exactly 0.
Cylindrical average: `weight` and, with unit weights, `neff` are integer counts and equal the reference's; NaN exactly
where the reference has it; per bin `|gpu - truth| <= (n - 1) 2**-53 sum |w p|` (the any-order summation bound, n the
population of the bin; taken over `sum w` too where that is smaller); two runs agree bit for bit.  Every input
container is device resident.  Each test prints its figures before it asserts.
"""

import os

import numpy as np
import pytest

import delay_twin
import powerspec_twin as twin
from conftest import GOLDEN
from test_powerspec_host import CYL, WINDOWS, cyl_input

pytestmark = pytest.mark.gpu

FLOOR = 2.0**-51
U = 2.0**-53
TEL = type("Tel", (), {"latitude": twin.LATITUDE, "lmax": 1, "mmax": 1, "frequencies": np.array([600.0])})()
# (nra, nel, ndelay, npol): the edges of the row-FFT plan
SEEDED = [(4096, 3, 2, 1), (8192, 2, 1, 1), (2049, 4, 2, 1), (4095, 5, 1, 1), (3, 4095, 2, 1), (256, 96, 6, 2)]
SEEDED_WINDOW = "hamming"  # (not zero at the ends: an axis of two or three points keeps all its rows)


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "powerspec.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ps():
    from draco_amd.analysis import powerspec

    return powerspec


def _to_device(container, *names):
    from draco_amd.device import Context

    ctx = Context.get()
    for name in names:
        ds = container.datasets[name]
        ds.set_device(ctx.to_device(np.ascontiguousarray(ds.host())))
    return container


def _pow2(n):
    return n & (n - 1) == 0


def _margin(nra, nel):
    return 2 if _pow2(nra) and _pow2(nel) else 8


def _check(name, got, truth, ref, e_ref, K):
    e_gpu, e_tri = twin.rel_err(got, truth), twin.rel_err(got, ref)
    print(f"powerspec {name}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} ratio {e_gpu / e_ref:.2f} (to the reference {e_tri:.3e}) K {K}")
    assert np.isfinite(np.ascontiguousarray(got).view(np.float64)).all()
    assert e_gpu <= max(K * e_ref, FLOOR), (name, e_gpu, e_ref)
    assert e_tri <= (K + 1) * e_ref + FLOOR, (name, e_tri, e_ref)


# ---- the spatial transform


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_spatial_golden(gold, ps, name):
    g = gold
    from draco_amd.device import Context

    ds = _to_device(twin.golden_delay_transform(g, name, tag=name), "spectrum")
    before = ds.spectrum.device(Context.get()).clone()
    window = WINDOWS[name]
    task = ps.SpatialTransformDelayMap(apply_spatial_window=window is not None, **({"spatial_window": window} if window else {}))
    task.setup(TEL)
    out = task.process(ds)
    assert out.vis.on_device and out.vis.dtype == np.complex128
    assert bool((ds.spectrum.device(Context.get()) == before).all())  # the input is not modified
    ref = g[f"{name}/ref"]
    vis = out.vis[:]
    assert vis.shape == ref.shape
    _check(name, vis, twin.from_bits(ref, g[f"{name}/truth_bits"]), ref, float(g[f"{name}/e_ref"]), _margin(ref.shape[2], ref.shape[3]))
    for key in ("kx", "ky", "kpara", "uv_mask"):
        assert out.datasets[key].dtype == g[f"{name}/{key}"].dtype and np.array_equal(out.datasets[key][:], g[f"{name}/{key}"]), key
    for key in ("u", "v", "delay", "pol"):
        assert np.array_equal(out.index_map[key], g[f"{name}/{key}"]), key
    for key in ("freq_center", "redshift", "volume", "window_spatial", "effective_ra", "effective_dec"):
        assert out.attrs[key] == g[f"{name}/attr_{key}"].item(), key
    assert out.attrs["window_los"] == str(g[f"{name}/window_los"]) and out.attrs["tag"] == name and out.cosmology is ps.get_cosmo()


_seeded_cache = {}


def _seeded_case(ps, shape):
    """Inputs, the sampled truth and numpy's own result for one seeded case (computed once)."""
    if shape in _seeded_cache:
        return _seeded_cache[shape]
    nra, nel, ndelay, npol = shape
    rng = np.random.default_rng(nra * 7 + nel)
    ra = 10.0 + (0.2 if nra <= 256 else 0.01) * np.arange(nra)
    el = np.sin(np.radians((0.2 if nel <= 256 else 0.005) * (np.arange(nel) - nel / 2)))
    freq = 600.0 + 0.390625 * np.arange(max(ndelay, 2))
    delay = np.fft.fftshift(np.fft.fftfreq(ndelay, d=0.390625))
    pol = ["XX", "YY"][:npol]
    spectrum = rng.normal(size=(npol * nel, nra, ndelay)) + 1j * rng.normal(size=(npol * nel, nra, ndelay))
    dec = twin.LATITUDE + np.degrees(np.arcsin(el))
    w_ra, w_el = ps._taper(ra, dec, SEEDED_WINDOW)
    cube = twin.spectrum_to_cube(spectrum, (npol, nel), ["pol", "el"])
    if twin.sampled(nra, nel):
        iu, iv = twin.sample_cells(nra, nel, nra + nel)
        truth = twin.uv_at(cube, iu, iv, w_ra, w_el).astype(np.complex128)
    else:
        iu = iv = None
        truth = twin.uv_full(cube, w_ra, w_el).astype(np.complex128)
    ref = np.fft.fftshift(np.fft.fft2(cube * np.outer(w_ra, w_el)), axes=(-2, -1)) * (1 / float(nra * nel))
    case = dict(spectrum=spectrum, ra=ra, el=el, freq=freq, delay=delay, pol=pol, iu=iu, iv=iv, truth=truth, ref=ref if iu is None else ref[:, :, iu, iv])
    _seeded_cache[shape] = case
    return case


@pytest.mark.parametrize("shape", SEEDED, ids=lambda s: "x".join(str(n) for n in s))
def test_spatial_seeded(ps, shape):
    nra, nel, ndelay, npol = shape
    c = _seeded_case(ps, shape)
    ds = _to_device(twin.delay_transform(c["spectrum"], c["ra"], c["el"], c["delay"], c["freq"], c["pol"], ["pol", "el"], "nuttall"), "spectrum")
    task = ps.SpatialTransformDelayMap(spatial_window=SEEDED_WINDOW)
    task.setup(TEL)
    out = task.process(ds)
    assert np.array_equal(ds.spectrum[:], c["spectrum"])
    vis = out.vis[:]
    assert vis.shape == (npol, ndelay, nra, nel) and np.isfinite(vis.view(np.float64)).all()
    got = vis if c["iu"] is None else vis[:, :, c["iu"], c["iv"]]
    _check("x".join(str(n) for n in shape), got, c["truth"], c["ref"], twin.rel_err(c["ref"], c["truth"]), _margin(nra, nel))
    # a second run, in the smallest slabs of delays: the same bits
    task2 = ps.SpatialTransformDelayMap(spatial_window=SEEDED_WINDOW, workspace_mib=1)
    task2.setup(TEL)
    assert np.array_equal(task2.process(ds).vis[:], vis)


@pytest.mark.parametrize("nra,nel,axis,n", [(8193, 2, "ra", 8193), (4097, 3, "ra", 4097), (4, 8193, "el", 8193), (5, 4097, "el", 4097)])
def test_unsupported_lengths(ps, nra, nel, axis, n):
    ra, el = 10.0 + 0.01 * np.arange(nra), np.sin(np.radians(0.001 * np.arange(nel)))
    ds = _to_device(twin.delay_transform(np.zeros((nel, nra, 1), dtype=np.complex128), ra, el, np.zeros(1), np.array([600.0, 600.4]), ["XX"], ["pol", "el"], "None"), "spectrum")
    task = ps.SpatialTransformDelayMap()
    task.setup(TEL)
    with pytest.raises(NotImplementedError, match=f"{axis} axis has length {n}"):
        task.process(ds)


# ---- cross and auto spectra


def _cube(g, ps, name, **attrs):
    from draco_amd.core import containers

    cube = containers.SpatialDelayCube(pol=g[f"{name}/pol"], delay=g[f"{name}/delay"], u=g[f"{name}/u"], v=g[f"{name}/v"], cosmology=ps.get_cosmo())
    for key in ("kx", "ky", "kpara", "uv_mask"):
        cube.datasets[key][:] = g[f"{name}/{key}"]
    cube.vis[:] = g[f"{name}/ref"]
    cube.attrs.update({k: g[f"{name}/attr_{k}"].item() for k in ("freq_center", "redshift", "volume", "window_spatial", "effective_ra", "effective_dec")})
    cube.attrs.update(window_los=str(g[f"{name}/window_los"]), **attrs)
    return _to_device(cube, "vis")


def test_cross(gold, ps):
    g = gold
    d, e = _cube(g, ps, "D", tag="d", lsd=np.array([3])), _cube(g, ps, "E", tag="e", lsd=np.array([4, 5]))
    out = ps.CrossPowerSpectrum3D().process(d, e)
    assert out.spectrum.on_device and out.spectrum.dtype == np.complex128
    assert list(out.index_map["pol"]) == list(g["XDE/pol"]) == ["XX-YY", "XX-XX", "YY-YY", "YY-XX"]
    assert out.attrs["ps_norm"] == float(g["XDE/ps_norm"]) == out.ps_norm and out.attrs["tag"] == str(g["XDE/tag"]) == "d_x_e"
    assert d.attrs["effective_bandwidth"] == float(g["XDE/effective_bandwidth"]) and "effective_bandwidth" not in e.attrs
    assert list(out.attrs["lsd_p0"]) == [3] and list(out.attrs["lsd_p1"]) == [4, 5]
    for key in ("kx", "ky", "kpara", "uv_mask"):
        assert np.array_equal(out.datasets[key][:], g[f"D/{key}"])
    ref = g["XDE/ref"]
    _check("cross D x E", out.spectrum[:], twin.from_bits(ref, g["XDE/truth_bits"]), ref, float(g["XDE/e_ref"]), 2)
    assert np.array_equal(d.vis[:], g["D/ref"]) and np.array_equal(e.vis[:], g["E/ref"])


def test_auto(gold, ps):
    g = gold
    b = _cube(g, ps, "B", tag="b")
    out = ps.AutoPowerSpectrum3D().process(b)
    assert list(out.index_map["pol"]) == ["XX-XX"] and out.attrs["ps_norm"] == float(g["AUTO_B/ps_norm"]) and "effective_bandwidth" not in b.attrs  # window_los is "None"
    spec = out.spectrum[:]
    ref = g["AUTO_B/ref"]
    _check("auto B", spec, twin.from_bits(ref, g["AUTO_B/truth_bits"]), ref, float(g["AUTO_B/e_ref"]), 2)
    assert not spec.imag.any() and (spec.real >= 0).all()
    # two polarisations: a pol with itself is real to the last bit, the mixed pairs are conjugates of each other
    a = _cube(g, ps, "A", tag="a")
    out = ps.AutoPowerSpectrum3D().process(a)
    spec = out.spectrum[:]
    assert list(out.index_map["pol"]) == ["XX-XX", "XX-YY", "YY-XX", "YY-YY"]
    assert not spec[0].imag.any() and not spec[3].imag.any() and spec[1].imag.any() and np.array_equal(spec[1], np.conj(spec[2]))
    truth = twin.cross(g["A/ref"], g["A/ref"], out.attrs["ps_norm"]).astype(np.complex128)
    host = out.attrs["ps_norm"] * (g["A/ref"][:, None] * np.conj(g["A/ref"][None, :])).reshape(truth.shape)
    _check("auto A", spec, truth, host, twin.rel_err(host, truth), 2)


# ---- the cylindrical average


@pytest.mark.parametrize("name", list(CYL))
def test_cylindrical(gold, ps, name):
    g = gold
    spec, sigma, u, v, uv_mask, redshift, freq_center, delay, pol, kx, ky, kpara = cyl_input(g, name)
    cfg = CYL[name][2]
    cosmo = ps.get_cosmo()
    p3 = _to_device(twin.power_spectrum_3d(spec, pol, delay, u, v, kx, ky, kpara, uv_mask, redshift, freq_center, cosmo), "spectrum")
    task = ps.CylindricalPowerSpectrum2D(**cfg)
    task.setup(None if sigma is None else _to_device(twin.power_spectrum_3d(sigma, pol, delay, u, v, kx, ky, kpara, uv_mask, redshift, freq_center, cosmo), "spectrum"))
    out = task.process(p3)
    again = task.process(p3)
    got, got_w, got_n = out.spectrum[:], out.weight[:], out.neff[:]
    assert out.spectrum.on_device and got.dtype == np.complex128 and got_w.dtype == got_n.dtype == np.float64
    for key in ("spectrum", "weight", "neff"):  # two runs: the same bits
        assert np.array_equal(out.datasets[key][:].view(np.float64), again.datasets[key][:].view(np.float64), equal_nan=True), key
    ref, ref_w, ref_n = g[f"{name}/ref"], g[f"{name}/ref_weight"], g[f"{name}/ref_neff"]
    truth, truth_w, truth_n, count, abs_sum = (g[f"{name}/{k}"] for k in ("truth", "truth_weight", "truth_neff", "count", "abs_sum"))
    assert np.array_equal(np.isnan(got.real), np.isnan(ref.real)) and np.array_equal(np.isnan(got.imag), np.isnan(ref.imag)) and np.array_equal(np.isnan(got_n), np.isnan(ref_n))
    assert np.isnan(got.real).any() and (count == 0).any()
    ok = ~np.isnan(truth)
    if sigma is None:
        assert np.array_equal(got_w, ref_w) and np.array_equal(got_n, ref_n, equal_nan=True) and np.array_equal(got_w, np.broadcast_to(count.astype(float), got_w.shape))
    else:
        # sums of non-negative terms, each weight good to 3 ulp (a hypot, a square, a reciprocal): (n + 2) ulp on sum w;
        # twice that, the squares' own (n + 6) and the quotient's 1 on neff
        assert (np.abs(got_w - truth_w) <= (count + 2) * U * truth_w).all()
        assert (np.abs(got_n - truth_n)[ok] <= ((3 * count + 12) * U * truth_n)[ok]).all()
    bound = np.maximum(count - 1, 0) * U * abs_sum
    bound = np.minimum(bound, bound / np.where(truth_w > 0, truth_w, 1.0))
    err, err_ref = np.abs(got - truth), np.abs(ref - truth)
    worst = np.nanmax(np.where(ok & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0))
    ratio = float(err[ok].max() / err_ref[ok].max()) if err_ref[ok].max() > 0 else float("inf") if err[ok].max() > 0 else 0.0
    print(f"powerspec {name}: populations {count.tolist()} largest error / bound {worst:.3f}, error {err[ok].max():.3e} against the reference's {err_ref[ok].max():.3e} (ratio {ratio:.2f})")
    assert (err[ok] <= bound[ok]).all(), (name, worst)
    assert out.mask.dtype == np.bool_ and np.array_equal(out.mask[:], g[f"{name}/ref_mask"])
    assert np.array_equal(out.kpara[:], g[f"{name}/kpara"]) and np.array_equal(out.kperp[:], g[f"{name}/kperp"]) and np.array_equal(out.index_map["uv_dist"], g[f"{name}/uv_dist"])
    assert out.attrs["delay_cut"] == cfg.get("delay_cut", 300.0e-9) == out.delay_cut and np.array_equal(out.index_map["delay"], delay)
    assert np.array_equal(p3.spectrum[:], spec)


# ---- Jy / beam to kelvin


@pytest.mark.parametrize("ncyl,in_place", [(0, False), (1, True)])
def test_jy_to_kelvin(gold, ps, ncyl, in_place):
    from draco_amd.core import containers
    from draco_amd.core.products import TransitTelescope

    g = gold
    tel = TransitTelescope(g["JY/freq"], lmax=12, ncyl=2, nfeed_cyl=3)
    rm = containers.RingMap(beam=1, pol=np.array(["XX", "YY"]), freq=g["JY/freq"], ra=6, el=5)
    rm.map[:], rm.weight[:] = g["JY/map"], g["JY/weight"]
    _to_device(rm, "map", "weight")
    task = ps.TransformJyPerBeamToKelvin(ncyl=ncyl, in_place=in_place)
    task.setup(tel)
    out = task.process(rm)
    assert (out is rm) == in_place and out.map.on_device and out.weight.on_device
    assert np.array_equal(out.map[:], g[f"JY/ref_map{ncyl}"]) and np.array_equal(out.weight[:], g[f"JY/ref_weight{ncyl}"])
    if not in_place:
        assert np.array_equal(rm.map[:], g["JY/map"]) and np.array_equal(rm.weight[:], g["JY/weight"])


# ---- the chain


def test_chain(ps):
    """DelaySpectrumFFT -> SpatialTransformDelayMap -> AutoPowerSpectrum3D -> CylindricalPowerSpectrum2D ->
    SphericalPowerSpectrum2Dto1D on a device-resident ring map [1 beam, 2 pol, 8 freq, 24 ra, 10 el].  Every stage is
    compared, on the input the device chain handed it, with its NumPy restatement (pinned to the reference's vectors
    by test_delay_host.py and test_powerspec_host.py) and with the long-double truth, under the criteria above; the end
    of the chain is compared with the end of the NumPy chain."""
    from draco_amd.analysis.delay import DelaySpectrumFFT
    from draco_amd.core import containers

    npol, nfreq, nra, nel = 2, 8, 24, 10
    rng = np.random.default_rng(2824)
    ra = 10.0 + 0.2 * np.arange(nra)
    el = np.sin(np.radians(0.2 * (np.arange(nel) - nel / 2)))
    freq = 600.0 + 0.390625 * np.arange(nfreq)
    rm = containers.RingMap(beam=1, pol=np.array(["XX", "YY"]), freq=freq, ra=ra, el=el)
    rmap = rng.normal(size=(1, npol, nfreq, nra, nel))
    rm.map[:], rm.weight[:] = rmap, rng.uniform(0.5, 1.5, size=(npol, nfreq, nra, nel))
    _to_device(rm, "map", "weight")
    cosmo = ps.get_cosmo()
    cyl_cfg = dict(bl_min=20.0, bl_max=110.0, Nbins_2D=6, delay_cut=0.0)

    ds = DelaySpectrumFFT(complex_timedomain=True, sample_axis="ra", remove_mean=False).process(rm)
    st = ps.SpatialTransformDelayMap()
    st.setup(TEL)
    cube = st.process(ds)
    p3 = ps.AutoPowerSpectrum3D().process(cube)
    cyl = ps.CylindricalPowerSpectrum2D(**cyl_cfg)
    cyl.setup()
    p2 = cyl.process(p3)
    with np.errstate(divide="ignore", invalid="ignore"):
        p1 = ps.SphericalPowerSpectrum2Dto1D(Nbins_3D=4).process(p2)
    assert list(ds.attrs["baseline_axes"]) == ["beam", "pol", "el"] and cube.vis.on_device and p3.spectrum.on_device and p2.spectrum.on_device

    # stage 1, the delay transform: the restatement of the reference's inverse-FFT estimator
    dview = rmap.transpose(0, 1, 4, 3, 2).reshape(npol * nel, nra, nfreq)
    tcfg = dict(time_frac=0.0, freq_frac=0.0, remove_mean=False, weight_boost=1.0, window="nuttall", complex_timedomain=True)
    wview = np.ones_like(dview)
    host_ds = delay_twin.evaluate(dview, wview, None, nfreq, np.arange(nfreq), tcfg, "fft")[0]
    truth_ds = delay_twin.evaluate(dview, wview, None, nfreq, np.arange(nfreq), tcfg, "fft", truth=True)[0]
    spec = ds.spectrum[:]
    _check("chain delay", spec, truth_ds, host_ds, twin.rel_err(host_ds, truth_ds), 2)

    # stage 2, the spatial transform of what stage 1 produced (24 x 10: Bluestein on both axes)
    dec = twin.LATITUDE + np.degrees(np.arcsin(el))
    view = twin.spectrum_to_cube(spec, (1, npol, nel), ["beam", "pol", "el"])
    w_ra, w_el = ps._taper(ra, dec, "tukey-0.5")
    host_vis = np.stack([np.stack([ps.image_to_uv(np.ascontiguousarray(view[p, d]), ra, dec)[0] for d in range(nfreq)]) for p in range(npol)])
    truth_vis = twin.uv_full(view, w_ra, w_el).astype(np.complex128)
    vis = cube.vis[:]
    _check("chain spatial", vis, truth_vis, host_vis, twin.rel_err(host_vis, truth_vis), 8)

    # stage 3, the auto spectrum of what stage 2 produced
    norm = p3.attrs["ps_norm"]
    assert norm == cube.attrs["volume"] * (1 / (ps.noise_equivalent_bandwidth(nfreq, "nuttall") * cube.attrs["effective_ra"] * cube.attrs["effective_dec"]))
    host_p3 = norm * (vis[:, None] * np.conj(vis[None, :])).reshape(npol * npol, nfreq, nra, nel)
    truth_p3 = twin.cross(vis, vis, norm).astype(np.complex128)
    s3 = p3.spectrum[:]
    _check("chain auto", s3, truth_p3, host_p3, twin.rel_err(host_p3, truth_p3), 2)
    assert not s3[0].imag.any() and not s3[3].imag.any()

    # stage 4, the cylindrical average of what stage 3 produced
    u_min, u_max, kperp = cyl._bins(p3)
    bm = ps.cyl_bin_map(p3.index_map["u"], p3.index_map["v"], p3.uv_mask[:], u_min, u_max, kperp, p3.attrs["redshift"], cosmo)
    t_s, t_w, t_n, count, t_a = twin.cyl_bin(s3, None, bm, len(kperp) - 1)
    g_s, g_w, g_n = p2.spectrum[:], p2.weight[:], p2.neff[:]
    host_s = np.full(g_s.shape, np.nan + 1j * np.nan)
    for p in range(npol * npol):
        for d in range(nfreq):
            flat, uu, vv = ps.reshape_data_cube(s3[p, d], p3.index_map["u"], p3.index_map["v"], u_min, u_max)
            mflat = ps.reshape_data_cube(p3.uv_mask[:], p3.index_map["u"], p3.index_map["v"], u_min, u_max)[0]
            with np.errstate(divide="ignore", invalid="ignore"):
                host_s[p, d], hw, hn = ps.get_2d_ps(flat[mflat], np.ones(int(mflat.sum())), kperp, uu[mflat], vv[mflat], p3.attrs["redshift"], cosmo)
            assert np.array_equal(g_w[p, d], hw) and np.array_equal(g_n[p, d], hn, equal_nan=True)
    assert (count > 0).sum() >= 2 and np.array_equal(np.isnan(g_s), np.isnan(host_s)) and np.array_equal(np.isnan(g_s), np.isnan(t_s))
    ok = ~np.isnan(t_s)
    bound = np.maximum(count - 1, 0) * U * t_a / np.maximum(t_w, 1.0)
    print(f"powerspec chain cylindrical: populations {count.tolist()} largest error / bound {np.max(np.abs(g_s - t_s)[ok & (bound > 0)] / bound[ok & (bound > 0)]):.3f}")
    assert (np.abs(g_s - t_s)[ok] <= bound[ok]).all()

    # stage 5 is the host function itself; the end of the chain against the end of the NumPy chain: sums of products of
    # a handful of roundings each, no cancellation in the spectra of a polarisation with itself
    with np.errstate(divide="ignore", invalid="ignore"):
        end = [ps.get_1d_ps(host_s[p], p2.kperp[:], p2.kpara[:], g_w[p], signal_window=p2.mask[:][p], Nbins_3D=4) for p in range(npol * npol)]
    for p in (0, 3):
        assert np.array_equal(p1.k1D[:][p], end[p][0], equal_nan=True)
        fin = np.isfinite(end[p][1])
        assert fin.any() and np.array_equal(fin, np.isfinite(p1.spectrum[:][p]))
        assert np.allclose(p1.spectrum[:][p][fin], end[p][1][fin], rtol=1e-12, atol=0)
