"""Host-side checks of the delay-spectrum feature: the NumPy twin against the vectors produced by executing the
reference (tests/golden/delay*.npz), the host functions of ``draco_amd`` against the stored reference values, the new
containers, and every error path that needs no GPU."""

import os

import numpy as np
import pytest

import delay_twin as twin
from conftest import GOLDEN

CFG = dict(time_frac=0.0, freq_frac=0.0, remove_mean=True, weight_boost=1.0, window="nuttall", complex_timedomain=False)
CASES = {
    "R32": ("R32", {}),
    "R70": ("R70", dict(freq_frac=0.3)),
    "C46": ("C46", dict(complex_timedomain=True, remove_mean=False)),
    "C46b": ("C46", dict(complex_timedomain=True, remove_mean=False)),
    "C48w": ("C48w", dict(complex_timedomain=True, weight_boost=4.0, window="blackman_harris")),
    "C48n": ("C48w", dict(complex_timedomain=True, weight_boost=4.0, window=None)),
    "R1100": ("R1100", {}),
}


@pytest.fixture(scope="module")
def gold():
    g = {}
    for name in ("delay.npz", "delay_r1100.npz"):
        with np.load(os.path.join(GOLDEN, name)) as z:
            g.update({k: z[k] for k in z.files})
    return g


@pytest.mark.parametrize("name", list(CASES))
def test_twin_matches_reference(gold, name):
    g = gold
    src, over = CASES[name]
    cfg = {**CFG, **over}
    dv, wv = g[f"{src}/vis"].transpose(1, 2, 0), g[f"{src}/weight"].transpose(1, 2, 0)
    ndelay = len(g[f"{name}/delays"])
    spec, mask = twin.evaluate(dv, wv, g[f"{name}/prior"], ndelay, g[f"{name}/channel_ind"], cfg, "wiener")
    e_ref = float(g[f"{name}/e_ref"])
    assert twin.rel_err(spec, g[f"{name}/ref"]) <= 1e-3 * e_ref + 1e-12
    assert twin.rel_err(g[f"{name}/ref"], g[f"{name}/truth"]) == e_ref
    assert ((g[f"{name}/cond"] >= 1e3) & (g[f"{name}/cond"] <= 1e7)).all()
    if f"{name}/ref_mask" in g:
        assert np.array_equal(mask, g[f"{name}/ref_mask"])


@pytest.mark.parametrize("name", ["FFT24w", "FFT24n", "FFT23w", "FFT23n", "RM", "RM70", "RM1100"])
def test_twin_matches_reference_other(gold, name):
    g = gold
    if name.startswith("RM"):
        rmap, rw = g[f"{name}/map"], g[f"{name}/weight"]
        nbase = rmap.shape[0] * rmap.shape[1] * rmap.shape[4]
        dv = rmap.transpose(0, 1, 4, 3, 2).reshape(nbase, rmap.shape[3], rmap.shape[2])
        wv = np.broadcast_to(rw[np.newaxis], rmap.shape).transpose(0, 1, 4, 3, 2).reshape(dv.shape)
        cfg = {**CFG, "freq_frac": 0.3} if name == "RM70" else CFG
        spec, mask = twin.evaluate(dv, wv, g[f"{name}/prior"], len(g[f"{name}/delays"]), g[f"{name}/channel_ind"], cfg, "wiener")
    else:
        src = name[:-1] + "w"
        cfg = {**CFG, "complex_timedomain": True, "window": "nuttall" if name.endswith("w") else None}
        spec, mask = twin.evaluate(g[f"{src}/vis"].transpose(1, 2, 0), g[f"{src}/weight"].transpose(1, 2, 0), None, len(g[f"{name}/delays"]), g[f"{name}/channel_ind"], cfg, "fft")
    e_ref = float(g[f"{name}/e_ref"])
    assert twin.rel_err(spec, g[f"{name}/ref"]) <= 1e-3 * e_ref + 1e-12
    assert twin.rel_err(g[f"{name}/ref"], g[f"{name}/truth"]) == e_ref
    if f"{name}/ref_mask" in g:
        assert np.array_equal(mask, g[f"{name}/ref_mask"])


def test_twin_functions_and_power_spectrum(gold):
    g = gold
    r = twin.wiener(g["fn_wr/ps"], g["fn_wr/data"], 32, g["fn_wr/Ni"], "nuttall", g["fn_wr/fsel"], False)
    assert twin.rel_err(r, g["fn_wr/ref"]) <= 1e-3 * float(g["fn_wr/e_ref"]) + 1e-12
    r = twin.wiener(g["fn_wc/ps"], g["fn_wc/data"], 23, g["fn_wc/Ni"], None, None, True)
    assert twin.rel_err(r, g["fn_wc/ref"]) <= 1e-3 * float(g["fn_wc/e_ref"]) + 1e-12
    r = twin.wiener(g["fn_wc94/ps"], g["fn_wc94/data"], 47, g["fn_wc94/Ni"], "blackman", None, True)
    assert twin.rel_err(r, g["fn_wc94/ref"]) <= 1e-3 * float(g["fn_wc94/e_ref"]) + 1e-12
    r = twin.fft_estimate(g["fn_fft/data"].copy(), 23, "nuttall")
    assert twin.rel_err(r, g["fn_fft/ref"]) <= 1e-3 * float(g["fn_fft/e_ref"]) + 1e-12
    for k in ("fn_wr", "fn_wc", "fn_wc94", "fn_fft"):
        assert twin.rel_err(g[f"{k}/ref"], g[f"{k}/truth"]) == float(g[f"{k}/e_ref"])
    with pytest.raises(ValueError):
        twin.fft_estimate(g["fn_fft/data"][:, :22].copy(), 23, "nuttall")
    ps, flagged = twin.power_spectrum(g["C48w/ref"], g["C48w/ref_mask"])
    assert np.array_equal(ps, g["PS/ref"]) and np.array_equal(flagged, g["PS/ref_mask"])


def test_circulant_structure(gold):
    """F^T N^-1 F is fixed by one cosine (and one sine) sequence: what csrc/delay.hip builds its matrix from."""
    g = gold
    fsel = g["fn_wr/fsel"]
    G = twin.wiener_matrix(32, g["fn_wr/Ni"], fsel, "nuttall", False, np.zeros(32))
    c = np.where((fsel == 0) | (fsel == 16), 1.0, 2.0) * g["fn_wr/Ni"] * twin.window(fsel, 17, "nuttall") ** 2
    gseq = (c[:, None] * np.cos(2 * np.pi * fsel[:, None] * np.arange(32)[None, :] / 32)).sum(axis=0)
    i, j = np.indices((32, 32))
    assert np.abs(G - gseq[(i - j) % 32]).max() <= 1e-12 * np.abs(G).max()
    Ni = g["fn_wc/Ni"]
    G = twin.wiener_matrix(23, Ni, np.arange(23), None, True, np.zeros(23))
    arg = 2 * np.pi * np.arange(23)[:, None] * np.arange(23)[None, :] / 23
    gs, ss = (2 * Ni[:, None] * np.cos(arg)).sum(axis=0), (2 * Ni[:, None] * np.sin(arg)).sum(axis=0)
    i, j = np.indices((46, 46))
    d = (i // 2 - j // 2) % 23
    want = np.where(i % 2 == j % 2, gs[d], np.where(i % 2 == 1, ss[d], -ss[d]))
    assert np.abs(G - want).max() <= 1e-12 * np.abs(G).max()


def test_window_generalised(gold):
    from draco_amd.util import tools

    g = gold
    x = g["win/x"]
    assert (x < 0).any() and (x > 1).any()
    for name, ref in zip(g["win/names"], g["win/ref"]):
        w = tools.window_generalised(x, window=str(name))
        assert np.abs(w - ref).max() <= 1e-15, name
        assert not w[(x < 0) | (x > 1)].any()
    with pytest.raises(KeyError):
        tools.window_generalised(x, window="boxcar")


def test_fourier_matrices_host(gold):
    from draco_amd.analysis import delay

    g = gold
    fsel = g["fm/fsel"]
    for nm, fn in (("r2c", delay.fourier_matrix_r2c), ("c2r", delay.fourier_matrix_c2r), ("c2c", delay.fourier_matrix_c2c), ("c", delay.fourier_matrix)):
        for tag, sel in (("all", None), ("sel", fsel)):
            got = fn(16, sel, device=False)
            assert got.shape == g[f"fm/{nm}_{tag}"].shape and got.dtype == g[f"fm/{nm}_{tag}"].dtype
            assert np.abs(got - g[f"fm/{nm}_{tag}"]).max() <= 1e-15
    assert np.abs(delay.fourier_matrix_c2c(7, device=False) - g["fm/c2c_odd"]).max() <= 1e-15


def _stream(freq, nstack=2, nra=4):
    from draco_amd.core import containers

    return containers.SiderealStream(freq=freq, ra=nra, stack=nstack)


@pytest.mark.parametrize("name", ["R32", "R70", "C46", "R1100"])
def test_calculate_delays(gold, name):
    from draco_amd.analysis.delay import DelaySpectrumWienerFilter

    g = gold
    cfg = {"R32": dict(skip_nyquist=False), "R70": dict(skip_nyquist=True, freq_zero=600.0, freq_spacing=0.390625), "C46": dict(complex_timedomain=True), "R1100": dict(skip_nyquist=False)}[name]
    delays, channel_ind = DelaySpectrumWienerFilter(sample_axis="ra", **cfg)._calculate_delays(_stream(g[f"{name}/freq"]))
    assert np.array_equal(delays, g[f"{name}/delays"]) and np.array_equal(channel_ind, g[f"{name}/channel_ind"])
    assert channel_ind.dtype == np.int64
    if name == "R70":
        assert channel_ind[0] == 5 and len(delays) == 70


def test_task_defaults_match_the_reference():
    from draco_amd.analysis import delay

    t = delay.DelaySpectrumWienerFilter()
    want = dict(freq_zero=None, freq_spacing=None, nfreq=None, skip_nyquist=True, apply_window=True, window="nuttall", complex_timedomain=False, use_average_weights=True, weight_boost=1.0,
                freq_frac=0.0, time_frac=0.0, remove_mean=True, scale_freq=False, dataset=None, save_spectrum_mask=False)
    for k, v in want.items():
        assert getattr(t, k) == v, k
    assert issubclass(delay.DelaySpectrumWienerFilterIteratePS, delay.DelaySpectrumWienerFilter)
    assert issubclass(delay.DelaySpectrumFFT, delay.DelayTransformBase)


def test_containers():
    from draco_amd.core import containers

    delays = np.fft.fftshift(np.fft.fftfreq(8, d=0.5))
    src = _stream(np.linspace(400.0, 410.0, 5))
    src.attrs["tag"] = "x"
    dt = containers.DelayTransform(baseline=3, sample=np.arange(4.0), delay=delays, attrs_from=src, weight_boost=2.5)
    assert isinstance(dt, containers.DelayContainer)
    assert dt.spectrum.shape == (3, 4, 8) and dt.spectrum.dtype == np.complex128 and dt.spectrum.attrs["axis"] == ["baseline", "sample", "delay"]
    assert dt.weight_boost == 2.5 and dt.attrs["tag"] == "x" and np.array_equal(dt.delay, delays)
    assert not dt.spectrum[:].any() and "spectrum_mask" not in dt.datasets
    dt.add_dataset("spectrum_mask")
    assert dt.datasets["spectrum_mask"].shape == (3, 4) and dt.datasets["spectrum_mask"].dtype == np.bool_
    dt.add_dataset("weight")
    assert dt.weight.shape == (3, 4, 8) and dt.weight.dtype == np.float32
    dt.attrs["freq"] = src.freq
    assert np.array_equal(dt.freq, src.freq)
    dt.create_index_map("stack", np.arange(3))
    assert np.array_equal(dt.index_map["stack"], np.arange(3))
    ps = containers.DelaySpectrum(attrs_from=dt, axes_from=dt)
    assert ps.spectrum.shape == (3, 8) and ps.spectrum.dtype == np.float64 and len(ps.index_map["sample"]) == 1
    assert ps.weight_boost == 1.0  # as in the reference: the constructor's default overwrites the copied attribute
    ps.add_dataset("spectrum_mask")
    ps.add_dataset("spectrum_samples")
    assert ps.datasets["spectrum_mask"].shape == (3,) and ps.datasets["spectrum_samples"].shape == (1, 3, 8)
    assert np.array_equal(ps.freq, src.freq)


def test_errors_without_a_gpu(gold):
    from draco_amd.analysis import delay

    s = _stream(gold["R32/freq"])
    with pytest.raises(NotImplementedError, match="use_average_weights"):
        delay.DelaySpectrumWienerFilter(sample_axis="ra", use_average_weights=False).process(s)
    with pytest.raises(NotImplementedError, match="scale_freq"):
        delay.DelaySpectrumFFT(sample_axis="ra", scale_freq=True).process(s)
    with pytest.raises(ValueError, match="window"):
        delay.DelaySpectrumWienerFilter(window="triangular")
    with pytest.raises(AttributeError):
        delay.DelaySpectrumWienerFilter(nsamp=3)
    with pytest.raises(ValueError, match="has no dataset 'map'"):
        delay.DelaySpectrumWienerFilter(sample_axis="ra", dataset="map").process(s)
    with pytest.raises(ValueError, match="no sample axis 'time'"):
        delay.DelaySpectrumWienerFilter(sample_axis="time").process(s)
    with pytest.raises(ValueError, match="no sample axis None"):
        delay.DelaySpectrumFFT(complex_timedomain=True).process(s)
    with pytest.raises(ValueError, match="inverse FFT"):
        delay.DelaySpectrumFFT(sample_axis="ra").process(s)
    with pytest.raises(ValueError, match="no delay power spectrum"):
        delay.DelaySpectrumWienerFilter(sample_axis="ra", skip_nyquist=False).process(s)
    big = _stream(400.0 + 0.390625 * np.arange(1026))
    from draco_amd.core import containers

    dps = containers.DelaySpectrum(baseline=2, delay=2050)
    t = delay.DelaySpectrumWienerFilter(sample_axis="ra", skip_nyquist=False)
    t.setup(dps)
    with pytest.raises(ValueError, match="order 2050"):
        t.process(big)
