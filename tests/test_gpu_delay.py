"""GPU delay spectrum estimators (`csrc/delay.hip`, `draco_amd/analysis/delay.py`) against a long-double truth and
against vectors produced by executing the reference (`tests/gen_golden_delay.py` -> tests/golden/delay*.npz).

Error measure, as for DAYENU.  Per case `e_gpu = max |gpu - truth| / max |truth|` with the truth (`tests/delay_twin.py`,
long double throughout) rounded once to complex128; required: `e_gpu <= max(2 e_ref, 2**-51)`, `e_ref` the same
measure of the reference's output (stored by the generator), and against the reference's vectors `<= 3 e_ref + 2**-51`.
The factor 2 is the margin for another rounding order; the floor is one float64 ulp of the largest value, doubled.

`e_ref` of the stream cases (complex64 data, float32 weights) is about 5e-8: the reference takes the mean of the data
and of the weights in single precision, so those cases check the paths, the masks and the exact properties but pin
the arithmetic only to single precision.  The float64 cases pin it to float64 at every order the code treats
differently: ring maps of order 32 (RM, e_ref 1.3e-13; one factorisation block), 70 (RM70, 1.9e-12; three blocks, two
tiles, freq_frac) and 1100 (RM1100, 1.3e-10; above 1024), the functions at order 32 (8.0e-14), 46 (1.6e-14) and 94
(complex, 6.9e-13), and the FFT function (1.8e-16; the floor applies).  Every input container is device resident.  Each
test prints `e_gpu` and `e_ref` before it asserts.
"""

import os

import numpy as np
import pytest

import delay_twin as twin
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FLOOR = 2.0**-51


@pytest.fixture(scope="module")
def gold():
    g = {}
    for name in ("delay.npz", "delay_r1100.npz"):
        with np.load(os.path.join(GOLDEN, name)) as z:
            g.update({k: z[k] for k in z.files})
    return g


def _check(name, got, truth, ref, e_ref):
    e_gpu, e_tri = twin.rel_err(got, truth), twin.rel_err(got, ref)
    print(f"delay {name}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} (to the reference {e_tri:.3e})")
    assert np.isfinite(got.view(np.float64)).all()
    assert e_gpu <= max(2 * e_ref, FLOOR), (name, e_gpu, e_ref)
    assert e_tri <= 3 * e_ref + FLOOR, (name, e_tri, e_ref)


CASES = {
    "R32": ("R32", dict(skip_nyquist=False, save_spectrum_mask=True)),
    "R70": ("R70", dict(skip_nyquist=True, freq_zero=600.0, freq_spacing=0.390625, freq_frac=0.3)),
    "C46": ("C46", dict(complex_timedomain=True, remove_mean=False)),
    "C48w": ("C48w", dict(complex_timedomain=True, weight_boost=4.0, window="blackman_harris", save_spectrum_mask=True)),
    "C48n": ("C48w", dict(complex_timedomain=True, weight_boost=4.0, window="blackman_harris", save_spectrum_mask=True, apply_window=False)),
    "R1100": ("R1100", dict(skip_nyquist=False)),
}


def _stream(g, src, device=False):
    from draco_amd.core import containers
    from draco_amd.device import Context

    vis, weight = g[f"{src}/vis"], g[f"{src}/weight"]
    s = containers.SiderealStream(freq=g[f"{src}/freq"], ra=vis.shape[2], stack=vis.shape[1])
    s.vis[:] = vis
    s.weight[:] = weight
    if device:
        ctx = Context.get()
        s.vis.set_device(ctx.to_device(vis))
        s.weight.set_device(ctx.to_device(weight))
    return s


def _dps(prior, delays):
    from draco_amd.core import containers

    d = containers.DelaySpectrum(baseline=prior.shape[0], delay=delays)
    d.spectrum[:] = prior
    return d


def _wiener(g, name, device=True, **over):
    from draco_amd.analysis.delay import DelaySpectrumWienerFilter

    src, cfg = CASES[name]
    s = _stream(g, src, device)
    task = DelaySpectrumWienerFilter(sample_axis="ra", **{**cfg, **over})
    task.setup(_dps(g[f"{name}/prior"], g[f"{name}/delays"]))
    out = task.process(s)
    assert out.spectrum.on_device and out.spectrum.dtype == np.complex128
    return task, s, out


@pytest.mark.parametrize("name", list(CASES))
def test_wiener_stream(gold, name):
    g = gold
    src, cfg = CASES[name]
    task, s, out = _wiener(g, name)
    delays, channel_ind = task._calculate_delays(s)
    assert np.array_equal(delays, g[f"{name}/delays"]) and np.array_equal(channel_ind, g[f"{name}/channel_ind"])
    spec = out.spectrum[:]
    ref, truth = g[f"{name}/ref"], g[f"{name}/truth"]
    assert spec.shape == ref.shape
    _check(name, spec, truth, ref, float(g[f"{name}/e_ref"]))
    # skipped baselines and dropped samples: exact zeros, exactly where the reference has them
    zero_rows = ~ref.any(axis=2)
    assert not spec[zero_rows].any() and spec[~zero_rows].any(axis=1).all()
    if cfg.get("save_spectrum_mask"):
        m = out.datasets["spectrum_mask"][:]
        assert m.dtype == np.bool_ and np.array_equal(m, g[f"{name}/ref_mask"]) and np.array_equal(m, zero_rows)
    else:
        assert "spectrum_mask" not in out.datasets
    if not cfg.get("complex_timedomain"):
        assert not spec.imag.any()
    if src == "C48w":  # baselines 0 and 3 share data, weights and prior
        assert np.array_equal(spec[0].view(np.uint64), spec[3].view(np.uint64))
    # the inputs are where they were and what they were
    assert s.vis.on_device and s.weight.on_device and s.vis._host is None
    assert np.array_equal(s.vis[:].view(np.uint32), g[f"{src}/vis"].view(np.uint32)) and np.array_equal(s.weight[:], g[f"{src}/weight"])
    assert out.attrs["baseline_axes"] == ["stack"] and np.array_equal(out.attrs["freq"], g[f"{src}/freq"])
    assert out.attrs["window_los"] == (task.window if task.apply_window else "None") and out.weight_boost == task.weight_boost


def test_small_workspace_batches(gold):
    """One baseline per batch gives the same bits as one batch."""
    _, _, a = _wiener(gold, "C48w")
    _, _, b = _wiener(gold, "C48w", workspace_mib=0)
    assert np.array_equal(a.spectrum[:].view(np.uint64), b.spectrum[:].view(np.uint64))


def test_iterate_ps(gold):
    from draco_amd.analysis.delay import DelaySpectrumWienerFilterIteratePS

    g = gold
    task = DelaySpectrumWienerFilterIteratePS(sample_axis="ra", complex_timedomain=True, remove_mean=False)
    task.setup()
    s = _stream(g, "C46")
    for name in ("C46", "C46b"):
        out = task.process(s, _dps(g[f"{name}/prior"], g["C46/delays"]))
        _check(f"iterate {name}", out.spectrum[:], g[f"{name}/truth"], g[f"{name}/ref"], float(g[f"{name}/e_ref"]))


@pytest.mark.parametrize("name", ["FFT24w", "FFT24n", "FFT23w", "FFT23n"])
def test_fft_stream(gold, name):
    from draco_amd.analysis.delay import DelaySpectrumFFT

    g = gold
    src = name[:-1] + "w"
    s = _stream(g, src, device=True)
    out = DelaySpectrumFFT(sample_axis="ra", complex_timedomain=True, apply_window=name.endswith("w"), save_spectrum_mask=True).process(s)
    spec = out.spectrum[:]
    _check(name, spec, g[f"{name}/truth"], g[f"{name}/ref"], float(g[f"{name}/e_ref"]))
    assert np.array_equal(out.datasets["spectrum_mask"][:], g[f"{name}/ref_mask"])
    assert not spec[g[f"{name}/ref_mask"]].any()


def test_fft_errors(gold):
    from draco_amd.analysis.delay import DelaySpectrumFFT
    from draco_amd.device import Context

    g = gold
    s = _stream(g, "FFT23w")
    s.weight[:] = g["FFTcut/weight"]
    s.weight.set_device(Context.get().to_device(g["FFTcut/weight"]))
    with pytest.raises(ValueError, match="cut channels"):
        DelaySpectrumFFT(sample_axis="ra", complex_timedomain=True).process(s)
    with pytest.raises(ValueError, match="inverse FFT"):
        DelaySpectrumFFT(sample_axis="ra").process(_stream(g, "FFT23w", device=True))


RINGMAPS = {
    "RM": dict(skip_nyquist=False, save_spectrum_mask=True),
    "RM70": dict(skip_nyquist=True, freq_zero=600.0, freq_spacing=0.390625, freq_frac=0.3, save_spectrum_mask=True),
    "RM1100": dict(skip_nyquist=False),
}


@pytest.mark.parametrize("name", list(RINGMAPS))
def test_ringmap(gold, name):
    """float64 ring maps, device resident; the weight has no `beam` axis (stride 0 in the view)."""
    from draco_amd.analysis.delay import DelaySpectrumWienerFilter
    from draco_amd.core import containers
    from draco_amd.device import Context

    g = gold
    rmap, rw = g[f"{name}/map"], g[f"{name}/weight"]
    nb, npol, nfreq, nra, nel = rmap.shape
    rm = containers.RingMap(freq=g[f"{name}/freq"], beam=nb, pol=np.array(["XX", "YY"])[:npol], ra=nra, el=np.linspace(-1, 1, nel), allocate=False)
    ctx = Context.get()
    rm.attach("map", ctx.to_device(rmap))
    rm.attach("weight", ctx.to_device(rw))
    task = DelaySpectrumWienerFilter(dataset="map", sample_axis="ra", **RINGMAPS[name])
    task.setup(_dps(g[f"{name}/prior"], g[f"{name}/delays"]))
    out = task.process(rm)
    assert rm.map._host is None and rm.weight._host is None
    spec = out.spectrum[:]
    ndelay = len(g[f"{name}/delays"])
    assert np.array_equal(out.delay, g[f"{name}/delays"])
    assert spec.shape == (nb * npol * nel, nra, ndelay) and out.attrs["baseline_axes"] == ["beam", "pol", "el"]
    assert all(np.array_equal(out.index_map[ax], rm.index_map[ax]) for ax in ("beam", "pol", "el"))
    _check(f"ring map {name}", spec, g[f"{name}/truth"], g[f"{name}/ref"], float(g[f"{name}/e_ref"]))
    zero_rows = ~g[f"{name}/ref"].any(axis=2)
    assert not spec[zero_rows].any() and not spec.imag.any()
    if RINGMAPS[name].get("save_spectrum_mask"):
        assert np.array_equal(out.datasets["spectrum_mask"][:], g[f"{name}/ref_mask"]) and np.array_equal(g[f"{name}/ref_mask"], zero_rows)
    if name == "RM":
        assert zero_rows[1 * nel + 2].all()  # the fully flagged (pol 1, el 2) column
    assert np.array_equal(rm.map[:], rmap) and np.array_equal(rm.weight[:], rw)


def test_functions(gold):
    from draco_amd.analysis import delay

    g = gold
    r = delay.delay_spectrum_wiener_filter(g["fn_wr/ps"], g["fn_wr/data"], 32, g["fn_wr/Ni"], window="nuttall", fsel=g["fn_wr/fsel"], complex_timedomain=False)
    assert r.is_cuda and r.dtype.is_floating_point
    _check("fn wiener real", r.cpu().numpy(), g["fn_wr/truth"], g["fn_wr/ref"], float(g["fn_wr/e_ref"]))
    r = delay.delay_spectrum_wiener_filter(g["fn_wc/ps"], g["fn_wc/data"], 23, g["fn_wc/Ni"], window=None, complex_timedomain=True)
    assert r.is_cuda and r.dtype.is_complex
    _check("fn wiener complex", r.cpu().numpy(), g["fn_wc/truth"], g["fn_wc/ref"], float(g["fn_wc/e_ref"]))
    r = delay.delay_spectrum_wiener_filter(g["fn_wc94/ps"], g["fn_wc94/data"], 47, g["fn_wc94/Ni"], window="blackman", complex_timedomain=True)
    _check("fn wiener complex, order 94", r.cpu().numpy(), g["fn_wc94/truth"], g["fn_wc94/ref"], float(g["fn_wc94/e_ref"]))
    data = g["fn_fft/data"].copy()
    r = delay.delay_spectrum_fft(data, 23, window="nuttall")
    assert r.is_cuda and np.array_equal(data, g["fn_fft/data"])
    _check("fn fft", r.cpu().numpy(), g["fn_fft/truth"], g["fn_fft/ref"], float(g["fn_fft/e_ref"]))
    with pytest.raises(ValueError):
        delay.delay_spectrum_fft(data[:, :22], 23)


def test_fourier_matrices_device(gold):
    """The device matrices reduce their arguments in integers.  Against the long-double values: x = 2 m / N < 2 is
    rounded once (pi x 2**-52 in the angle), sincospi is good to an ulp or two of 1, the truth is rounded once:
    6 x 2**-52 covers the sum."""
    from draco_amd.analysis import delay

    fsel = gold["fm/fsel"]
    for N, sel, cplx in ((16, None, False), (16, fsel, False), (16, fsel, True), (7, None, True), (1100, np.arange(551), False)):
        fn = delay.fourier_matrix_c2c if cplx else delay.fourier_matrix_r2c
        F = fn(N, sel).cpu().numpy()
        full = np.arange(N if cplx else N // 2 + 1) if sel is None else sel
        T = twin.fourier(N, full, cplx, truth=True)
        assert F.shape == T.shape and np.abs(F - T.astype(np.float64)).max() <= 6 * 2.0**-52
    for nm, fn in (("c2r", delay.fourier_matrix_c2r), ("c", delay.fourier_matrix)):
        assert np.array_equal(fn(16, fsel).cpu().numpy(), fn(16, fsel, device=False))


def test_after_dayenu(gold):
    """A stream straight from DayenuDelayFilter.process (device-resident vis and weight) goes through the Wiener
    filter where it lies: no host copy of either dataset appears."""
    import types

    from draco_amd.analysis.dayenu import DayenuDelayFilter
    from draco_amd.analysis.delay import DelaySpectrumWienerFilter
    from draco_amd.core import containers

    g = gold
    vis, weight = g["R32/vis"], g["R32/weight"].copy()
    weight[:, 1, 2] = 1.0  # DAYENU's single mask would otherwise flag every channel of entry 1
    prod = np.zeros(3, dtype=[("input_a", "<u2"), ("input_b", "<u2")])
    prod["input_b"] = np.arange(1, 4)
    s = containers.SiderealStream(freq=g["R32/freq"], ra=vis.shape[2], prod=prod, input=4)
    s.vis[:] = vis
    s.weight[:] = weight
    feedpos = np.zeros((4, 2))
    feedpos[1:, 1] = [3.0, 6.0, 9.0]
    f = DayenuDelayFilter(epsilon=1e-6)
    f.setup(types.SimpleNamespace(feedpositions=feedpos, lmax=1, mmax=1, frequencies=None))
    s = f.process(s)
    assert s.vis._host is None and s.weight._host is None
    task = DelaySpectrumWienerFilter(sample_axis="ra", skip_nyquist=False)
    task.setup(_dps(g["R32/prior"], g["R32/delays"]))
    out = task.process(s)
    assert s.vis._host is None and s.weight._host is None and out.spectrum.on_device
    fv, fw = s.vis[:], s.weight[:]
    cfg = dict(time_frac=0.0, freq_frac=0.0, remove_mean=True, weight_boost=1.0, window="nuttall", complex_timedomain=False)
    truth, _ = twin.evaluate(fv.transpose(1, 2, 0), fw.transpose(1, 2, 0), g["R32/prior"], 32, np.arange(17), cfg, "wiener", truth=True)
    e = twin.rel_err(out.spectrum[:], truth)
    print(f"delay after dayenu: e_gpu {e:.3e}")
    conds = []
    for b in range(fv.shape[1]):
        t = twin.cut_data(fv[:, b].T, fw[:, b].T, cfg)
        if t is not None:
            conds.append(np.linalg.cond(twin.wiener_matrix(32, t[1].astype(np.float64), np.arange(17)[t[2]], "nuttall", False, np.fft.fftshift(g["R32/prior"][b]))))
    # float64 throughout from the filtered stream: the forward error of a Cholesky solve, order x cond(G) x 2**-53
    assert conds and e <= 32 * max(conds) * 2.0**-53, (e, conds)


def test_singular_matrix_raises(gold):
    """A zero prior with cut channels leaves G singular: a non-positive pivot sets the status word, no fault."""
    g = gold
    from draco_amd.analysis.delay import DelaySpectrumWienerFilter

    s = _stream(g, "R32")
    task = DelaySpectrumWienerFilter(sample_axis="ra", skip_nyquist=False, apply_window=False)  # (baseline 0 keeps full rank)
    task.setup(_dps(np.zeros_like(g["R32/prior"]), g["R32/delays"]))
    with pytest.raises(np.linalg.LinAlgError, match="baseline 1"):
        task.process(s)
    prior = g["R32/prior"].copy()
    prior[1] = -1e-3  # Si = -1000 on the diagonal: the first pivot is negative
    task.setup(_dps(prior, g["R32/delays"]))
    with pytest.raises(np.linalg.LinAlgError, match="baseline 1"):
        task.process(s)


def test_power_spectrum(gold):
    from draco_amd.analysis.delay import DelaySpectrumToPowerSpectrum
    from draco_amd.core import containers

    g = gold
    _, _, out = _wiener(g, "C48w")
    ps = DelaySpectrumToPowerSpectrum().process(out)
    assert isinstance(ps, containers.DelaySpectrum) and ps.spectrum.on_device and ps.spectrum.dtype == np.float64
    got = ps.spectrum[:]
    # the variance of the reference's own spectrum differs by its e_ref; sums of 6 terms in float64 add a few ulp
    tol = 2 * (3 * float(g["C48w/e_ref"]) + FLOOR) + 16 * 2.0**-52
    assert twin.rel_err(got, g["PS/ref"]) <= tol
    assert np.array_equal(ps.datasets["spectrum_mask"][:], g["PS/ref_mask"]) and not got[2].any()
    assert len(ps.index_map["sample"]) == 1 and np.array_equal(ps.delay, out.delay)
