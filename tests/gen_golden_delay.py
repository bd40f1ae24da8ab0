"""Generate tests/golden/delay.npz and tests/golden/delay_r1100.npz by EXECUTING the reference's own
``delay_spectrum_wiener_filter``, ``delay_spectrum_fft``, ``_calculate_delays``, ``_cut_data``,
``DelaySpectrumBase._evaluate`` (through ``DelaySpectrumWienerFilter`` / ``DelaySpectrumFFT``),
``DelaySpectrumToPowerSpectrum.process``, the Fourier-matrix functions and ``window_generalised`` from source (through
``oracle._refstub``, unmodified; what its stubs lack -- ``invert_no_zero``, ``fft.fftw.ifft``, the container classes --
is patched on the imported module at run time).  Only the data is committed; run where the reference checkout exists:

    python tests/gen_golden_delay.py

Per case the files hold the inputs, the reference's output, the truth (``tests/delay_twin.py``, long double
throughout, rounded once) and ``e_ref = rel_err(reference, truth)``.  The priors are smooth delay power spectra that
fall three to five decades from zero delay onto a floor, scaled so that the condition number of every Wiener matrix
lies between 1e3 and 1e7 (printed, stored and asserted).  Where the inputs are float64 (the ring maps RM, RM70, RM1100
and the functions) that keeps ``e_ref`` set by the conditioning; on the streams (complex64 data, float32 weights) the
reference takes its means in single precision and ``e_ref`` is about 5e-8 whatever the conditioning.  The generator
asserts that the reference factorises every baseline it does not skip (it raises otherwise).
"""

import importlib
import logging
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import delay_twin as twin  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DF = 0.390625
WINDOW_NAMES = ["uniform", "hann", "hanning", "hamming", "blackman", "nuttall", "blackman_nuttall", "blackman_harris", "triangular", "tukey-0.5", "tukey-0.2"]
DEFAULTS = dict(freq_zero=None, freq_spacing=None, nfreq=None, skip_nyquist=True, apply_window=True, window="nuttall", complex_timedomain=False, use_average_weights=True, weight_boost=1.0,
                freq_frac=0.0, time_frac=0.0, remove_mean=True, scale_freq=False, dataset=None, sample_axis="ra", save_spectrum_mask=False)


class Arr(np.ndarray):
    """ndarray with the few MPIArray attributes the tasks touch."""

    local_array = property(lambda s: s.view(np.ndarray))
    global_shape = property(lambda s: s.shape)
    local_shape = property(lambda s: s.shape)

    def enumerate(self, axis):
        return enumerate(range(self.shape[axis]))


class DS:
    def __init__(self, arr):
        self.arr = np.asarray(arr).view(Arr)

    def __getitem__(self, k):
        return self.arr[k]

    def __setitem__(self, k, v):
        self.arr[k] = v

    global_shape = property(lambda s: s.arr.shape)
    local_shape = property(lambda s: s.arr.shape)


class FakeFreq:
    def __init__(self, freq):
        self.freq = np.asarray(freq)


class FakeOut:
    def __init__(self, shape, dtype, mask_shape=None):
        self.datasets = {"spectrum": DS(np.zeros(shape, dtype=dtype))}
        self._mask_shape = mask_shape
        self.attrs = {}

    spectrum = property(lambda s: s.datasets["spectrum"])

    def add_dataset(self, name):
        self.datasets[name] = DS(np.zeros(self._mask_shape, dtype=bool))

    def redistribute(self, axis):
        pass


def make_task(cls, **cfg):
    t = cls()
    t.log = logging.getLogger("gen")
    for k, v in {**DEFAULTS, **cfg}.items():
        setattr(t, k, v)
    return t


def prior_rows(nbase, ndelay, rng, decades, amp, floor):
    """A smooth delay power spectrum per baseline in the task's (fftshift) order."""
    tau = np.abs(np.arange(ndelay) - ndelay // 2) / (ndelay / 2)
    return np.stack([amp * rng.uniform(0.8, 1.25) * 10.0 ** (-decades * tau ** rng.uniform(0.7, 1.0)) + floor for _ in range(nbase)])


def run_case(mod, out, name, cls, freq, dview, wview, prior, store_inputs, prefix_inputs=True, **cfg):
    """``dview`` / ``wview``: [baseline, sample, freq] views of the container's datasets."""
    task = make_task(cls, **cfg)
    delays, channel_ind = task._calculate_delays([FakeFreq(freq)])
    ndelay = len(delays)
    nbase, nsample = dview.shape[:2]
    oc = FakeOut((nbase, nsample, ndelay), np.complex128, (nbase, nsample))
    if task.save_spectrum_mask:
        oc.add_dataset("spectrum_mask")
    if prior is not None:
        task.dps = types.SimpleNamespace(spectrum=DS(prior))
    dv, wv = types.SimpleNamespace(local_array=np.array(dview)), types.SimpleNamespace(local_array=np.array(wview))
    task._evaluate(dv, wv, oc, delays, channel_ind)  # raises if the reference cannot factorise a baseline
    ref = np.array(oc.spectrum[:])
    tcfg = dict(time_frac=task.time_frac, freq_frac=task.freq_frac, remove_mean=task.remove_mean, weight_boost=task.weight_boost, window=task.window if task.apply_window else None,
                complex_timedomain=task.complex_timedomain)
    est = "wiener" if prior is not None else "fft"
    truth, tmask = twin.evaluate(np.array(dview), np.array(wview), prior, ndelay, channel_ind, tcfg, est, truth=True)
    e_ref = twin.rel_err(ref, truth)
    conds = []
    if prior is not None:
        for bi in range(nbase):
            t = task._cut_data(np.array(dview[bi]), np.array(wview[bi]))
            if t is None:
                continue
            _, wt, nzf, _ = t
            G = twin.wiener_matrix(ndelay, wt.astype(np.float64), channel_ind[nzf], tcfg["window"], task.complex_timedomain, np.fft.fftshift(prior[bi]))
            conds.append(np.linalg.cond(G))
        assert all(1e3 <= c <= 1e7 for c in conds), (name, conds)
    print(f"{name}: ndelay {ndelay} channel_ind {channel_ind[0]}..{channel_ind[-1]} e_ref {e_ref:.3e} cond {['%.2e' % c for c in conds]} skipped {int(tmask.all(axis=1).sum())}")
    blob = dict(ref=ref, truth=truth, e_ref=np.array(e_ref), delays=delays, channel_ind=channel_ind, cond=np.array(conds))
    if task.save_spectrum_mask:
        blob["ref_mask"] = np.array(oc.datasets["spectrum_mask"][:])
        assert np.array_equal(blob["ref_mask"], tmask)
    if prior is not None:
        blob["prior"] = prior
    blob.update(store_inputs)
    for k, v in blob.items():
        out[f"{name}/{k}"] = v
    return ref, blob.get("ref_mask")


def stream(rng, nfreq, nstack, nra, amp=1.0):
    vis = (amp * (rng.normal(size=(nfreq, nstack, nra)) + 1j * rng.normal(size=(nfreq, nstack, nra)))).astype(np.complex64)
    weight = rng.uniform(0.5, 1.5, size=(nfreq, nstack, nra)).astype(np.float32)
    return vis, weight


def sview(a):
    return a.transpose(1, 2, 0)  # [freq, stack, ra] -> [stack, ra, freq]


def main():
    _refstub.load_reference()
    mod = importlib.import_module("draco.analysis.delay")
    mod.tools.invert_no_zero = _refstub._invert_no_zero
    mod.fft = types.SimpleNamespace(fftw=types.SimpleNamespace(ifft=lambda x, axes=-1: np.fft.ifft(x, axis=axes)))
    ref_tools = importlib.import_module("draco.util.tools")
    W, F = mod.DelaySpectrumWienerFilter, mod.DelaySpectrumFFT
    out, big = {}, {}

    # ---- R32: real, order below one tile, both strictly-real channels present
    rng = np.random.default_rng(32001)
    freq = 400.0 + DF * np.arange(17)
    vis, weight = stream(rng, 17, 3, 5)
    weight[[3, 4, 9], 1, :] = 0.0
    weight[:, 1, 2] = 0.0  # a sample without any weight: nzt drops it
    weight[:, 2, :] = 0.0  # skipped
    prior = prior_rows(3, 32, rng, 4.0, 1000.0, 3e-3)
    run_case(mod, out, "R32", W, freq, sview(vis), sview(weight), prior, dict(freq=freq, vis=vis, weight=weight), skip_nyquist=False, save_spectrum_mask=True)

    # ---- R70: order no multiple of 16, channel_ind starts above 0, freq_frac cuts a weighted channel
    rng = np.random.default_rng(70002)
    freq = 600.0 + DF * np.arange(5, 35)
    vis, weight = stream(rng, 30, 2, 10)
    weight[7, 0, 3:] = 0.0  # 3 of 10 samples: 0.3 is not above 0.3, the channel is cut although its average weight is not zero
    weight[12, 0, 4:] = 0.0  # 4 of 10: retained
    weight[20, 1, :] = 0.0
    prior = prior_rows(2, 70, rng, 3.0, 1000.0, 3e-3)
    cfg = dict(skip_nyquist=True, freq_zero=600.0, freq_spacing=DF, freq_frac=0.3)
    run_case(mod, out, "R70", W, freq, sview(vis), sview(weight), prior, dict(freq=freq, vis=vis, weight=weight), **cfg)
    t = make_task(W, **cfg)._cut_data(np.array(sview(vis)[0]), np.array(sview(weight)[0]))
    assert not t[2][7] and t[2][12] and weight[7, 0].mean() > 0
    out["R70/nzf0"] = t[2]

    # ---- C46: complex, odd length (the task's second fftshift is not the inverse of its first), two priors
    rng = np.random.default_rng(46003)
    freq = 600.0 + DF * np.arange(23)
    vis, weight = stream(rng, 23, 2, 4)
    weight[[5, 6], 1, :] = 0.0
    p1 = prior_rows(2, 23, rng, 4.0, 1000.0, 3e-3)
    p2 = prior_rows(2, 23, rng, 3.0, 300.0, 1e-2)
    cfg = dict(complex_timedomain=True, remove_mean=False)
    run_case(mod, out, "C46", W, freq, sview(vis), sview(weight), p1, dict(freq=freq, vis=vis, weight=weight), **cfg)
    run_case(mod, out, "C46b", W, freq, sview(vis), sview(weight), p2, {}, **cfg)

    # ---- C48w: complex, weight_boost, another window, no window, the mask dataset, two identical baselines
    rng = np.random.default_rng(48004)
    freq = 600.0 + DF * np.arange(24)
    vis, weight = stream(rng, 24, 4, 6)
    weight[[2, 11, 12], 1, :] = 0.0
    weight[:, 1, 4] = 0.0
    weight[:, 2, :] = 0.0
    vis[:, 3], weight[:, 3] = vis[:, 0], weight[:, 0]
    prior = prior_rows(4, 24, rng, 5.0, 0.1, 1e-6)
    prior[3] = prior[0]
    cfg = dict(complex_timedomain=True, weight_boost=4.0, window="blackman_harris", save_spectrum_mask=True)
    ref, rmask = run_case(mod, out, "C48w", W, freq, sview(vis), sview(weight), prior, dict(freq=freq, vis=vis, weight=weight), **cfg)
    run_case(mod, out, "C48n", W, freq, sview(vis), sview(weight), prior, {}, apply_window=False, **cfg)

    # ---- PS: DelaySpectrumToPowerSpectrum on C48w's output and mask (baseline 2 is masked throughout)
    mod.containers = types.SimpleNamespace(FreqContainer=FakeFreq, DelaySpectrum=lambda attrs_from=None, axes_from=None: FakeOut(ref.shape[::2], np.float64, (ref.shape[0],)))
    dspec = FakeOut(ref.shape, np.complex128, rmask.shape)
    dspec.spectrum[:] = ref
    dspec.add_dataset("spectrum_mask")
    dspec.datasets["spectrum_mask"][:] = rmask
    with np.errstate(invalid="ignore", divide="ignore"):
        ps = mod.DelaySpectrumToPowerSpectrum().process(dspec)
    out["PS/ref"], out["PS/ref_mask"] = np.array(ps.spectrum[:]), np.array(ps.datasets["spectrum_mask"][:])
    assert out["PS/ref_mask"].tolist() == [False, False, True, False] and not out["PS/ref"][2].any()
    tps, tfl = twin.power_spectrum(ref, rmask)
    assert np.array_equal(tps, out["PS/ref"]) and np.array_equal(tfl, out["PS/ref_mask"])

    # ---- FFT estimator: 24 and 23 channels, with and without a window; a cut channel makes the reference raise
    for nf in (24, 23):
        rng = np.random.default_rng(9000 + nf)
        freq = 600.0 + DF * np.arange(nf)
        vis, weight = stream(rng, nf, 3, 5)
        weight[:, 1, 3] = 0.0
        weight[:, 2, :] = 0.0
        for tag, aw in (("w", True), ("n", False)):
            run_case(mod, out, f"FFT{nf}{tag}", F, freq, sview(vis), sview(weight), None, dict(freq=freq, vis=vis, weight=weight) if aw else {}, complex_timedomain=True, apply_window=aw, save_spectrum_mask=True)
    wcut = weight.copy()
    wcut[4, 0, :] = 0.0
    try:
        run_case(mod, {}, "FFTcut", F, freq, sview(vis), sview(wcut), None, {}, complex_timedomain=True)
        raise RuntimeError("the reference did not raise on a cut channel")
    except ValueError as e:
        print("FFT with a cut channel: the reference raises ValueError:", str(e)[:60])
    out["FFTcut/weight"] = wcut

    # ---- ring map [1 beam, 2 pol, 17 freq, 6 ra, 5 el] float64; baseline = beam x pol x el
    rng = np.random.default_rng(17005)
    freq = 400.0 + DF * np.arange(17)
    rmap = rng.normal(size=(1, 2, 17, 6, 5))
    rw = rng.uniform(0.5, 1.5, size=(2, 17, 6, 5))
    rw[0, [6, 7], :, 1] = 0.0
    rw[1, 3, 2, 4] = 0.0
    rw[1, :, :, 2] = 0.0  # a fully flagged (pol, el) column
    dview = rmap.transpose(0, 1, 4, 3, 2).reshape(10, 6, 17)
    wview = np.broadcast_to(rw[np.newaxis], rmap.shape).transpose(0, 1, 4, 3, 2).reshape(10, 6, 17)
    prior = prior_rows(10, 32, rng, 4.0, 1000.0, 3e-3)
    run_case(mod, out, "RM", W, freq, dview, wview, prior, dict(freq=freq, map=rmap, weight=rw), skip_nyquist=False, dataset="map", save_spectrum_mask=True)

    # ---- R1100: real, order just above 1024, twenty channels cut in two stretches
    rng = np.random.default_rng(110006)
    freq = 400.0 + DF * np.arange(551)
    vis, weight = stream(rng, 551, 2, 3)
    weight[100:112, 0, :] = 0.0
    weight[300:308, 0, :] = 0.0
    weight[40:52, 1, :] = 0.0
    weight[500:508, 1, :] = 0.0
    prior = prior_rows(2, 1100, rng, 4.0, 1000.0, 3e-3)
    run_case(mod, big, "R1100", W, freq, sview(vis), sview(weight), prior, dict(freq=freq, vis=vis, weight=weight), skip_nyquist=False)

    # ---- float64 inputs at the orders of R70 and R1100: ring maps [1 beam, 1 pol, freq, ra, el], where e_ref is set by the
    # conditioning alone (the stream cases carry the reference's single-precision means, e_ref about 5e-8)
    rng = np.random.default_rng(70008)
    freq = 600.0 + DF * np.arange(5, 35)
    rmap = rng.normal(size=(1, 1, 30, 10, 3))
    rw = rng.uniform(0.5, 1.5, size=(1, 30, 10, 3))
    rw[0, 7, 3:, 0] = 0.0  # 3 of 10 samples: cut by freq_frac = 0.3
    rw[0, 12, 4:, 0] = 0.0
    rw[0, 20, :, 1] = 0.0
    rw[0, :, 6, 2] = 0.0  # a dropped sample
    dview, wview = rmap[0, 0].transpose(2, 1, 0), rw[0].transpose(2, 1, 0)
    prior = prior_rows(3, 70, rng, 3.0, 1000.0, 3e-3)
    run_case(mod, out, "RM70", W, freq, dview, wview, prior, dict(freq=freq, map=rmap, weight=rw), skip_nyquist=True, freq_zero=600.0, freq_spacing=DF, freq_frac=0.3, dataset="map",
             save_spectrum_mask=True)
    rng = np.random.default_rng(110009)
    freq = 400.0 + DF * np.arange(551)
    rmap = rng.normal(size=(1, 1, 551, 3, 2))
    rw = rng.uniform(0.5, 1.5, size=(1, 551, 3, 2))
    rw[0, 100:112, :, 0] = 0.0
    rw[0, 300:308, :, 0] = 0.0
    rw[0, 40:52, :, 1] = 0.0
    rw[0, 500:508, :, 1] = 0.0
    dview, wview = rmap[0, 0].transpose(2, 1, 0), rw[0].transpose(2, 1, 0)
    prior = prior_rows(2, 1100, rng, 4.0, 1000.0, 3e-3)
    run_case(mod, big, "RM1100", W, freq, dview, wview, prior, dict(freq=freq, map=rmap, weight=rw), skip_nyquist=False, dataset="map")

    # ---- the two functions
    rng = np.random.default_rng(5007)
    fsel = np.delete(np.arange(17), [3, 4, 9])
    data = (rng.normal(size=(4, fsel.size)) + 1j * rng.normal(size=(4, fsel.size)))
    Ni = rng.uniform(0.5, 1.5, size=fsel.size)
    ps = np.fft.fftshift(prior_rows(1, 32, rng, 4.0, 1000.0, 3e-3)[0])
    r = mod.delay_spectrum_wiener_filter(ps, data.copy(), 32, Ni, window="nuttall", fsel=fsel, complex_timedomain=False)
    tr = twin.wiener(ps, data, 32, Ni, "nuttall", fsel, False, truth=True).astype(np.float64)
    out.update({"fn_wr/ps": ps, "fn_wr/data": data, "fn_wr/Ni": Ni, "fn_wr/fsel": fsel, "fn_wr/ref": r, "fn_wr/truth": tr, "fn_wr/e_ref": np.array(twin.rel_err(r, tr))})
    data = (rng.normal(size=(3, 23)) + 1j * rng.normal(size=(3, 23)))
    Ni = rng.uniform(0.5, 1.5, size=23)
    Ni[[7, 8]] = 0.0
    ps = np.fft.fftshift(prior_rows(1, 23, rng, 4.0, 1000.0, 3e-3)[0])
    r = mod.delay_spectrum_wiener_filter(ps, data.copy(), 23, Ni, window=None, fsel=None, complex_timedomain=True)
    tr = twin.wiener(ps, data, 23, Ni, None, None, True, truth=True).astype(np.complex128)
    out.update({"fn_wc/ps": ps, "fn_wc/data": data, "fn_wc/Ni": Ni, "fn_wc/ref": r, "fn_wc/truth": tr, "fn_wc/e_ref": np.array(twin.rel_err(r, tr))})
    r = mod.delay_spectrum_fft(data.copy(), 23, window="nuttall")
    tr = twin.fft_estimate(data, 23, "nuttall", truth=True).astype(np.complex128)
    out.update({"fn_fft/data": data, "fn_fft/ref": r, "fn_fft/truth": tr, "fn_fft/e_ref": np.array(twin.rel_err(r, tr))})
    data = (rng.normal(size=(3, 47)) + 1j * rng.normal(size=(3, 47)))  # complex, order 94: more than one tile
    Ni = rng.uniform(0.5, 1.5, size=47)
    Ni[[7, 8, 30]] = 0.0
    ps = np.fft.fftshift(prior_rows(1, 47, rng, 4.0, 1000.0, 3e-3)[0])
    r = mod.delay_spectrum_wiener_filter(ps, data.copy(), 47, Ni, window="blackman", fsel=None, complex_timedomain=True)
    tr = twin.wiener(ps, data, 47, Ni, "blackman", None, True, truth=True).astype(np.complex128)
    out.update({"fn_wc94/ps": ps, "fn_wc94/data": data, "fn_wc94/Ni": Ni, "fn_wc94/ref": r, "fn_wc94/truth": tr, "fn_wc94/e_ref": np.array(twin.rel_err(r, tr))})
    print("functions: e_ref", float(out["fn_wr/e_ref"]), float(out["fn_wc/e_ref"]), float(out["fn_fft/e_ref"]), float(out["fn_wc94/e_ref"]))

    # ---- window_generalised on a grid that leaves [0, 1], the four Fourier-matrix functions
    x = np.concatenate([[-0.25, -1e-9], np.linspace(0.0, 1.0, 41), [1.0 + 1e-9, 1.5]])
    out["win/x"] = x
    out["win/names"] = np.array(WINDOW_NAMES)
    out["win/ref"] = np.stack([ref_tools.window_generalised(x, window=w) for w in WINDOW_NAMES])
    fsel = np.array([0, 1, 2, 5, 8])
    for nm, fn in (("r2c", mod.fourier_matrix_r2c), ("c2r", mod.fourier_matrix_c2r), ("c2c", mod.fourier_matrix_c2c), ("c", mod.fourier_matrix)):
        out[f"fm/{nm}_all"] = fn(16)
        out[f"fm/{nm}_sel"] = fn(16, fsel)
    out["fm/c2c_odd"] = mod.fourier_matrix_c2c(7)
    out["fm/fsel"] = fsel

    for fname, blob in (("delay.npz", out), ("delay_r1100.npz", big)):
        path = os.path.join(GOLDEN, fname)
        np.savez_compressed(path, **blob)
        print(path, os.path.getsize(path))
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
