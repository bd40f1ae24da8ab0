"""Generate tests/golden/nrml.npz by EXECUTING the reference's own ``delay_power_spectrum_maxpost``, ``LogLikePS``,
``GaussianProcessPrior``, ``AddFunctions`` (``draco/analysis/delayopt.py``) and ``DelayPowerSpectrumNRML._evaluate`` /
``_cut_data`` / ``_calculate_delays`` (``draco/analysis/delay.py``) from source, through ``oracle._refstub``,
unmodified, with the scipy that is installed (its ``minimize(method="Newton-CG")`` is the specification).  Only the data
is committed; run where the reference checkout exists:

    python tests/gen_golden_nrml.py

Per case and baseline the file holds the inputs, every iterate (``log S``), the success flag, the masks, and at the
first and the last iterate: value and gradient, the Hessian (exact and Fisher; whole up to 16 delays, rows ``HROWS`` of it
above), the condition number of ``C`` and ``e_ref = rel_err(reference, truth)`` of each quantity, the truth being
``tests/nrml_twin.py`` in long double.  All cases use the task's default ``tol = 1e-3``: below it the reference's own
trajectory is decided by rounding in the line search.

The generator asserts that ``line_search_wolfe2`` is never entered, that no ``|w_f|`` lies within 1e-6 relative of the
pseudo-inverse cut, and that three seeded re-runs in which every value, gradient and Hessian is perturbed at relative
``max(e_ref, 1e-13)`` keep the iteration count.  ``allow`` = 10 x the largest movement of any iterate (in ``log S``) in
those re-runs is printed and stored: it is what an implementation of the same algorithm with other rounding may differ
by (the factor 10 because that movement is itself random: it differs by about a factor of two between seeds).
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

import nrml_twin as twin  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DF = 0.390625
TOL = 1e-3
NSAMP = 60  # the iteration cap of the task cases: above every iteration count here
DEFAULTS = dict(freq_zero=None, freq_spacing=None, nfreq=None, skip_nyquist=True, apply_window=True, window="nuttall", complex_timedomain=False, use_average_weights=True, weight_boost=1.0,
                freq_frac=0.0, time_frac=0.0, remove_mean=True, scale_freq=False, dataset=None, sample_axis="ra", save_spectrum_mask=True, save_samples=True, nsamp=NSAMP, maxpost_tol=TOL)


def hrows(N):
    return np.arange(N) if N <= 16 else np.array([0, 1, N // 2, N - 1])


class Total(float):
    def allreduce(self):
        return self


class Arr(np.ndarray):
    local_array = property(lambda s: s.view(np.ndarray))
    global_shape = property(lambda s: s.shape)
    local_shape = property(lambda s: s.shape)

    def enumerate(self, axis):
        return enumerate(range(self.shape[axis]))

    def sum(self, *a, **k):
        return Total(self.view(np.ndarray).sum(*a, **k))


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
    def __init__(self, nbase, ndelay, nsamp):
        self.datasets = {"spectrum": DS(np.zeros((nbase, ndelay))), "spectrum_samples": DS(np.zeros((nsamp, nbase, ndelay))), "spectrum_mask": DS(np.zeros(nbase, dtype=bool))}

    spectrum = property(lambda s: s.datasets["spectrum"])


REF = types.SimpleNamespace()


def load():
    _refstub.load_reference()
    REF.opt = importlib.import_module("draco.analysis.delayopt")
    REF.dl = importlib.import_module("draco.analysis.delay")
    REF.tools = importlib.import_module("draco.util.tools")
    REF.opt.tools.invert_no_zero = _refstub._invert_no_zero
    REF.dl.tools.invert_no_zero = _refstub._invert_no_zero
    import scipy.optimize._linesearch as ls
    import scipy.optimize._optimize as so

    REF.w2 = [0]
    orig = ls.line_search_wolfe2

    def counted(*a, **k):
        REF.w2[0] += 1
        return orig(*a, **k)

    so.line_search_wolfe2 = counted
    REF.clean = (REF.opt.AddFunctions.value, REF.opt.AddFunctions.gradient, REF.opt.AddFunctions.hessian)


def perturb(eps, seed):
    """Every value, gradient and Hessian of the reference's objective times (1 + eps x normal)."""
    OV, OG, OH = REF.clean
    if eps == 0:
        REF.opt.AddFunctions.value, REF.opt.AddFunctions.gradient, REF.opt.AddFunctions.hessian = OV, OG, OH
        return
    rng = np.random.default_rng(seed)

    def nv(s, x):
        return OV(s, x) * (1 + eps * rng.normal())

    def ng(s, x):
        g = OG(s, x)
        return g * (1 + eps * rng.normal(size=g.shape))

    def nh(s, x):
        h = np.array(OH(s, x))
        n = rng.normal(size=h.shape)
        return h * (1 + eps * (n + n.T) / 2)

    REF.opt.AddFunctions.value, REF.opt.AddFunctions.gradient, REF.opt.AddFunctions.hessian = nv, ng, nh


def ref_functions(data, N, Ni, fsel, window):
    """The reference's objective, set up as ``delay_power_spectrum_maxpost`` sets it up: (exact, Fisher)."""
    opt = REF.opt
    nsamp = data.shape[0]
    F = REF.dl.fourier_matrix(N, fsel).astype(np.complex128)
    data = data.astype(np.complex128)
    w = np.ones(len(fsel))
    if window is not None:
        w = REF.tools.window_generalised(fsel / N, window=window)
        F *= w[:, np.newaxis]
        data = data * w[np.newaxis, :]
    X = (data.T @ data.conj()) / nsamp
    Nm = _refstub._invert_no_zero(Ni)
    F[Ni == 0] = 0.0
    prior = opt.GaussianProcessPrior(N, width=5, alpha=1.0, kernel="matern", nu=1.5)
    return (opt.AddFunctions([opt.LogLikePS(X, F, Nm, nsamp, exact_hessian=True, bounds=(1e-15, 1e10)), prior]),
            opt.AddFunctions([opt.LogLikePS(X, F, Nm, nsamp, exact_hessian=False, bounds=(1e-15, 1e10)), prior]), w, prior.Ci)


def point(out, key, fex, ffi, m, Ci, x):
    """Reference and e_ref of value, gradient, Hessians at ``x``; returns the largest e_ref."""
    N = len(x)
    ref = dict(value=fex.value(x), grad=np.array(fex.gradient(x)), hess=np.array(fex.hessian(x)), fisher=np.array(ffi.hessian(x)))
    tr = twin.evaluate(m, x, Ci, truth=True)
    worst = 0.0
    for q in ("value", "grad", "hess", "fisher"):
        e = twin.rel_err(ref[q], tr[q])
        worst = max(worst, e)
        out[f"{key}/e_{q}"] = np.array(e)
        out[f"{key}/{q}"] = ref[q][hrows(N)] if q in ("hess", "fisher") else ref[q]
    out[f"{key}/x"] = np.array(x)
    out[f"{key}/cond"] = np.array(twin.cond(m, x))
    return worst, {q: float(out[f'{key}/e_{q}']) for q in ("value", "grad", "hess", "fisher")}, float(out[f"{key}/cond"])


def run_baseline(out, key, data, N, Ni, fsel, window, maxiter=NSAMP, expect_fail=False, store_data=True):
    """One baseline through the reference's function: stores inputs, iterates, success, the evaluation points; returns
    the movement of the iterates under perturbation."""
    fsel = np.asarray(fsel)
    perturb(0, 0)
    REF.w2[0] = 0
    samples, ok = REF.opt.delay_power_spectrum_maxpost(data, N, Ni, None, window=window, fsel=fsel, maxiter=maxiter, tol=TOL)
    assert REF.w2[0] == 0, (key, "line_search_wolfe2 was entered")
    xs = np.log(np.array(samples))
    if store_data:
        out.update({f"{key}/data": np.asarray(data, dtype=np.complex128), f"{key}/Ni": np.asarray(Ni, dtype=np.float64)})
    out.update({f"{key}/fsel": fsel, f"{key}/x": xs, f"{key}/success": np.array(bool(ok)),
                f"{key}/N": np.array(N), f"{key}/window": np.array("None" if window is None else window)})
    if expect_fail:
        assert not ok and len(samples) == 1, (key, ok, len(samples))
        print(f"{key}: the reference fails at the first factorisation: success {ok}, {len(samples)} sample")
        return 0.0
    assert ok, key
    fex, ffi, w, Ci = ref_functions(np.asarray(data), N, np.asarray(Ni), fsel, window)
    live = np.abs(w[np.asarray(Ni) != 0])
    cut = 1e-3 * live.max()
    assert not np.any(np.abs(live / cut - 1) < 1e-6), (key, "a window coefficient lies at the pseudo-inverse cut")
    mt = twin.model(data, N, Ni, fsel, window, truth=True)
    e_s0 = twin.rel_err(samples[0], mt["S0"].astype(np.float64))
    out[f"{key}/e_S0"] = np.array(e_s0)
    worst = 0.0
    msg = []
    for tag, x in (("first", xs[0]), ("last", xs[-1])):
        e, each, kappa = point(out, f"{key}/{tag}", fex, ffi, mt, Ci, x)
        worst = max(worst, e)
        msg.append(f"{tag}: " + " ".join(f"{q} {v:.1e}" for q, v in each.items()) + f" cond {kappa:.1e}")
    eps = max(worst, 1e-13)
    move = 0.0
    for seed in (1, 2, 3):
        perturb(eps, seed)
        s2, ok2 = REF.opt.delay_power_spectrum_maxpost(data, N, Ni, None, window=window, fsel=fsel, maxiter=maxiter, tol=TOL)
        assert ok2 and len(s2) == len(samples), (key, "the iteration count changed under perturbation", len(s2), len(samples))
        move = max(move, float(np.abs(np.log(np.array(s2)) - xs).max()))
    perturb(0, 0)
    out[f"{key}/move"] = np.array(move)
    print(f"{key}: N {N} chan {len(fsel)} ns {data.shape[0]} iters {len(samples) - 1} e_S0 {e_s0:.1e} | " + " | ".join(msg) + f" | eps {eps:.1e} move {move:.2e}")
    return move


def make_task(**cfg):
    t = REF.dl.DelayPowerSpectrumNRML()
    t.log = logging.getLogger("gen")
    for k, v in {**DEFAULTS, **cfg}.items():
        setattr(t, k, v)
    return t


def run_task(out, name, freq, dview, wview, store, expect_fail=(), **cfg):
    """A task case: every baseline through ``run_baseline``, then the reference's ``_evaluate`` on the whole."""
    task = make_task(**cfg)
    delays, channel_ind = task._calculate_delays([FakeFreq(freq)])
    ndelay = len(delays)
    nbase = dview.shape[0]
    window = task.window if task.apply_window else None
    move = 0.0
    skipped = []
    for b in range(nbase):
        t = task._cut_data(np.array(dview[b]), np.array(wview[b]))
        if t is None:
            skipped.append(b)
            continue
        data, weight, nzf, _ = t
        move = max(move, run_baseline(out, f"{name}/b{b}", np.array(data), ndelay, np.array(weight, dtype=np.float64), channel_ind[nzf], window, expect_fail=b in expect_fail, store_data=False))
        out[f"{name}/b{b}/nzf"] = np.array(nzf)
    oc = FakeOut(nbase, ndelay, task.nsamp)
    dv, wv = types.SimpleNamespace(local_array=np.array(dview)), types.SimpleNamespace(local_array=np.array(wview))
    task._evaluate(dv, wv, oc, delays, channel_ind)
    out.update({f"{name}/spectrum": np.array(oc.spectrum[:]), f"{name}/spectrum_samples": np.array(oc.datasets["spectrum_samples"][:]), f"{name}/spectrum_mask": np.array(oc.datasets["spectrum_mask"][:]),
                f"{name}/delays": delays, f"{name}/channel_ind": channel_ind, f"{name}/skipped": np.array(skipped, dtype=np.int64), f"{name}/nbase": np.array(nbase)})
    for b in range(nbase):  # the task's rows are the function's iterates
        if b not in skipped:
            xs = out[f"{name}/b{b}/x"]
            assert np.allclose(out[f"{name}/spectrum"][b], np.fft.fftshift(np.exp(xs[-1])), rtol=1e-13, atol=0)
            assert np.allclose(out[f"{name}/spectrum_samples"][-len(xs):, b], np.exp(xs), rtol=1e-13, atol=0)
    out.update({f"{name}/{k}": v for k, v in store.items()})
    print(f"{name}: ndelay {ndelay} baselines {nbase} skipped {skipped} mask {out[f'{name}/spectrum_mask'].astype(int).tolist()}")
    return move


def sky(rng, chan, N, ns, noise, decades=4.0, amp=100.0):
    """``[ns, len(chan)]`` complex128 samples of a delay spectrum that falls ``decades`` from zero delay, plus noise."""
    tau = np.abs(np.fft.fftfreq(N)) * 2
    S = amp * 10.0 ** (-decades * tau**0.8) + 1e-3
    E = np.exp(-2j * np.pi * ((np.asarray(chan)[:, None] * np.arange(N)[None, :]) % N) / N)
    d = (rng.normal(size=(ns, N)) + 1j * rng.normal(size=(ns, N))) * np.sqrt(S / 2)
    return d @ E.T + noise * (rng.normal(size=(ns, len(chan))) + 1j * rng.normal(size=(ns, len(chan)))) / np.sqrt(2)


def stream(rng, chan, N, nstack, nra, noise, **kw):
    """vis ``[freq, stack, ra]`` complex128 and weight float64 (the inverse noise variance, uneven over the band)."""
    vis = np.stack([sky(rng, chan, N, nra, noise, **kw) for _ in range(nstack)]).transpose(2, 0, 1).copy()
    weight = np.repeat((rng.uniform(0.8, 1.25, size=(len(chan), nstack)) / noise**2)[:, :, None], nra, axis=2)
    return vis, weight


def sview(a):
    return a.transpose(1, 2, 0)  # [freq, stack, ra] -> [stack, ra, freq]


def main():
    load()
    out = {}
    moves = {}

    # ---- N16: 8 channels with one cut, below one tile
    rng = np.random.default_rng(16001)
    freq = 400.0 + DF * np.arange(8)
    vis, weight = stream(rng, np.arange(8), 16, 1, 12, 0.1)
    weight[3] = 0.0
    moves["N16"] = run_task(out, "N16", freq, sview(vis), sview(weight), dict(freq=freq, vis=vis, weight=weight))

    # ---- N32: three baselines; three channels cut on one, one sample without weight, one baseline fully flagged
    rng = np.random.default_rng(32002)
    freq = 400.0 + DF * np.arange(16)
    vis, weight = stream(rng, np.arange(16), 32, 3, 24, 0.1)
    weight[[3, 4, 9], 1, :] = 0.0
    weight[:, 1, 2] = 0.0
    weight[:, 2, :] = 0.0
    moves["N32"] = run_task(out, "N32", freq, sview(vis), sview(weight), dict(freq=freq, vis=vis, weight=weight))

    # ---- C23: complex time domain, 23 channels, odd N, no window
    rng = np.random.default_rng(23003)
    freq = 600.0 + DF * np.arange(23)
    vis, weight = stream(rng, np.arange(23), 23, 2, 20, 0.3, decades=3.0)
    weight[[5, 6], 1, :] = 0.0
    moves["C23"] = run_task(out, "C23", freq, sview(vis), sview(weight), dict(freq=freq, vis=vis, weight=weight), complex_timedomain=True, apply_window=False)

    # ---- N70: channel_ind starts above 0, freq_frac cuts a weighted channel, ndelay no multiple of 16
    rng = np.random.default_rng(70004)
    freq = 600.0 + DF * np.arange(5, 35)
    vis, weight = stream(rng, np.arange(5, 35), 70, 2, 10, 0.1)
    weight[7, 0, 3:] = 0.0  # 3 of 10 samples: 0.3 is not above 0.3, the channel is cut although its average weight is not zero
    weight[12, 0, 4:] = 0.0  # 4 of 10: retained
    weight[20, 1, :] = 0.0
    cfg = dict(freq_zero=600.0, freq_spacing=DF, freq_frac=0.3)
    moves["N70"] = run_task(out, "N70", freq, sview(vis), sview(weight), dict(freq=freq, vis=vis, weight=weight), **cfg)
    assert not out["N70/b0/nzf"][7] and out["N70/b0/nzf"][12] and weight[7, 0].mean() > 0

    # ---- N80hann: the window is exactly zero at channel 0
    rng = np.random.default_rng(80005)
    freq = 400.0 + DF * np.arange(40)
    vis, weight = stream(rng, np.arange(40), 80, 1, 30, 0.1)
    assert REF.tools.window_generalised(np.arange(40) / 80, window="hann")[0] == 0.0
    moves["N80hann"] = run_task(out, "N80hann", freq, sview(vis), sview(weight), dict(freq=freq, vis=vis, weight=weight), window="hann")

    # ---- RM32: a float64 ring map [1 beam, 2 pol, 17 freq, 6 ra, 5 el]; baseline = beam x pol x el
    rng = np.random.default_rng(17026)
    freq = 400.0 + DF * np.arange(17)
    rmap = np.stack([sky(rng, np.arange(17), 32, 6, 1.0, decades=1.0).real * np.sqrt(2) for _ in range(10)]).reshape(1, 2, 5, 6, 17).transpose(0, 1, 4, 3, 2).copy()
    rw = np.repeat(rng.uniform(0.8, 1.25, size=(2, 17, 1, 5)), 6, axis=2)
    rw[0, [6, 7], :, 1] = 0.0
    rw[1, 3, 2, 4] = 0.0
    rw[1, :, :, 2] = 0.0  # a fully flagged (pol, el) column
    dview = rmap.transpose(0, 1, 4, 3, 2).reshape(10, 6, 17)
    wview = np.broadcast_to(rw[np.newaxis], rmap.shape).transpose(0, 1, 4, 3, 2).reshape(10, 6, 17)
    moves["RM32"] = run_task(out, "RM32", freq, dview, wview, dict(freq=freq, map=rmap, weight=rw), skip_nyquist=False, dataset="map")

    # ---- N160: one baseline, crosses the 64 and 128 tile edges
    rng = np.random.default_rng(160007)
    freq = 400.0 + DF * np.arange(80)
    vis, weight = stream(rng, np.arange(80), 160, 1, 48, 0.1)
    weight[[10, 11, 50]] = 0.0
    moves["N160"] = run_task(out, "N160", freq, sview(vis), sview(weight), dict(freq=freq, vis=vis, weight=weight))

    # ---- NEG: weight_boost = -1 with strong noise: the first factorisation fails
    rng = np.random.default_rng(16008)
    freq = 400.0 + DF * np.arange(8)
    vis, weight = stream(rng, np.arange(8), 16, 1, 12, 100.0)
    run_task(out, "NEG", freq, sview(vis), sview(weight), dict(freq=freq, vis=vis, weight=weight), expect_fail=(0,), weight_boost=-1.0)
    assert out["NEG/spectrum_mask"].tolist() == [True]

    # ---- evaluation only: 130 channels / 272 delays at two points
    rng = np.random.default_rng(272009)
    fsel = np.delete(np.arange(136), [20, 21, 22, 70, 100, 101])
    data = sky(rng, fsel, 272, 40, 0.1)
    Ni = rng.uniform(0.8, 1.25, size=130) / 0.1**2
    fex, ffi, w, Ci = ref_functions(data, 272, Ni, fsel, "nuttall")
    mt = twin.model(data, 272, Ni, fsel, "nuttall", truth=True)
    x0 = np.log((data * w @ np.linalg.pinv((REF.dl.fourier_matrix(272, fsel) * w[:, None]).T, rcond=1e-3)).var(axis=0))
    pts = [x0, x0 + 0.5 * np.cos(2 * np.pi * np.arange(272) / 272) - 0.3]
    out.update({"EVAL/b0/data": data, "EVAL/b0/Ni": Ni, "EVAL/b0/fsel": fsel, "EVAL/b0/N": np.array(272), "EVAL/b0/window": np.array("nuttall")})
    out["EVAL/b0/e_S0"] = np.array(twin.rel_err(np.exp(x0), mt["S0"].astype(np.float64)))
    for tag, x in zip(("first", "last"), pts):
        e, each, kappa = point(out, f"EVAL/b0/{tag}", fex, ffi, mt, Ci, x)
        print(f"EVAL {tag}: " + " ".join(f"{q} {v:.1e}" for q, v in each.items()) + f" cond {kappa:.1e} e_S0 {float(out['EVAL/b0/e_S0']):.1e}")

    allow = 10 * max(moves.values())
    out["allow"] = np.array(allow)
    print("movement per case:", {k: f"{v:.2e}" for k, v in moves.items()}, "-> allow", f"{allow:.3e}")
    path = os.path.join(GOLDEN, "nrml.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
