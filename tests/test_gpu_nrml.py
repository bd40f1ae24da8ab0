"""NRML delay power spectrum estimator on the GPU against tests/golden/nrml.npz (the reference executed from source by
gen_golden_nrml.py) and the long-double truth of tests/nrml_twin.py, which is computed here once per case.

* Evaluation: value, gradient, exact and Fisher Hessian and the starting spectrum at every stored point against the
  truth: ``rel_err <= max(2 e_ref, 4 kappa(C) 2^-53)``, ``e_ref`` the reference's own error and the second term the
  forward-error scale of a backward-stable Cholesky solve.  The task cases go through the prepare pass and
  ``dmm_nrml_start``; the 130-channel / 272-delay case through host arrays.
* Direction: the device's conjugate gradient against the NumPy rule: same pass count, 1e-12 relative.
* Function and task: same number of samples, same success, every iterate within ``allow`` in ``log S``.
"""

import ctypes as C

import numpy as np
import pytest

import nrml_cases as cases
import nrml_twin as twin

pytestmark = pytest.mark.gpu

U53 = 2.0**-53
QUANT = ("value", "grad", "hess", "fisher")


@pytest.fixture(scope="module")
def z():
    return cases.load()


_TRUTH = {}


def truth_of(z, name):
    """Per baseline: the long-double model and the truth at the stored points (computed once)."""
    if name not in _TRUTH:
        out = {}
        for b, data, Ni, fsel, N, win in cases.baselines(z, name, truth=True):
            m = twin.model(data, N, Ni, fsel, win, truth=True)
            Ci = twin.matern_inverse(N)
            out[b] = dict(S0=m["S0"].astype(np.float64), N=N, **{pt: twin.evaluate(m, z[f"{name}/b{b}/{pt}/x"], Ci, truth=True) for pt in cases.POINTS})
        _TRUTH[name] = out
    return _TRUTH[name]


def container(z, name):
    from draco_amd.core import containers
    from draco_amd.device import Context

    ctx = Context.get()
    if f"{name}/map" in z.files:
        rmap, rw = z[f"{name}/map"], z[f"{name}/weight"]
        nb, npol, nfreq, nra, nel = rmap.shape
        c = containers.RingMap(freq=z[f"{name}/freq"], beam=nb, pol=np.array(["XX", "YY"])[:npol], ra=nra, el=np.linspace(-1, 1, nel), allocate=False)
        c.attach("map", ctx.to_device(rmap))
        c.attach("weight", ctx.to_device(rw))
        return c
    vis, weight = z[f"{name}/vis"], z[f"{name}/weight"]
    c = containers.SiderealStream(freq=z[f"{name}/freq"], ra=vis.shape[2], stack=vis.shape[1], allocate=False)
    # (double-precision datasets, so that the reference's own error is set by the conditioning: `attach` would hold them
    # to the container's complex64 / float32)
    for ds, arr in (("vis", vis), ("vis_weight", weight)):
        c.datasets[ds] = containers.Dataset(dev=ctx.to_device(arr), attrs={"axis": c._dataset_spec[ds]["axes"]})
    return c


def make_task(name, **over):
    from draco_amd.analysis.delay import DelayPowerSpectrumNRML

    return DelayPowerSpectrumNRML(**{**dict(sample_axis="ra", nsamp=60, save_samples=True, save_spectrum_mask=True), **cases.CFG[name], **over})


def evaluator(z, name):
    """One evaluator over all baselines of a case, built as the task builds it."""
    from draco_amd.analysis import delay, delayopt
    from draco_amd.device import Context

    ctx = Context.get()
    if name == "EVAL":
        _, data, Ni, fsel, N, win = next(cases.baselines(z, name))
        X, MF, Nm, nsamp, S0 = delayopt._model_host(data, N, Ni, win, fsel)
        ev = delayopt.DeviceEvaluator.from_arrays(ctx, N, fsel, MF[:, 0].real, Nm, X, [nsamp])
        return ev, None
    task = make_task(name)
    ss = container(z, name)
    delays, channel_ind = task._calculate_delays(ss)
    dsname, axes, waxes, fold = task._resolve(ss)
    data, weight, data_v, weight_v, fold_n = task._prepare_inputs(ss, ctx, dsname, axes, waxes, fold)
    nbase = int(np.prod(fold_n)) if fold_n else 1
    (b0, ev), = list(delay.nrml_evaluators(ctx, data_v, weight_v, fold_n, nbase, len(ss.index_map["ra"]), channel_ind, len(delays), task.window if task.apply_window else None,
                                           remove_mean=task.remove_mean, time_frac=task.time_frac, freq_frac=task.freq_frac, weight_boost=task.weight_boost))
    return ev, (data, weight)


@pytest.mark.parametrize("name", [c for c in cases.TASK_CASES if c != "NEG"] + ["EVAL"])
def test_evaluation(z, name):
    tr = truth_of(z, name)
    ev, hold = evaluator(z, name)
    live = np.zeros(ev.nb, dtype=bool)
    live[list(tr)] = True
    assert np.array_equal(ev.base == 0, live)
    if ev.S0 is not None:
        S0 = ev.S0.cpu().numpy()
        for b, t in tr.items():
            key = f"{name}/b{b}"
            lim = max(2 * float(z[f"{key}/e_S0"]), 4 * float(z[f"{key}/first/cond"]) * U53)
            e = twin.rel_err(S0[b], t["S0"])
            print(f"{key} start: {e:.2e} (allowed {lim:.2e})")
            assert e <= lim, (key, e, lim)
    N = ev.N
    for pt in cases.POINTS:
        x = np.zeros((ev.nb, N))
        for b in tr:
            x[b] = z[f"{name}/b{b}/{pt}/x"]
        f, g, ok = ev.value_grad(x, live)
        assert np.array_equal(ok, live)
        got = {"value": f, "grad": g}
        for q, exact in (("hess", 1), ("fisher", 0)):
            ev.hessian(live, exact=exact)
            got[q] = ev.H.cpu().numpy()
        for b, t in tr.items():
            key = f"{name}/b{b}/{pt}"
            for q in QUANT:
                lim = max(2 * float(z[f"{key}/e_{q}"]), 4 * float(z[f"{key}/cond"]) * U53)
                e = twin.rel_err(got[q][b], t[pt][q])
                print(f"{key} {q}: {e:.2e} e_ref {float(z[f'{key}/e_{q}']):.2e} (allowed {lim:.2e})")
                assert np.all(np.isfinite(got[q][b])) and e <= lim, (key, q, e, lim)
            assert np.array_equal(got["hess"][b], got["hess"][b].T)


def _device_cg(H, g):
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    N = len(g)
    H_d, g_d = ctx.to_device(np.ascontiguousarray(H)[None]), ctx.to_device(np.ascontiguousarray(g)[None])
    st, p, info = ctx.zeros((1,), np.int32), ctx.zeros((1, N), np.float64), ctx.zeros((1, 2), np.int32)
    _lib.check(_lib.lib.dmm_nrml_direction(ctx.handle, N, 1, ptr(H_d), ptr(g_d), ptr(st), ptr(p), ptr(info)))
    i = info.cpu().numpy()[0]
    return p.cpu().numpy()[0], int(i[0]), int(i[1])


@pytest.mark.parametrize("name", ["N16", "C23", "N70", "N160", "EVAL", "saddle", "flat"])
def test_direction(z, name):
    from draco_amd.analysis import delayopt

    pairs = []
    if name == "saddle":  # negative curvature at the first pass: the scaled steepest-descent step
        pairs.append((np.diag([-2.0, 2.0, -1.0, 3.0, 1.0]), np.array([0.3, -0.4, 0.1, 0.2, -0.7])))
        H = np.diag(np.r_[np.linspace(1, 5, 69), -0.5])  # negative curvature after some passes
        pairs.append((H, np.r_[np.ones(69), 1e-3]))
    elif name == "flat":  # a gradient below the termination threshold, and zero curvature
        pairs.append((np.eye(3), np.zeros(3)))
        pairs.append((np.zeros((3, 3)), np.array([1.0, 2.0, 3.0])))
    else:
        for b, data, Ni, fsel, N, win in cases.baselines(z, name):
            m = twin.model(data, N, Ni, fsel, win)
            for pt in cases.POINTS:
                t = twin.evaluate(m, z[f"{name}/b{b}/{pt}/x"], twin.matern_inverse(N))
                pairs.append(((t["hess"] + t["hess"].T) / 2, t["grad"]))
    for H, g in pairs:
        p, passes, flag = delayopt.cg_direction(H, g)
        pd, passes_d, flag_d = _device_cg(H, g)
        scale = np.abs(p).max()
        e = float(np.abs(pd - p).max() / scale) if scale > 0 else float(np.abs(pd).max())
        print(f"{name}: N {len(g)} passes {passes} / {passes_d} flag {flag} / {flag_d} err {e:.2e}")
        assert (passes_d, flag_d) == (passes, flag)
        assert e <= 1e-12


def _compare_iterates(tag, samples, xs, allow):
    assert len(samples) == len(xs), (tag, len(samples), len(xs))
    with np.errstate(divide="ignore"):
        d = float(np.abs(np.log(np.asarray(samples)) - xs).max())
    print(f"{tag}: {len(xs) - 1} iterations, iterates differ by {d:.2e} (allow {allow:.2e})")
    assert d <= allow, (tag, d, allow)


@pytest.mark.parametrize("name", cases.TASK_CASES)
def test_function(z, name):
    from draco_amd.analysis.delayopt import delay_power_spectrum_maxpost

    for b, data, Ni, fsel, N, win in cases.baselines(z, name):
        samples, ok = delay_power_spectrum_maxpost(data, N, Ni, window=win, fsel=fsel, maxiter=60, tol=1e-3)
        assert ok == bool(z[f"{name}/b{b}/success"]), (name, b)
        _compare_iterates(f"{name}/b{b}", samples, z[f"{name}/b{b}/x"], float(z["allow"]))


def _run_task(z, name, **over):
    task = make_task(name, **over)
    ss = container(z, name)
    out = task.process(ss)
    return task, ss, out


@pytest.mark.parametrize("name", cases.TASK_CASES)
def test_task(z, name):
    task, ss, out = _run_task(z, name)
    allow = float(z["allow"])
    nbase, ndelay = int(z[f"{name}/nbase"]), len(z[f"{name}/delays"])
    assert out.spectrum.on_device and out.spectrum.dtype == np.float64
    spec, samp, mask = out.spectrum[:], out.datasets["spectrum_samples"][:], out.datasets["spectrum_mask"][:]
    rspec, rsamp, rmask = z[f"{name}/spectrum"], z[f"{name}/spectrum_samples"], z[f"{name}/spectrum_mask"]
    assert spec.shape == (nbase, ndelay) and samp.shape == rsamp.shape and mask.dtype == np.bool_
    assert np.array_equal(mask, rmask)
    assert np.array_equal(out.index_map["delay"], z[f"{name}/delays"])
    assert np.array_equal(samp != 0, rsamp != 0) and np.array_equal(spec != 0, rspec != 0)
    for b in range(nbase):
        if b in z[f"{name}/skipped"]:
            assert mask[b] and not spec[b].any() and not samp[:, b].any()
            continue
        k = len(z[f"{name}/b{b}/x"])
        _compare_iterates(f"{name} task b{b}", samp[-k:, b], z[f"{name}/b{b}/x"], allow)
        assert np.array_equal(spec[b], np.fft.fftshift(samp[-1, b]))
        assert np.abs(np.log(spec[b]) - np.log(rspec[b])).max() <= allow
    if name == "NEG":
        assert mask.tolist() == [True] and samp[:-1].any() == False  # noqa: E712  (flagged, one sample, no exception)
    # the baseline axis and the attributes
    if f"{name}/map" in z.files:
        assert out.attrs["baseline_axes"] == ["beam", "pol", "el"] and len(out.index_map["baseline"]) == nbase
        assert np.array_equal(out.index_map["baseline"], np.arange(nbase)) and np.array_equal(out.index_map["el"], ss.index_map["el"])
        assert np.array_equal(ss.map[:], z[f"{name}/map"]) and np.array_equal(ss.weight[:], z[f"{name}/weight"])
    else:
        assert out.attrs["baseline_axes"] == ["stack"] and np.array_equal(out.index_map["baseline"], ss.index_map["stack"]) and np.array_equal(out.index_map["stack"], ss.index_map["stack"])
        assert np.array_equal(ss.vis[:], z[f"{name}/vis"]) and np.array_equal(ss.weight[:], z[f"{name}/weight"])
    assert np.array_equal(out.attrs["freq"], z[f"{name}/freq"]) and len(out.index_map["sample"]) == 60


def test_task_options(z):
    from draco_amd.analysis.delay import DelayPowerSpectrumNRML

    # without the optional datasets; the cap keeps the last nsamp iterates and flags the baseline
    task = DelayPowerSpectrumNRML(sample_axis="ra", nsamp=60)
    out = task.process(container(z, "N16"))
    assert "spectrum_samples" not in out.datasets and "spectrum_mask" not in out.datasets
    _, _, full = _run_task(z, "N16")
    assert np.array_equal(out.spectrum[:], full.spectrum[:])
    _, _, cap = _run_task(z, "N16", nsamp=5)
    assert cap.datasets["spectrum_mask"][:].tolist() == [True]
    assert np.array_equal(cap.datasets["spectrum_samples"][:, 0], full.datasets["spectrum_samples"][:, 0][full.datasets["spectrum_samples"][:, 0].any(axis=1)][1:6])
    with pytest.raises(NotImplementedError):
        DelayPowerSpectrumNRML(sample_axis="ra", use_average_weights=False).process(container(z, "N16"))
    with pytest.raises(NotImplementedError):
        DelayPowerSpectrumNRML(sample_axis="ra", scale_freq=True).process(container(z, "N16"))


@pytest.mark.parametrize("name", ["N32", "RM32"])
def test_workspace_batches(z, name):
    """One baseline per batch gives the same bits as one batch."""
    _, _, a = _run_task(z, name)
    _, _, b = _run_task(z, name, workspace_mib=0)
    assert np.array_equal(a.spectrum[:].view(np.uint64), b.spectrum[:].view(np.uint64))
    assert np.array_equal(a.datasets["spectrum_samples"][:].view(np.uint64), b.datasets["spectrum_samples"][:].view(np.uint64))
    assert np.array_equal(a.datasets["spectrum_mask"][:], b.datasets["spectrum_mask"][:])


def test_loglike_class(z):
    """``LogLikePS`` on the device as a batch of one against its NumPy form."""
    from draco_amd.analysis import delayopt

    _, data, Ni, fsel, N, win = next(cases.baselines(z, "N32"))
    X, MF, Nm, nsamp, S0 = delayopt._model_host(data, N, Ni, win, fsel)
    x = z["N32/b0/last/x"]
    for exact in (True, False):
        dev = delayopt.LogLikePS(X, MF, Nm, nsamp, exact_hessian=exact, bounds=(1e-15, 1e10))
        host = delayopt.LogLikePS(X, MF, Nm, nsamp, exact_hessian=exact, bounds=(1e-15, 1e10), device=False)
        lim = 2 * 4 * float(z["N32/b0/last/cond"]) * U53  # two float64 evaluations, each within 4 kappa u of the truth
        assert abs(dev.value(x) - host.value(x)) <= lim * abs(host.value(x))
        assert twin.rel_err(dev.hessian(x), host.hessian(x)) <= lim
        assert twin.rel_err(dev.gradient(x), host.gradient(x)) <= lim
    with pytest.raises(ValueError, match="device=False"):  # a general matrix is for the NumPy form
        delayopt.LogLikePS(X, MF * (1 + 0.01 * np.arange(N)), Nm, nsamp)
    with pytest.raises(ValueError, match="device=False"):  # a zero row kept through fsel
        delayopt.LogLikePS(X, np.where(np.arange(len(MF))[:, None] == 2, 0, MF), Nm, nsamp, fsel=np.ones(len(MF), dtype=bool))


def test_limits():
    from draco_amd.analysis import delayopt
    from draco_amd.device import Context

    with pytest.raises(ValueError, match="at most"):
        delayopt.delay_power_spectrum_maxpost(np.ones((2, 4), dtype=complex), 2050, np.ones(4))
    with pytest.raises(ValueError, match="at most"):
        delayopt.delay_power_spectrum_maxpost(np.ones((2, 1025), dtype=complex), 2048, np.ones(1025))
    with pytest.raises(ValueError, match="at most"):
        delayopt.DeviceEvaluator(Context.get(), 2049, np.arange(4), 1)
