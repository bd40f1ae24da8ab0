"""The chi-squared mask path on the GPU: ``dmm_axis_reduce`` against the long-double twin under the criterion of
DESIGN.md section 7b (no further from the truth than twice the reference's own error, or 2^-22), the reduction tasks,
``RFIMaskChisqHighDelay`` against the reference-executed masks of ``tests/golden/chisqmask.npz`` (equal exactly), and
the chain delay filter -> chi-squared -> mask -> weights."""

import os
import types
import warnings

import numpy as np
import pytest

import chisqmask_twin as twin

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chisqmask.npz")
FLOOR = 2.0**-22
DTYPES = {"f32": np.float32, "f64": np.float64, "c64": np.complex64, "c128": np.complex128}


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _err(got, truth):
    truth, got = np.asarray(truth), np.asarray(got)
    if np.iscomplexobj(got) and not np.iscomplexobj(truth):
        assert not got.imag.any()
        got = got.real
    diff, scale = float(np.abs(np.asarray(got, dtype=truth.dtype) - truth).max()), float(np.abs(truth).max())
    if scale == 0.0:  # a truth of zeros (one sample per column): only zeros are right
        return 0.0 if diff == 0.0 else np.inf
    return diff / scale


def _reduce(op, x, w, axis, factor=1.0):
    from draco_amd.analysis.transform import axis_reduce_device
    from draco_amd.device import Context

    ctx = Context.get()
    out, out_w = axis_reduce_device(ctx, op, ctx.to_device(x), None if w is None else ctx.to_device(w), axis[0], axis[-1], factor)
    return out.cpu().numpy(), out_w.cpu().numpy()


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("sname", ["s3x5x70", "s2x1x65", "s1x193x2", "hybrid"])
def test_axis_reduce(gold, sname, dname):
    from draco_amd import _lib

    dt = DTYPES[dname]
    x, w, axis = gold[f"red/{sname}/x"], gold[f"red/{sname}/w"], tuple(int(a) for a in gold[f"red/{sname}/axis"])
    x = (x if np.dtype(dt).kind == "c" else x.real).astype(dt)
    key = f"red/{sname}/{dname}"

    def check(what, got, truth):
        e_gpu, e_ref = _err(got, truth), _err(gold[f"{key}/{what}"], truth)
        print(f"{key}/{what}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e}")
        assert e_gpu <= max(2.0 * e_ref, FLOOR)

    v, num = _reduce(_lib.DMM_REDUCE_CHISQ, x, w, axis)
    tv, tnum = twin.reduce_chisq(x, w, axis)
    assert v.dtype == dt and v.shape == tv.shape and np.array_equal(num, tnum) and np.array_equal(num, gold[f"{key}/chisq_w"])
    assert not np.iscomplexobj(v) or not v.imag.any()
    check("chisq", v.real, tv)
    lone = np.broadcast_to((w > 0), x.shape).sum(axis=axis, keepdims=True) <= 1  # no or one positive weight
    assert lone.any() and not v[lone].any() and not num[lone].any()

    for weighting, op in (("none", _lib.DMM_REDUCE_VAR_NONE), ("masked", _lib.DMM_REDUCE_VAR_MASKED), ("weighted", _lib.DMM_REDUCE_VAR_WEIGHTED)):
        v, ws = _reduce(op, x, w, axis)
        tv, tws = twin.reduce_var(x, w, axis, weighting)
        assert np.array_equal(ws, np.asarray(tws, dtype=np.float64)) and np.array_equal(ws, gold[f"{key}/var_{weighting}_w"])
        check(f"var_{weighting}", v, tv)

    y, s = _reduce(_lib.DMM_REDUCE_WMEAN, x, w, axis, factor=3.0)
    ty, ts = twin.reduce_wmean(x, np.broadcast_to(w, x.shape), axis, 3.0)
    assert y.dtype == np.float64 and np.array_equal(s.squeeze(axis), np.asarray(ts, dtype=np.float64))
    y1, s1 = _reduce(_lib.DMM_REDUCE_WMEAN, x, w, axis)
    ty1, _ = twin.reduce_wmean(x, np.broadcast_to(w, x.shape), axis)
    assert np.array_equal(s1.squeeze(axis), gold[f"{key}/wmean_w"])
    e_gpu, e_ref = _err(y1.squeeze(axis), ty1), _err(gold[f"{key}/wmean"], ty1)
    assert e_gpu <= max(2.0 * e_ref, FLOOR) and _err(y.squeeze(axis), ty) <= max(2.0 * e_ref, FLOOR)


def test_axis_reduce_expands_a_weight_it_cannot_address():
    """Three reduced axes with three different weight strides do not fit the kernel's two: the weight is expanded."""
    from draco_amd import _lib

    rng = np.random.default_rng(2)
    x = rng.normal(size=(2, 3, 4, 2, 33)).astype(np.float32)
    w = rng.integers(0, 5, size=(1, 3, 1, 2, 33)).astype(np.float32)  # lacks the outer axis and the middle reduced one
    y, s = _reduce(_lib.DMM_REDUCE_WMEAN, x, w, (1, 2, 3))
    ty, ts = twin.reduce_wmean(x, np.broadcast_to(w, x.shape), (1, 2, 3))
    assert np.array_equal(s.squeeze((1, 2, 3)), np.asarray(ts, dtype=np.float64)) and _err(y.squeeze((1, 2, 3)), ty) <= FLOOR


def _timestream(gold, ns=3, device=False):
    from draco_amd.core import containers
    from draco_amd.device import Context

    x, w = gold["in/ts/x"][:, :ns], gold["in/ts/w"][:, :ns]
    s = containers.TimeStream(freq=gold["in/freq"], stack=ns, time=gold["in/time"])
    s.vis[:] = x + 1j * x[..., ::-1]
    s.weight[:] = w
    if device:
        ctx = Context.get()
        s.vis.set_device(s.vis.device(ctx))
        s.weight.set_device(s.weight.device(ctx))
    return s


def _telescope():
    return types.SimpleNamespace(lmax=1, mmax=1, frequencies=None, lsd_to_unix=lambda lsd: 1.5e9 + 86164.0905 * np.asarray(lsd))


def _run_case(gold, name, device=False, subclass=None):
    from draco_amd.analysis import flagging
    from draco_amd.core import containers

    kind = str(gold[f"case/{name}/input"])
    cfg = {k: gold[f"case/{name}/{k}"].item() for k in ("win_t", "win_f", "estimate_var", "only_positive", "separate_pol", "mask_type")}
    if gold[f"case/{name}/flag_ew"].size:
        cfg["flag_ew"] = gold[f"case/{name}/flag_ew"]
    hooks = bool(gold[f"case/{name}/hooks"])
    day, sources = gold["in/day"], gold["in/sources"]

    class Hooked(flagging.RFIMaskChisqHighDelay):
        def _day_flag_hook(self, times):
            assert times.shape == day.shape
            return day

        def _source_flag_hook(self, times, freq):
            assert (freq.size, times.size) == sources.shape
            return sources

    cls = subclass or (Hooked if hooks else flagging.RFIMaskChisqHighDelay)
    task = cls(**cfg)
    if kind in ("ts", "ts1"):
        s = _timestream(gold, 3 if kind == "ts" else 1, device)
        task.setup()
        want = containers.RFIMask
    else:
        if kind == "sid":
            x, w = gold["in/ts/x"], gold["in/ts/w"]
            s = containers.SiderealStream(freq=gold["in/freq"], stack=3, ra=gold["in/ra"])
            want = containers.SiderealRFIMask
        else:
            x, w = gold["in/hyb/x"], gold["in/hyb/w"]
            s = containers.HybridVisStream(pol=np.array(["XX", "YY"]), freq=gold["in/freq"], ew=2, el=2, ra=gold["in/ra"])
            want = containers.SiderealRFIMaskByPol if cfg["separate_pol"] else containers.SiderealRFIMask
        s.vis[:] = x + 1j * x[..., ::-1]
        s.weight[:] = w
        lsd = gold[f"case/{name}/lsd"]
        s.attrs["lsd"] = 4321 if (lsd.ndim == 0 and lsd < 0) else (int(lsd) if lsd.ndim == 0 else lsd)
        task.setup(_telescope())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the baseline fit says when it stops at its iteration limit)
        out = task.process(s)
    assert type(out) is want
    return out


CASES = ["mad_t21", "mad_t601", "mad_var", "mad_positive", "st_t21", "st_t601", "st_var_positive", "stack1", "hybrid_bypol", "hybrid_all", "sidereal_scalar",
         "sidereal_vector"]


def test_golden_lists_these_cases(gold):
    assert list(gold["case/names"]) == CASES


@pytest.mark.parametrize("name", CASES)
def test_mask_equals_the_reference(gold, name):
    out = _run_case(gold, name)
    got, ref = np.asarray(out.mask[:]), gold[f"case/{name}/mask"]
    assert got.dtype == bool and got.shape == ref.shape
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} samples differ"


def test_hooks_are_honoured(gold):
    from draco_amd.analysis import flagging

    hooked = np.asarray(_run_case(gold, "sidereal_scalar").mask[:])
    plain = np.asarray(_run_case(gold, "sidereal_scalar", subclass=flagging.RFIMaskChisqHighDelay).mask[:])
    assert np.array_equal(hooked, gold["case/sidereal_scalar/mask"]) and not np.array_equal(hooked, plain)
    # several days: the daytime hook is not asked
    many = np.asarray(_run_case(gold, "sidereal_vector").mask[:])
    assert np.array_equal(many, gold["case/sidereal_vector/mask"])


@pytest.mark.parametrize("name", ["mad_t21", "st_t21"])
def test_device_resident_input(gold, name):
    a = np.asarray(_run_case(gold, name, device=True).mask[:])
    assert np.array_equal(a, gold[f"case/{name}/mask"])


def test_public_steps(gold):
    from draco_amd.analysis import flagging
    from draco_amd.device import Context

    for name, mask_type in (("mad_t21", "mad"), ("st_t21", "sumthreshold")):
        task = flagging.RFIMaskChisqHighDelay(win_t=21, mask_type=mask_type)
        task.setup()
        y, w, m = gold[f"step/{name}/y"], gold[f"step/{name}/w"], gold[f"step/{name}/m"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert np.array_equal(task.mask_1d(y, m), gold[f"step/{name}/mask_1d"])
        assert np.array_equal(task.mask_2d(y, w), gold[f"step/{name}/mask_2d"])
        ctx = Context.get()
        on_dev = task.mask_2d(ctx.to_device(y), ctx.to_device(w))
        assert on_dev.is_cuda and np.array_equal(on_dev.cpu().numpy(), gold[f"step/{name}/mask_2d"])
    assert np.array_equal(task.mask_2d_sumthreshold(y, w), gold["step/st_t21/mask_2d_sumthreshold"])


def test_reduce_tasks(gold):
    """ReduceChisq and ReduceVar on a time stream and on a hybrid stream whose weight lacks ``el``."""
    from draco_amd.analysis.transform import ReduceChisq, ReduceVar
    from draco_amd.core import containers

    s = _timestream(gold)
    vis, w = np.asarray(s.vis[:]), np.asarray(s.weight[:])
    out = ReduceChisq(axes=["stack"], dataset="vis").process(s)
    assert type(out) is containers.TimeStream and out.vis.on_device and out.weight.on_device
    assert out.vis.shape == (24, 1, 160) and out.weight.shape == (24, 1, 160) and out.index_map["stack"].tolist() == [0]
    assert out.attrs["reduction_op"] == "chisq_per_dof" and out.attrs["reduced"] is True
    tv, tnum = twin.reduce_chisq(vis, w, (1,))
    assert np.array_equal(out.weight[:], tnum) and _err(out.vis[:].real, tv) <= FLOOR and not out.vis[:].imag.any()

    for dev in (False, True):
        s = _timestream(gold, device=dev)
        out = ReduceVar(axes=["stack"], dataset="vis", weighting="weighted").process(s)
        tv, tws = twin.reduce_var(vis, w, (1,), "weighted")
        assert np.array_equal(out.weight[:], np.asarray(tws, dtype=np.float32)) and _err(out.vis[:], tv) <= FLOOR

    x, wh = gold["in/hyb/x"], gold["in/hyb/w"]
    h = containers.HybridVisStream(pol=np.array(["XX", "YY"]), freq=gold["in/freq"], ew=2, el=2, ra=gold["in/ra"])
    h.vis[:] = x + 1j * x[..., ::-1]
    h.weight[:] = wh
    out = ReduceChisq(axes=["ew", "el"], dataset="vis").process(h)
    tv, tnum = twin.reduce_chisq(np.asarray(h.vis[:]), wh[:, :, :, None, :], (2, 3))
    assert out.vis.shape == (2, 24, 1, 1, 160) and out.weight.shape == (2, 24, 1, 160)
    assert np.array_equal(out.weight[:], tnum[:, :, :, 0]) and _err(out.vis[:].real, tv) <= FLOOR


def test_chain():
    """Noise and a smooth foreground with a burst on 3 frequencies x 8 times: delay filter, chi-squared over the
    baselines, mask, weights."""
    from draco_amd.analysis.dayenu import DayenuDelayFilter
    from draco_amd.analysis.flagging import ApplyTimeFreqMask, RFIMaskChisqHighDelay
    from draco_amd.analysis.transform import ReduceChisq
    from draco_amd.core import containers

    nf, ns, nt = 32, 12, 192
    rng = np.random.default_rng(8)
    freq = 800.0 - 0.390625 * np.arange(nf)
    prod = np.zeros(ns, dtype=[("input_a", "<u2"), ("input_b", "<u2")])
    prod["input_b"] = 1 + np.arange(ns)
    feedpos = np.zeros((ns + 1, 2))
    feedpos[1:, 1] = 0.3 * (1 + np.arange(ns))
    sigma = 0.5
    noise = sigma * np.sqrt(0.5) * (rng.normal(size=(nf, ns, nt)) + 1j * rng.normal(size=(nf, ns, nt)))
    fg = 30.0 * np.exp(2j * np.pi * rng.uniform(size=(1, ns, nt))) * (1.0 + 0.05 * np.cos((freq - 794.0) / 9.0))[:, None, None]  # smooth over the band
    burst = np.zeros((nf, nt), dtype=bool)
    burst[11:14, 100:108] = True
    rfi = 5.0 * sigma * np.exp(2j * np.pi * rng.uniform(size=(nf, ns, nt))) * burst[:, None, :]
    s = containers.TimeStream(freq=freq, time=1.6e9 + 10.0 * np.arange(nt), prod=prod, input=ns + 1)
    s.vis[:] = (noise + fg + rfi).astype(np.complex64)
    s.weight[:] = np.float32(1.0 / sigma**2)

    filt = DayenuDelayFilter(tauw=0.2, epsilon=1e-10)
    filt.setup(types.SimpleNamespace(feedpositions=feedpos, lmax=1, mmax=1, frequencies=None))
    s = filt.process(s)
    chisq = ReduceChisq(axes=["stack"], dataset="vis").process(s)
    assert chisq.vis.on_device and chisq.vis.shape == (nf, 1, nt)
    task = RFIMaskChisqHighDelay(win_t=41)
    task.setup()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rfimask = task.process(chisq)
        mask = np.asarray(rfimask.mask[:])
        replay = twin.chisq_mask(chisq.vis[:].real[:, 0], chisq.weight[:][:, 0].astype(np.float64), win=(1, 41))
    print(f"chain: {100 * mask[~burst].mean():.2f} % of the clean samples masked, rows {np.flatnonzero(mask.all(axis=1)).tolist()}")
    assert mask[burst].all()
    assert mask[~burst].mean() < 0.05
    assert np.array_equal(mask, replay)
    before = np.asarray(s.weight[:]).copy()
    assert (before > 0).all()
    out = ApplyTimeFreqMask().process(s, rfimask)
    after = np.asarray(out.weight[:])
    assert np.array_equal(after == 0, np.broadcast_to(mask[:, None, :], after.shape))
    assert np.array_equal(after[after != 0], before[after != 0])
