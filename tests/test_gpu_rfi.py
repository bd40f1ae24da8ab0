"""The RFI kernels and mask tasks on the GPU against the NumPy twin (``tests/rfi_twin.py``) and the reference-executed
vectors of ``tests/golden/rfi.npz``.  Medians are exact: the same number as the twin's sort-based median at every
sample, NaN at the same samples.  Masks are equal exactly."""

import os

import numpy as np
import pytest

import rfi_twin as twin
from test_rfi_host import SENS_CFG, SENS_NAMES, SIR_KW, ST_KW, st_kwargs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rfi.npz")
TILE = 32  # output times per block of the median kernel


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def plane(seed, nf, nt, block=None, quantised=False):
    """About 30 % random flags, a fully flagged row and column, a flagged block, NaN under flags, negative values and
    both zeros; ``quantised``: eight distinct values, so many equal keys."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(nf, nt))
    if quantised:
        x = np.round(x * 2.0).clip(-4, 3) / 2.0
    m = rng.uniform(size=(nf, nt)) < 0.3
    if nf > 2 and nt > 2:
        m[nf // 3] = True
        m[:, nt // 4] = True
        x[nf - 1, 0], x[nf - 1, 1] = 0.0, -0.0
        x[0, nt - 1] = -0.0
    if block is not None:
        m[block] = True
    x[m & (rng.uniform(size=(nf, nt)) < 0.3)] = np.nan
    return x, m


# (name, nf, nt, window, flagged block, quantised)
MED_CASES = [
    ("one", 1, 1, (3, 3), None, False),
    ("small_big_window", 7, 5, (37, 181), None, False),
    ("w7x15", 40, 96, (7, 15), (slice(10, 24), slice(30, 64)), False),
    ("w11x5", 40, 96, (11, 5), (slice(10, 24), slice(30, 64)), True),
    ("w1x9", 40, 96, (1, 9), (slice(10, 24), slice(30, 64)), False),
    ("w9x1", 40, 96, (9, 1), (slice(10, 24), slice(30, 64)), True),
    ("w7x15_below_tile", 40, 3 * TILE - 1, (7, 15), None, True),
    ("w7x15_above_tile", 40, 3 * TILE + 1, (7, 15), None, False),
    ("w37x181", 48, 260, (37, 181), (slice(0, 40), slice(0, 200)), False),
    ("w101x31", 48, 260, (101, 31), (slice(0, 48), slice(100, 140)), True),
]


@pytest.fixture(scope="module")
def med_refs():
    out = {}
    for i, (name, nf, nt, size, block, quant) in enumerate(MED_CASES):
        x, m = plane(100 + i, nf, nt, block, quant)
        out[name] = (x, m, twin.moving_weighted_median(x, ~m, size))
    return out


@pytest.mark.parametrize("case", MED_CASES, ids=[c[0] for c in MED_CASES])
def test_medfilt(med_refs, case):
    from draco_amd.util import filters

    name, nf, nt, size, block, _ = case
    x, m, ref = med_refs[name]
    got = filters.medfilt(x, m, size)
    assert got.shape == ref.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got, ref, equal_nan=True)
    if block is not None and name != "w9x1" and name != "w1x9":
        assert np.isnan(ref).any()  # the flagged block is larger than the window: empty windows are covered


def test_medfilt_batch_bits(med_refs):
    """A plane filtered alone and as one plane of a batch: identical bits."""
    import torch

    from draco_amd.device import Context
    from draco_amd.util import filters

    ctx = Context.get()
    xs, ms = zip(*[med_refs[n][:2] for n in ("w7x15", "w11x5", "w1x9")])
    xb, mb = ctx.to_device(np.stack(xs)), ctx.to_device(np.stack(ms).view(np.uint8))
    batch = filters.medfilt(xb, mb, (7, 15))
    assert isinstance(batch, torch.Tensor) and batch.shape == xb.shape
    for i in range(3):
        alone = filters.medfilt(xb[i].clone(), mb[i].clone(), (7, 15))
        assert torch.equal(alone.view(torch.int64), batch[i].view(torch.int64))
    assert np.array_equal(batch[0].cpu().numpy(), med_refs["w7x15"][2], equal_nan=True)


def test_medfilt_1d_and_complex():
    from draco_amd.util import filters

    rng = np.random.default_rng(7)
    x = rng.normal(size=300)
    m = rng.uniform(size=300) < 0.3
    m[100:140] = True
    assert np.array_equal(filters.medfilt(x, m, 21), twin.moving_weighted_median(x, ~m, 21), equal_nan=True)
    assert np.array_equal(filters.medfilt(x, m, (191,)), twin.moving_weighted_median(x, ~m, 191), equal_nan=True)
    xc = (rng.normal(size=(12, 40)) + 1j * rng.normal(size=(12, 40))).astype(np.complex64)
    mc = rng.uniform(size=(12, 40)) < 0.2
    assert np.array_equal(filters.medfilt(xc, mc, (3, 5)), twin.medfilt(xc, mc, (3, 5)), equal_nan=True)
    with pytest.raises(ValueError):
        filters.medfilt(x, m, 20)


def test_quantile():
    from draco_amd.device import Context
    from draco_amd.util import filters

    rng = np.random.default_rng(11)
    counts = [0, 1, 2, 7, 20, 40, 59, 60]
    n = 60
    y = np.round(rng.normal(size=(len(counts), n)), 1)  # ties
    m = np.ones((len(counts), n), dtype=bool)
    for i, c in enumerate(counts):
        m[i, rng.permutation(n)[:c]] = False
    y[m & (rng.uniform(size=m.shape) < 0.5)] = np.nan
    ctx = Context.get()
    for q in (0.15, 0.0, 0.5, 1.0, 0.05):
        got, cnt = filters.quantile_device(ctx, ctx.to_device(y), ctx.to_device(m.view(np.uint8)), q, count=True)
        assert np.array_equal(got.cpu().numpy(), twin.quantile(y, ~m, q), equal_nan=True), q
        assert list(cnt.cpu().numpy()) == counts
    long = rng.normal(size=(3, 8640))
    lm = rng.uniform(size=long.shape) < 0.3
    got = filters.quantile_device(ctx, ctx.to_device(long), ctx.to_device(lm.view(np.uint8)), 0.15)
    assert np.array_equal(got.cpu().numpy(), twin.quantile(long, ~lm, 0.15))


@pytest.mark.parametrize("name", list(ST_KW))
def test_sumthreshold(gold, name):
    from draco_amd.util import rfi

    got = rfi.sumthreshold(gold["st/data"], **st_kwargs(gold, name))
    assert got.dtype == np.bool_ and np.array_equal(got, gold[f"st/{name}/mask"])


def test_sumthreshold_forms(gold):
    """Device tensors in and out, one line, and the twin on a second plane with hits at both ends of each axis."""
    import torch

    from draco_amd.device import Context
    from draco_amd.util import rfi

    ctx = Context.get()
    kw = st_kwargs(gold, "m8_var")
    dev = {k: (ctx.to_device(v if v.dtype != np.bool_ else v.view(np.uint8)) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    got = rfi.sumthreshold_py(ctx.to_device(gold["st/data"]), **dev)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), gold["st/m8_var/mask"])
    rng = np.random.default_rng(5)
    d = rng.normal(size=(9, 70))
    d[0, 0], d[8, 69], d[0, 69], d[8, 0] = 12.0, -12.0, 11.0, -11.0
    for kw in (dict(max_m=64, threshold1=3.5), dict(max_m=4, threshold1=3.5, axes=(0, 1), only_positive=True), dict(max_m=8)):
        assert np.array_equal(rfi.sumthreshold(d, **kw), twin.sumthreshold(d, **kw)), kw
    line = d[3]
    assert np.array_equal(rfi.sumthreshold(line, max_m=8, threshold1=2.0), twin.sumthreshold(line[None, :], max_m=8, threshold1=2.0, axes=(1,))[0])
    with pytest.raises(RuntimeError, match="starting threshold"):
        rfi.sumthreshold(d, variance=np.ones_like(d))


@pytest.mark.parametrize("name", list(SIR_KW))
def test_sir(gold, name):
    from draco_amd.util import rfi

    eta, axis = SIR_KW[name]
    got = rfi.scale_invariant_rank(gold["sir/base"], eta=eta, axis=axis)
    assert got.dtype == np.bool_ and np.array_equal(got, gold[f"sir/{name}/mask"])


def test_sir_ties():
    """Runs of four clean samples and one flagged one at eta 0.2: the sums return to values that tie."""
    from draco_amd.util import rfi

    line = np.tile([False, False, False, False, True], 40)
    ref = twin.sir_line(line, 0.2)
    assert np.array_equal(rfi.sir1d(line, eta=0.2), ref)
    assert np.array_equal(rfi._sir_lastaxis(np.stack([line, ~line]), 0.2, axis=-1), np.stack([ref, twin.sir_line(~line, 0.2)]))
    assert np.array_equal(rfi.sir1d(np.stack([line, ~line]).T.copy(), eta=0.2, axis=0), np.stack([ref, twin.sir_line(~line, 0.2)]).T)
    with pytest.raises(ValueError, match="same length"):
        rfi.scale_invariant_rank(np.stack([line, line]), eta=(0.1, 0.2, 0.3), axis=(0, 1))


def test_sir_tiles():
    """More lines and more samples than one 64 x 64 tile of the time-axis kernel, neither a multiple of 64."""
    from draco_amd.util import rfi

    rng = np.random.default_rng(23)
    base = rng.uniform(size=(70, 150)) < 0.15
    base[65, 120:] = True
    base[:, 64] = True
    for axis in (-1, 0, (0, -1)):
        assert np.array_equal(rfi.scale_invariant_rank(base, eta=0.2, axis=axis), twin.scale_invariant_rank(base, eta=0.2, axis=axis)), axis
    one = base[:1, :64]
    assert np.array_equal(rfi.sir1d(one, eta=0.3), twin.sir1d(one, eta=0.3))


def test_mad_and_tv(gold):
    from draco_amd.analysis import flagging

    r = flagging.mad(gold["mad/x"], gold["mad/mask"], base_size=(5, 3), mad_size=(7, 9))
    assert np.array_equal(r, gold["mad/real"], equal_nan=True)
    rc = flagging.mad(gold["mad/xc"], gold["mad/mask"], base_size=(5, 3), mad_size=(7, 9))
    ref = gold["mad/complex"]
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isnan(rc), ~ok) and np.all(np.abs(rc[ok] - ref[ok]) <= 8 * 2.0**-53 * np.abs(ref[ok]))
    r2, dev, m = flagging.mad(gold["mad/x"], gold["mad/mask"], base_size=(5, 3), mad_size=(7, 9), debug=True, sigma=False)
    assert np.array_equal(m, twin.medfilt(dev, gold["mad/mask"], (7, 9)), equal_nan=True)
    mask, frac = flagging.tv_channels_flag(gold["tv/x"], gold["mad/freq"], sigma=3.0, f=0.3, debug=True)
    assert frac.dtype == np.float32 and np.array_equal(frac, gold["tv/frac"]) and np.array_equal(mask, gold["tv/mask"])
    assert np.array_equal(flagging.tv_channels_flag(gold["tv/x"], gold["mad/freq"], sigma=3.0, f=0.3), gold["tv/mask"])
    # frequencies outside every TV channel keep the fraction 1
    mask = flagging.tv_channels_flag(gold["tv/x"], np.linspace(200.0, 240.0, gold["tv/x"].shape[0]), sigma=3.0, f=0.3)
    assert mask.all()


def _device_resident(cont, ctx):
    for ds in cont.datasets.values():
        if ds.dtype != np.bool_:
            ds.set_device(ctx.to_device(ds.host()))
    return cont


@pytest.mark.parametrize("name", SENS_NAMES)
def test_sensitivity_mask(gold, name):
    from draco_amd.analysis import flagging
    from draco_amd.core import containers
    from draco_amd.device import Context

    mixed, static, sir, only_time, glob, pol = (bool(b) for b in gold[f"sens/{name}/flags"])

    class Task(flagging.RFISensitivityMask):
        def _combine_st_mad_hook(self, times, freq):
            return gold["sens/mixed"] if mixed else super()._combine_st_mad_hook(times, freq)

        def _static_rfi_mask_hook(self, freq, timestamp=None):
            return ~gold["sens/static"] if static else super()._static_rfi_mask_hook(freq, timestamp)

    cfg = dict(SENS_CFG, mask_type=str(gold[f"sens/{name}/mask_type"]), sir=sir, only_time=only_time)
    if glob:
        cfg["win_f_1d"] = None
    if pol:
        cfg["include_pol"] = ["YY"]
    sens = containers.SystemSensitivity(freq=gold["sens/freq"], pol=np.array(["XX", "YY"]), time=gold["sens/time"])
    sens.measured[:], sens.radiometer[:], sens.weight[:] = gold["sens/measured"], gold["sens/radiometer"], gold["sens/weight"]
    sens.attrs["tag"] = "day"
    _device_resident(sens, Context.get())
    task = Task(**cfg)
    task.setup()
    out = task.process(sens)
    assert isinstance(out, containers.RFIMask) and out.attrs["tag"] == "day" and np.array_equal(out.time, gold["sens/time"])
    assert out.mask[:].dtype == np.bool_ and np.array_equal(out.mask[:], gold[f"sens/{name}/mask"])


def _stream(gold, kind, ctx):
    from draco_amd.core import containers

    freq, time = gold["sens/freq"], gold["sens/time"]
    if kind == "time":
        ts = containers.TimeStream(freq=freq, stack=3, time=time)
    else:
        ts = containers.SiderealStream(freq=freq, stack=3, ra=len(time))
    ts.vis[:], ts.weight[:] = gold["rfimask/vis"], gold["rfimask/weight"]
    return _device_resident(ts, ctx)


@pytest.mark.parametrize("kind", ["time", "ra"])
def test_rfimask_task(gold, kind):
    from draco_amd.analysis import flagging
    from draco_amd.core import containers
    from draco_amd.device import Context

    ts = _stream(gold, kind, Context.get())
    out = flagging.RFIMask(stack_ind=1).process(ts)
    assert type(out) is (containers.RFIMask if kind == "time" else containers.SiderealRFIMask)
    assert np.array_equal(out.mask[:], gold[f"rfimask/{kind}/mask"])
    assert ts.vis.on_device and ts.vis._host is None  # the stream was not brought back to the host
    with pytest.raises(ValueError, match="stack_ind"):
        flagging.RFIMask(stack_ind=3).process(ts)


def test_apply_device(gold):
    from draco_amd.analysis import flagging
    from draco_amd.core import containers
    from draco_amd.device import Context

    ctx = Context.get()
    freq, time = gold["sens/freq"], gold["sens/time"]
    ts = _stream(gold, "time", ctx)
    w0 = ts.weight._dev.clone()
    rm = containers.RFIMask(freq=freq, time=time)
    rm.mask[:] = gold["apply/mask"]
    res = flagging.ApplyTimeFreqMask(share="vis").process(ts, rm)
    assert res.vis is ts.vis and res.weight.on_device and res.weight._host is None and (ts.weight._dev == w0).all()
    assert np.array_equal(res.weight[:], gold["apply/time/weight"])
    lo, hi = gold["apply/time_sub/range"]
    sub = containers.RFIMask(freq=freq, time=time[lo:hi])
    sub.mask[:] = gold["apply/mask"][:, lo:hi]
    res = flagging.ApplyTimeFreqMask(share="none", match_axes=False).process(ts, sub)
    assert res.weight.on_device and np.array_equal(res.weight[:], gold["apply/time_sub/weight"])
    res = flagging.ApplyTimeFreqMask().process(ts, rm)
    assert res is ts and ts.weight.on_device and np.array_equal(ts.weight[:], gold["apply/time/weight"])
    ss = _stream(gold, "ra", ctx)
    rp = containers.SiderealRFIMaskByPol(freq=freq, ra=ss.ra, pol=np.array(["XX", "YY"]))
    rp.mask[:] = gold["apply/mask_pol"]
    res = flagging.ApplyTimeFreqMask(share="none", collapse_pol=True).process(ss, rp)
    assert res.weight.on_device and np.array_equal(res.weight[:], gold["apply/ra_pol/weight"])
    hs = containers.HybridVisStream(pol=np.array(["XX", "YY"]), freq=freq, ew=3, el=2, ra=ss.ra)
    hs.weight[:] = gold["apply/hybrid/in"]
    _device_resident(hs, ctx)
    res = flagging.ApplyTimeFreqMask(share="none").process(hs, rp)
    assert res.weight.on_device and np.array_equal(res.weight[:], gold["apply/hybrid/weight"])
