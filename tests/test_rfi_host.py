"""Host-side checks of the RFI flagging path (no GPU): the NumPy twin against the reference-executed vectors of
``tests/golden/rfi.npz``, the TV thresholds, the new containers, and what ``ApplyTimeFreqMask`` and the median wrappers
refuse or do on host-resident data."""

import os

import numpy as np
import pytest

import rfi_twin as twin
from draco_amd.analysis import flagging
from draco_amd.core import containers
from draco_amd.util import filters

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rfi.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


ST_KW = {
    "m1": dict(max_m=1, threshold1=3.0),
    "m8": dict(max_m=8, threshold1=3.0, start_flag="start"),
    "m64": dict(max_m=64, threshold1=3.0, start_flag="start"),
    "m8_axes01": dict(max_m=8, threshold1=3.0, axes=(0, 1)),
    "m8_axis0": dict(max_m=8, threshold1=3.0, axes=0),
    "m8_var": dict(max_m=8, threshold1=3.0, variance="var", remove_median=False, start_flag="start"),
    "m8_var_nan": dict(max_m=8, threshold1=3.0, variance="var_nan", remove_median=False, start_flag="start", rho=1.0),
    "m8_positive": dict(max_m=8, threshold1=3.0, only_positive=True),
    "m8_nomissing": dict(max_m=8, threshold1=3.0, correct_for_missing=False, start_flag="start"),
    "m16_default": dict(),
}
SIR_KW = {"eta0": (0.0, -1), "eta02": (0.2, -1), "eta1": (1.0, -1), "eta02_ax0": (0.2, 0), "both": (0.2, (0, -1)), "tuple": ((0.1, 0.3), (0, -1))}
SENS_NAMES = ["mad_sir0", "mad_sir1", "sumthreshold_sir0", "sumthreshold_sir1", "combine_sir0", "combine_sir1", "combine_mixed_sir0", "combine_mixed_sir1", "mad_pol_global"]
SENS_CFG = dict(nsigma_1d=5.0, quantile_1d=0.15, win_f_1d=9, nsigma=5.0, niter=5, rho=1.5, base_size=(7, 15), mad_size=(11, 5), tv_fraction=0.5, max_m=64, eta=0.2)


def st_kwargs(gold, name):
    return {k: (gold[f"st/{v}"] if isinstance(v, str) else v) for k, v in ST_KW[name].items()}


def test_golden_lists(gold):
    assert list(gold["st/names"]) == list(ST_KW) and list(gold["sir/names"]) == list(SIR_KW) and list(gold["sens/names"]) == SENS_NAMES
    for k in gold:
        if k.endswith("/margin"):
            assert gold[k] > 1e-9, k


@pytest.mark.parametrize("name", list(ST_KW))
def test_twin_sumthreshold(gold, name):
    assert np.array_equal(twin.sumthreshold(gold["st/data"], **st_kwargs(gold, name)), gold[f"st/{name}/mask"])


@pytest.mark.parametrize("name", list(SIR_KW))
def test_twin_sir(gold, name):
    eta, axis = SIR_KW[name]
    assert np.array_equal(twin.scale_invariant_rank(gold["sir/base"], eta=eta, axis=axis), gold[f"sir/{name}/mask"])


def test_twin_mad(gold):
    r = twin.mad(gold["mad/x"], gold["mad/mask"], base_size=(5, 3), mad_size=(7, 9))
    assert np.array_equal(r, gold["mad/real"], equal_nan=True)
    rc = twin.mad(gold["mad/xc"], gold["mad/mask"], base_size=(5, 3), mad_size=(7, 9))
    ref = gold["mad/complex"]
    assert np.array_equal(np.isnan(rc), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.all(np.abs(rc[ok] - ref[ok]) <= 8 * 2.0**-53 * np.abs(ref[ok]))


def test_tv_thresholds(gold):
    freq = gold["mad/freq"]
    thr = np.array([t for _, t in twin.tv_thresholds(freq, 3.0, 0.3)])
    assert np.array_equal(thr, gold["tv/thresholds"]) and np.array_equal(gold["tv/thresholds"], gold["tv/thresholds_ref"])
    # the library's own host functions give the recorded values
    got = [flagging.p_to_sigma(flagging.inverse_binom_cdf_prob(int(0.3 * len(r)), len(r), 1 - flagging.sigma_to_p(3.0))) for r, _ in twin.tv_thresholds(freq, 3.0, 0.3)]
    assert np.array_equal(np.array(got), gold["tv/thresholds"])
    assert np.array_equal(twin.tv_channels_flag(gold["tv/x"], freq, sigma=3.0, f=0.3), gold["tv/mask"])


def sens_twin(gold, name):
    mixed, static, sir, only_time, glob, pol = (bool(b) for b in gold[f"sens/{name}/flags"])
    cfg = dict(SENS_CFG)
    if glob:
        cfg["win_f_1d"] = None
    return twin.sensitivity_mask(gold["sens/measured"], gold["sens/radiometer"], gold["sens/weight"], gold["sens/freq"], mask_type=str(gold[f"sens/{name}/mask_type"]),
                                 include=[False, True] if pol else None, static=gold["sens/static"] if static else None, madtimes=gold["sens/mixed"] if mixed else None,
                                 sir=sir, only_time=only_time, **cfg)


@pytest.mark.parametrize("name", SENS_NAMES)
def test_twin_sensitivity(gold, name):
    assert np.array_equal(sens_twin(gold, name), gold[f"sens/{name}/mask"])


def test_twin_rfimask(gold):
    m = twin.rfi_mask(gold["rfimask/vis"][:, 1], gold["rfimask/weight"][:, 1], gold["sens/freq"], 5.0, 0.5)
    assert np.array_equal(m, gold["rfimask/time/mask"]) and np.array_equal(m, gold["rfimask/ra/mask"])


def test_twin_conventions():
    x = np.array([[3.0, 1.0, 2.0, 5.0, 4.0]])
    w = np.array([[1, 1, 0, 1, 1]])
    assert np.array_equal(twin.moving_weighted_median(x, w, (1, 3)), [[2.0, 2.0, 3.0, 4.5, 4.5]])
    assert np.isnan(twin.moving_weighted_median(x, np.zeros_like(w), (1, 3))).all()
    with pytest.raises(ValueError):
        twin.moving_weighted_median(x, w, (1, 4))
    y = np.arange(20.0)[None, :]
    assert twin.quantile(y, np.ones_like(y), 0.15)[0] == 2.5  # t = 3 exactly: the mean of v[2] and v[3]
    assert twin.quantile(y[:, :7], np.ones((1, 7)), 0.15)[0] == 1.0
    assert np.isnan(twin.quantile(y, np.zeros_like(y), 0.15)[0])


def test_containers():
    freq, time = np.linspace(800, 400, 4), 1.0e9 + np.arange(6.0)
    ra = np.linspace(0, 360, 6, endpoint=False)
    pol = np.array(["XX", "YY"])
    m = containers.RFIMask(freq=freq, time=time)
    assert m.mask.shape == (4, 6) and m.mask.dtype == np.bool_ and list(m.mask.attrs["axis"]) == ["freq", "time"] and np.array_equal(m.time, time)
    s = containers.SiderealRFIMask(freq=freq, ra=6)
    assert s.mask.shape == (4, 6) and list(s.mask.attrs["axis"]) == ["freq", "ra"] and np.array_equal(s.ra, ra)
    mp = containers.RFIMaskByPol(freq=freq, time=time, pol=pol)
    sp = containers.SiderealRFIMaskByPol(freq=freq, ra=ra, pol=pol)
    assert mp.mask.shape == sp.mask.shape == (2, 4, 6) and list(sp.mask.attrs["axis"]) == ["pol", "freq", "ra"] and list(mp.pol) == ["XX", "YY"]
    assert isinstance(mp, containers.RFIMask) and isinstance(sp, containers.SiderealRFIMask)
    ss = containers.SystemSensitivity(freq=freq, pol=pol, time=time)
    for name in ("measured", "radiometer", "weight"):
        assert getattr(ss, name).shape == (4, 2, 6) and getattr(ss, name).dtype == np.float32
    assert ss.frac_lost.shape == (4, 6) and np.array_equal(ss.freq, freq) and list(ss.pol) == ["XX", "YY"]
    out = containers.RFIMask(axes_from=ss, attrs_from=ss)
    assert out.mask.shape == (4, 6) and np.array_equal(out.time, time)


def _stream(gold, kind="time", n=None):
    freq, time = gold["sens/freq"], gold["sens/time"]
    n = len(time) if n is None else n
    if kind == "time":
        ts = containers.TimeStream(freq=freq, stack=3, time=time[:n])
    else:
        ts = containers.SiderealStream(freq=freq, stack=3, ra=np.linspace(0, 360, n, endpoint=False))
    ts.vis[:] = gold["rfimask/vis"][:, :, :n]
    ts.weight[:] = gold["rfimask/weight"][:, :, :n]
    return ts


def test_apply_host(gold):
    freq, time = gold["sens/freq"], gold["sens/time"]
    ts = _stream(gold)
    rm = containers.RFIMask(freq=freq, time=time)
    rm.mask[:] = gold["apply/mask"]
    w0 = np.array(ts.weight[:])
    res = flagging.ApplyTimeFreqMask(share="none").process(ts, rm)
    assert res is not ts and res.vis is not ts.vis and np.array_equal(ts.weight[:], w0)
    assert np.array_equal(res.weight[:], gold["apply/time/weight"])
    res = flagging.ApplyRFIMask(share="vis").process(ts, rm)
    assert res.vis is ts.vis and res.weight is not ts.weight and np.array_equal(ts.weight[:], w0)
    assert np.array_equal(res.weight[:], gold["apply/time/weight"])
    lo, hi = gold["apply/time_sub/range"]
    sub = containers.RFIMask(freq=freq, time=time[lo:hi])
    sub.mask[:] = gold["apply/mask"][:, lo:hi]
    res = flagging.ApplyTimeFreqMask(share="none", match_axes=False).process(ts, sub)
    assert np.array_equal(res.weight[:], gold["apply/time_sub/weight"])
    res = flagging.ApplyTimeFreqMask().process(ts, rm)  # share="all": in place
    assert res is ts and np.array_equal(ts.weight[:], gold["apply/time/weight"])
    ss = _stream(gold, "ra")
    rp = containers.SiderealRFIMaskByPol(freq=freq, ra=ss.ra, pol=np.array(["XX", "YY"]))
    rp.mask[:] = gold["apply/mask_pol"]
    res = flagging.ApplyTimeFreqMask(share="none", collapse_pol=True).process(ss, rp)
    assert np.array_equal(res.weight[:], gold["apply/ra_pol/weight"])
    hs = containers.HybridVisStream(pol=np.array(["XX", "YY"]), freq=freq, ew=3, el=2, ra=ss.ra)
    hs.weight[:] = gold["apply/hybrid/in"]
    res = flagging.ApplyTimeFreqMask(share="none").process(hs, rp)
    assert np.array_equal(res.weight[:], gold["apply/hybrid/weight"])


def test_apply_errors(gold):
    freq, time = gold["sens/freq"], gold["sens/time"]
    ts, ss = _stream(gold), _stream(gold, "ra")
    rm = containers.RFIMask(freq=freq, time=time)
    sm = containers.SiderealRFIMask(freq=freq, ra=ss.ra)
    task = flagging.ApplyTimeFreqMask()
    with pytest.raises(TypeError, match="timestream like"):
        task.process(ss, rm)
    with pytest.raises(TypeError, match="sidereal stream like"):
        task.process(ts, sm)
    with pytest.raises(TypeError, match="Require a RFIMask"):
        task.process(ts, ts)
    with pytest.raises(ValueError, match="different freq axes"):
        task.process(ts, containers.RFIMask(freq=freq + 1.0, time=time))
    with pytest.raises(ValueError, match="different time-like axes"):
        task.process(ts, containers.RFIMask(freq=freq, time=time + 1.0))
    with pytest.raises(ValueError, match="No overlapping samples"):
        flagging.ApplyTimeFreqMask(match_axes=False).process(ts, containers.RFIMask(freq=freq, time=time + 1.0))
    hs = containers.HybridVisStream(pol=np.array(["XX", "YY"]), freq=freq, ew=3, el=2, ra=ss.ra)
    rp = containers.SiderealRFIMaskByPol(freq=freq, ra=ss.ra, pol=np.array(["YY", "XX"]))
    with pytest.raises(ValueError, match="different pol axes"):
        task.process(hs, rp)
    with pytest.raises(ValueError, match="share"):
        flagging.ApplyTimeFreqMask(share="some")


def test_size_errors():
    x, m = np.zeros((8, 8)), np.zeros((8, 8), dtype=bool)
    for size in ((4, 3), (3, 2), (0, 3)):
        with pytest.raises(ValueError, match="odd"):
            filters.medfilt(x, m, size)
    for size in ((257, 3), (255, 255), (3, 3, 3)):
        with pytest.raises(ValueError):
            filters.medfilt(x, m, size)
    with pytest.raises(ValueError, match="odd"):
        flagging.mad(x, m, base_size=(2, 3))
    with pytest.raises(ValueError, match="mask_type"):
        flagging.RFISensitivityMask(mask_type="median")
    t = flagging.RFISensitivityMask(nsigma_1d=None, win_f_1d=None, niter=3)
    t.setup()
    assert t.nsigma_1d is None and t.win_f_1d is None and np.allclose(t.threshold, 5.0 * 1.5 ** np.array([2, 1, 0]))
    assert t.MAD_TO_RMS == 1.4826 and flagging.ApplyRFIMask is flagging.ApplyTimeFreqMask
    assert t._static_rfi_mask_hook(np.arange(4.0)).all() and t._combine_st_mad_hook(np.arange(3.0), np.arange(4.0)).shape == (4, 3)
