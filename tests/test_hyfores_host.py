"""Host side of the stored-filter apply and the HyFoReS bandpass tasks: the NumPy twin (`tests/hyfores_twin.py`) against
the vectors produced by executing the reference (`tests/gen_golden_hyfores.py` -> tests/golden/hyfores.npz and
hyfores_apply.npz), `compensate_window`, the new containers, and the configuration and mismatch errors that are raised
before the device is touched.

The twin's float64 form agrees with every reference vector within `3 e_ref` of the vector's largest modulus, plus the
floor of the dataset's storage (`2**-22` for complex64 / float32, `2**-51` for float64) or, for `bandpass` and `window`,
the float64 summation bound `allow` of the truth form.
"""

import os

import numpy as np
import pytest

import hyfores_twin as twin
from conftest import GOLDEN

FLOOR = {"vis": 2.0**-22, "weight": 2.0**-22, "freq_cov": 2.0**-51}
ESTIMATES = [("Y33", k) for k in twin.KINDS] + [("Y70", twin.KINDS[0]), ("Y6", twin.KINDS[2])]
APPLIES = [("Y33", "apply", dict(calculate_cov=True)), ("Y70", "apply", dict(atten=True)), ("Y6", "apply", {})]
CLEANS = [("Y33", "clean", dict(calculate_cov=True)), ("Y33", "clean0", {}), ("Y70", "clean", dict(atten=True))]


@pytest.fixture(scope="module")
def gold():
    out = {}
    for name in ("hyfores.npz", "hyfores_apply.npz"):
        with np.load(os.path.join(GOLDEN, name)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def _close(label, got, ref, e_ref, floor):
    err = float(np.abs(got - ref).max())
    top = float(np.abs(ref).max())
    print(f"hyfores twin {label}: |twin - ref| {err:.3e} of {top:.3e}, e_ref {e_ref:.3e}")
    assert err <= 3 * e_ref * top + floor, (label, err, e_ref, top)


@pytest.mark.parametrize("name,kind", ESTIMATES)
def test_twin_estimate(gold, name, kind):
    c = twin.case(gold, name)
    got, t = twin.estimator(kind, c), twin.estimator(kind, c, truth=True)
    for ds, k in (("bandpass", "y"), ("window", "W")):
        assert np.all(np.abs(got[k] - t[k]) <= t[f"allow_{k}"])
        _close(f"{name} {kind} {ds}", got[k], gold[f"{name}/{kind}/{ds}"], float(gold[f"{name}/{kind}/e_ref_{ds}"]), float(t[f"allow_{k}"].max()))
    zero = t["D"] == 0
    assert not got["y"][zero].any() and not got["W"][zero].any()
    if name == "Y33" and "Mask" in kind:
        assert zero[1, :, 12].all()  # the masked (pol, freq) plane


@pytest.mark.parametrize("name,label,cfg", APPLIES)
def test_twin_apply(gold, name, label, cfg):
    c = twin.case(gold, name)
    atten = c["atten_threshold"] if cfg.get("atten") else 0.0
    v, w, cov, st = twin.apply_filter(c["vis"], c["weight"], c["filter"], atten_threshold=atten, calculate_cov=cfg.get("calculate_cov", False))
    key = f"{name}/{label}"
    _close(f"{key} vis", twin.at_positions("vis", v, c["pos"]), gold[f"{key}/vis"], float(gold[f"{key}/e_ref_vis"]), FLOOR["vis"] * np.abs(gold[f"{key}/vis"]).max())
    _close(f"{key} weight", w, gold[f"{key}/weight"], float(gold[f"{key}/e_ref_weight"]), FLOOR["weight"] * gold[f"{key}/weight"].max())
    assert np.array_equal(w == 0, gold[f"{key}/weight"] == 0)
    if cov is not None:
        ref = gold[f"{key}/freq_cov"]
        _close(f"{key} freq_cov", twin.at_positions("freq_cov", cov, c["pos"]), ref, float(gold[f"{key}/e_ref_freq_cov"]), FLOOR["freq_cov"] * np.abs(ref).max())
    keep = np.isin(st, (twin.SKIPPED, twin.MISSING_FREQ))[:, None, :, None, :]
    assert np.array_equal(np.where(keep, v, 0), np.where(keep, c["vis"], 0))
    if name == "Y33":
        assert {int(s) for s in np.unique(st)} == {twin.OK, twin.SKIPPED, twin.ZERO_FILTER, twin.MISSING_FREQ}
        assert st[0, 0, 5] == twin.MISSING_FREQ and st[1, 0, 5] == twin.OK  # the flags are per polarisation


@pytest.mark.parametrize("name,label,cfg", CLEANS)
def test_twin_clean_and_compensate_window(gold, name, label, cfg):
    from draco_amd.analysis.hyforesbandpass import compensate_window

    c = twin.case(gold, name)
    key, kind = f"{name}/{label}", twin.KINDS[0]
    y, w = gold[f"{name}/{kind}/bandpass"], gold[f"{name}/{kind}/window"]
    cutoff, allow_g = float(gold[f"{key}/cutoff"]), float(gold[f"{key}/allow_g"])
    for fn in (compensate_window, twin.compensate_window):
        g, sval, rank = fn(w, y, cutoff)
        assert np.array_equal(rank, gold[f"{key}/rank"])
        assert np.abs(g - gold[f"{key}/comp_bandpass"]).max() <= allow_g and np.abs(sval - gold[f"{key}/sval"]).max() <= allow_g
        if cutoff == 0.0:
            assert g is y and not sval.any() and not rank.any()
    atten = c["atten_threshold"] if cfg.get("atten") else 0.0
    v, wt, cov, _ = twin.apply_filter(c["vis"], c["weight"], c["filter"], gain=g, atten_threshold=atten, calculate_cov=cfg.get("calculate_cov", False))
    _close(f"{key} vis", twin.at_positions("vis", v, c["pos"]), gold[f"{key}/vis"], float(gold[f"{key}/e_ref_vis"]), FLOOR["vis"] * np.abs(gold[f"{key}/vis"]).max())
    _close(f"{key} weight", wt, gold[f"{key}/weight"], float(gold[f"{key}/e_ref_weight"]), FLOOR["weight"] * gold[f"{key}/weight"].max())
    assert np.array_equal(wt == 0, gold[f"{key}/weight"] == 0)
    if cov is not None:
        ref = gold[f"{key}/freq_cov"]
        _close(f"{key} freq_cov", twin.at_positions("freq_cov", cov, c["pos"]), ref, float(gold[f"{key}/e_ref_freq_cov"]), FLOOR["freq_cov"] * np.abs(ref).max())


def test_golden_conditions(gold):
    for k, v in gold.items():
        if "/e_ref_" in k:
            assert float(v) <= 1e-3, k
    for name in ("hyfores.npz", "hyfores_apply.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, name)) < (1 << 20)
    c = twin.case(gold, "Y33")
    assert twin.el_mask(c["el"], c["freq"], c["min_ysep"]).tolist() == [False, True, True, True, False]
    assert c["mask"][1, 12].all() and 0.05 < c["mask"].mean() < 0.2 and (c["mask"] & c["masks"]).any()
    assert gold["Y33/vis_q"].dtype == np.int16 and gold["Y33/pf_vis_q"].dtype == np.int8


def test_containers():
    from draco_amd.core import containers

    freq = 600.0 + np.arange(6)
    m = containers.RingMapMask(pol=np.array(["XX", "YY"]), freq=freq, ra=8, el=np.linspace(-1, 1, 3))
    assert m.mask.shape == (2, 6, 8, 3) and m.mask.dtype == np.bool_ and not m.mask[:].any()
    for cls, names, shapes in (
        (containers.VisBandpassWindow, ("bandpass", "window"), ((2, 6), (2, 6, 6))),
        (containers.VisBandpassCompensate, ("comp_bandpass", "sval"), ((2, 6), (2, 6))),
    ):
        c = cls(pol=2, freq=freq)
        for n, s in zip(names, shapes):
            assert c.datasets[n].shape == s and c.datasets[n].dtype == np.complex128 and getattr(c, n) is c.datasets[n]
    w = containers.VisBandpassWindowBaseline(pol=2, ew=4, freq=freq)
    assert w.bandpass.shape == (2, 4, 6) and w.window.shape == (2, 4, 6, 6) and w.window.dtype == np.complex128
    assert isinstance(w, containers.VisBandpassWindow) and np.array_equal(w.freq, freq)
    g = containers.VisBandpassCompensateBaseline(pol=2, ew=4, freq=freq)
    assert g.comp_bandpass.shape == (2, 4, 6) and g.sval.shape == (2, 4, 6) and g.sval.dtype == np.complex128
    g.attrs["rank"], g.attrs["cutoff"] = np.zeros((2, 4)), 0.1
    assert isinstance(g, containers.VisBandpassCompensate)


def _streams(**change):
    from draco_amd.core import containers

    axes = dict(pol=np.array(["XX", "YY"]), freq=600.0 + np.arange(4), ew=2, el=np.linspace(-1, 1, 3), ra=5)
    hv = containers.HybridVisStream(**axes)
    axes.update(change)
    src = containers.HybridVisStream(**axes)
    src.add_dataset("filter", allocate=True)
    return hv, src


def test_config_and_mismatch_errors():
    from draco_amd.analysis import dayenu, hyforesbandpass as hy
    from draco_amd.core import containers

    a = dayenu.ApplyDelayFilterHybridVis()
    assert (a.atten_threshold, a.calculate_cov, a.copy_weight, a.copy_tag) == (0.0, False, False, False)
    a = dayenu.ApplyDelayFilterHybridVis(atten_threshold=0.1, calculate_cov=True, copy_weight=True, copy_tag=True)
    assert a.copy_weight and a.copy_tag and a.calculate_cov and a.atten_threshold == 0.1
    with pytest.raises(AttributeError):
        dayenu.ApplyDelayFilterHybridVis(cutoff=0.1)
    clean = hy.DelayFilterHyFoReSBandpassHybridVisClean()
    assert (clean.cutoff, clean.atten_threshold, clean.calculate_cov) == (0.1, 0.0, False)
    for kind in twin.KINDS:
        t = getattr(hy, kind)(atten_threshold=0.2)
        assert t.atten_threshold == 0.2 and isinstance(t, hy.DelayFilterHyFoReSBandpassHybridVis)
        with pytest.raises(AttributeError):
            getattr(hy, kind)(cutoff=0.1)
    with pytest.raises(NotImplementedError):
        dayenu.DayenuDelayFilterFixedCutoff()
    single = dayenu.ApplyDelayFilterHybridVisSingleSource()
    changes = (
        (dict(freq=601.0 + np.arange(4)), "Frequencies do not match"),
        (dict(el=np.linspace(-0.5, 0.5, 3)), "Elevations do not match"),
        (dict(ew=np.array([0, 2])), "EW baselines do not match"),
        (dict(pol=np.array(["XX", "XY"])), "Polarisations do not match"),
        (dict(ra=np.linspace(1.0, 361.0, 5, endpoint=False)), "Right Ascension do not match"),
    )
    est = hy.DelayFilterHyFoReSBandpassHybridVis()
    est.min_ysep = 0.3
    for change, msg in changes:
        hv, src = _streams(**change)
        with pytest.raises(ValueError, match=msg):
            dayenu.ApplyDelayFilterHybridVis().process(hv, src)
        single.setup(src)
        with pytest.raises(ValueError, match=msg):
            single.process(hv)
        with pytest.raises(ValueError, match=msg):
            est.process(hv, src)
        with pytest.raises(ValueError, match=msg):
            clean.process(hv, src, None)
    # a stream without a filter, and complex filters
    hv, src = _streams()
    del src["filter"]
    with pytest.raises(KeyError, match="filter"):
        dayenu.ApplyDelayFilterHybridVis().process(hv, src)
    src.datasets["complex_filter"] = containers.Dataset(host=np.zeros((2, 4, 4, 2, 5), dtype=np.complex128))
    for call in (lambda: dayenu.ApplyDelayFilterHybridVis().process(hv, src), lambda: est.process(hv, src), lambda: clean.process(hv, src, None),
                 lambda: hy.HyFoReSBandpassHybridVis().process(src, hv)):
        with pytest.raises(NotImplementedError, match="complex"):
            call()

    class Comm:
        size = 2

    hv, src = _streams()
    hv.comm = Comm()
    with pytest.raises(NotImplementedError, match="one process"):
        est.process(hv, src)


def test_horizon_limit_and_setup():
    from draco_amd.analysis import hyforesbandpass as hy

    t = hy.HyFoReSBandpassHybridVisMask()
    t.min_ysep = 0.3048
    assert t.get_horizon_limit(600.0) == pytest.approx(299792458.0 / (600e6 * 0.3048) - 1.0, rel=1e-15)
    hv, _ = _streams()
    assert np.array_equal(t.aliased_el_mask(hv), np.abs(hv.index_map["el"]) < t.get_horizon_limit(603.0))

    class Telescope:  # two feeds one unit apart north-south, and one a cylinder over
        baselines = np.array([[0.0, 0.0], [0.0, 0.5], [22.0, 0.0], [22.0, 0.5], [0.0, 1.0]])
        lmax = mmax = 1
        frequencies = np.array([600.0])

    t.setup(Telescope())
    assert t.min_ysep == pytest.approx(0.5)
