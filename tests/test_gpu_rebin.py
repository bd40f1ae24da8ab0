"""GPU rebinner, gradient correction and direct interpolators (`csrc/rebin.hip`; `SiderealRebinner`,
`RebinGradientCorrection`, `SiderealRegridderNearest` / `Linear` / `Cubic`) against the long-double twin
(`tests/rebin_twin.py`) and against vectors produced by executing the reference (`tests/gen_golden_rebin.py` ->
tests/golden/rebin.npz).

Tolerances, the regridder's (`tests/test_gpu_regrid.py`).  The kernels work in float64 and round once, so against the
twin the bound is `4 * 2**-24` of the row's largest output (vis), the same relative bound element-wise with an identical
zero pattern (weight), `4 * 2**-24 * 360` absolute (effective_ra, and exactly float32(ra) where the weight is zero);
nsample is exact in uint16 and within `4 * 2**-24` as the hybrid stream's float32.  The reference multiplies in
complex64; its own distance from the twin, `e_ref` = max |reference - twin| / max |twin|, is measured by the generator
and stored per case; against the reference vectors the bound is `2 * e_ref + 4 * 2**-24`.  Measured `e_ref`:

    rebinner 1.9e-8 ... 7.8e-8, interpolators 3.2e-8 ... 1.0e-7 (nearest 0), with down_mix 8.1e-8 / 1.3e-7,
    gradient correction 5.0e-8 with float64 RA positions and 1.6e-6 ... 4.1e-6 with float32 effective_ra positions
    (the reference differences float32 coordinates there)
"""

import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EPS32 = 2.0**-24
LSD = 312
MODES = ("uniform", "inverse_variance")


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "rebin.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def mixgold():
    with np.load(os.path.join(GOLDEN, "regrid.npz")) as z:
        return {k: z[k] for k in z.files if k.startswith("task/")}


class _Observer:
    """Linear time map (and, for down_mix, the regridder fixture's feed mask, baselines and latitude)."""

    lmax = mmax = 4
    frequencies = np.array([600.0, 612.5])

    def __init__(self, gold, mixgold=None):
        self.t0, self.day = (float(v) for v in gold["obs"])
        if mixgold is not None:
            self.baselines, self.feedmask, self.latitude = mixgold["task/baselines"], mixgold["task/feedmask"], float(mixgold["task/obs"][2])

    def unix_to_lsd(self, t):
        return (np.asarray(t, dtype=np.float64) - self.t0) / self.day


def _stream(gold, lsd, vis, w, form="time", **axes):
    from draco_amd.core import containers

    obs = _Observer(gold)
    freq = _Observer.frequencies[: vis.shape[0]]
    if form == "time":
        data = containers.TimeStream(freq=freq, time=obs.t0 + lsd * obs.day, **(axes or {"stack": vis.shape[1]}))
    else:
        data = containers.SiderealStream(freq=freq, ra=(lsd - LSD) * 360.0, **(axes or {"stack": vis.shape[1]}))
    data.vis[:] = vis
    data.weight[:] = w
    data.attrs["lsd"] = LSD
    src = obs.unix_to_lsd(data.time) if form == "time" else LSD + data.ra / 360.0
    return data, src


def _check_vis(x, xt, ref, e_ref, what):
    x, xt, ref = (np.asarray(a).reshape(-1, a.shape[-1]) for a in (x, xt, ref))
    for k in range(x.shape[0]):
        err, top = np.abs(x[k] - xt[k]).max(), np.abs(xt[k]).max()
        print(f"{what} row {k}: vis err {err:.3e} of max {top:.3e} (bound {4 * EPS32 * top:.3e})")
        assert err <= 4 * EPS32 * top, (what, k)
    err = np.abs(x - ref).max() / np.abs(ref).max()
    bound = 2 * float(e_ref) + 4 * EPS32
    print(f"{what}: vs reference {err:.3e} (bound {bound:.3e})")
    assert err <= bound, what


def _check_weight(w, wt, ref, what):
    w, wt, ref = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (w, wt, ref))
    for name, other in (("twin", wt), ("reference", ref)):
        nz = other != 0
        rel = (np.abs(w - other)[nz] / np.abs(other[nz])).max() if nz.any() else 0.0
        print(f"{what}: weight vs {name} {rel:.3e} (bound {4 * EPS32:.3e})")
        assert np.all(np.abs(w - other) <= 4 * EPS32 * np.abs(other)), (what, name)
        assert np.array_equal(w == 0, other == 0), (what, name)


def _check_rebinned(sd, twin_out, gold, key, nra, what, hybrid=False):
    import torch

    tv, tw, tn, te = twin_out
    for name in ("vis", "vis_weight", "nsample", "effective_ra"):
        assert isinstance(sd.datasets[name]._dev_t, torch.Tensor) and sd.datasets[name]._host is None, f"{name} stays on the device"
    assert sd.vis.dtype == np.complex64 and sd.weight.dtype == np.float32 and sd.effective_ra.dtype == np.float32
    assert np.array_equal(sd.ra, np.linspace(0.0, 360.0, nra, endpoint=False))
    _check_vis(sd.vis[:], tv, gold[f"{key}/vis"], gold[f"{key}/e_ref"], what)
    w = sd.weight[:]
    _check_weight(w, tw, gold[f"{key}/vis_weight"], what)
    ns, ref_ns = sd.nsample[:], gold[f"{key}/nsample"]
    if hybrid:
        assert ns.dtype == np.float32
        assert np.all(np.abs(ns - ref_ns) <= 4 * EPS32 * np.abs(ref_ns)) and np.all(np.abs(ns.reshape(tn.shape) - tn) <= 4 * EPS32 * np.abs(tn)), what
    else:
        assert ns.dtype == np.uint16 and np.array_equal(ns, ref_ns), what
    era, ref_era = sd.effective_ra[:], gold[f"{key}/effective_ra"]
    e_t, e_r = np.abs(era.reshape(te.shape) - te).max(), np.abs(era.astype(np.float64) - ref_era).max()
    print(f"{what}: effective_ra vs twin {e_t:.3e}, vs reference {e_r:.3e} (bound {4 * EPS32 * 360:.3e})")
    assert e_t <= 4 * EPS32 * 360 and e_r <= 4 * EPS32 * 360, what
    centre = np.broadcast_to(sd.ra.astype(np.float32), era.shape)
    assert (w == 0).any() and np.array_equal(era[w == 0], centre[w == 0]), "the bin centre where the weight is zero"


@pytest.mark.parametrize("cname", ["c37", "c11", "c150", "c48", "c1100", "c2600"])
def test_rebinner_stream(gold, cname):
    import rebin_twin as twin
    from draco_amd.analysis.sidereal import SiderealRebinner
    from draco_amd.core import containers

    lsd, vis, w, nra = gold[f"rebin/{cname}/lsd"], gold[f"rebin/{cname}/vis"], gold[f"rebin/{cname}/weight"], int(gold[f"rebin/{cname}/samples"])
    for form in ["time"] + (["ra"] if cname == "c37" else []):
        for mode in MODES:
            data, src = _stream(gold, lsd, vis, w, form)
            t = SiderealRebinner(samples=nra, weight=mode)
            t.setup(_Observer(gold))
            sd = t.process(data)
            assert type(sd) is containers.SiderealStream and sd.vis.shape == vis.shape[:-1] + (nra,)
            assert sd.attrs["lsd"] == LSD and "tag" not in sd.attrs
            tw_out = twin.rebin_twin(vis.reshape(-1, len(lsd)), w.reshape(-1, len(lsd)), src, nra, float(LSD), mode)
            _check_rebinned(sd, tw_out, gold, f"rebin/{cname}/{form}/{mode}", nra, f"{cname}/{form}/{mode}")
            x, nw = sd.vis[:], sd.weight[:]
            zero_row = (0, 0) if vis.shape[0] == 2 else (0, 1)
            assert not x[zero_row].any() and not nw[zero_row].any(), "the all-zero-weight row comes out as exact zeros"


@pytest.mark.parametrize("cname", ["h37", "h11"])
def test_rebinner_hybrid(gold, cname):
    import rebin_twin as twin
    from draco_amd.analysis.sidereal import SiderealRebinner
    from draco_amd.core import containers

    lsd, vis, w, nra = gold[f"hybrid/{cname}/lsd"], gold[f"hybrid/{cname}/vis"], gold[f"hybrid/{cname}/weight"], int(gold[f"hybrid/{cname}/samples"])
    for mode in MODES:
        data = containers.HybridVisStream(pol=2, freq=_Observer.frequencies, ew=3, el=5, ra=gold[f"hybrid/{cname}/ra_axis"])
        data.vis[:] = vis
        data.weight[:] = w
        data.attrs["lsd"] = LSD
        sd = SiderealRebinner(samples=nra, weight=mode).process(data)
        assert type(sd) is containers.HybridVisStream and sd.vis.shape == (2, 2, 3, 5, nra) and sd.weight.shape == sd.nsample.shape == sd.effective_ra.shape == (2, 2, 3, nra)
        tw_out = twin.rebin_twin(vis.reshape(-1, len(lsd)), w.reshape(-1, len(lsd)), LSD + data.ra / 360.0, nra, float(LSD), mode)
        _check_rebinned(sd, tw_out, gold, f"hybrid/{cname}/{mode}", nra, f"{cname}/{mode}", hybrid=True)


def _gradient_streams(gold, gname):
    from draco_amd.core import containers

    def build(prefix):
        s = containers.SiderealStream(freq=_Observer.frequencies, stack=5, ra=gold["gradient/ra"])
        s.vis[:] = gold[f"{prefix}/vis"]
        s.weight[:] = gold[f"{prefix}/vis_weight"]
        if f"{prefix}/effective_ra" in gold:
            s.add_dataset("effective_ra")
            s.effective_ra[:] = gold[f"{prefix}/effective_ra"]
        return s

    s = build(f"gradient/{gname}/in")
    return s, (s if gname in ("self", "wrap") else build(f"gradient/{gname}/ref"))


@pytest.mark.parametrize("gname", ["self", "fixed_ra", "other_mask", "equal_positions", "wrap"])
def test_gradient_correction(gold, gname):
    import rebin_twin as twin
    from draco_amd.analysis.sidereal import RebinGradientCorrection

    s, ref = _gradient_streams(gold, gname)
    flat = lambda ds: np.array(ds[:]).reshape(-1, 48)  # noqa: E731
    pos = flat(ref.effective_ra) if "effective_ra" in ref else np.asarray(ref.ra)
    assert (gname == "fixed_ra") == (pos.ndim == 1)
    w_in = flat(s.weight)
    tv, tw = twin.gradient_twin(flat(s.vis), w_in, flat(s.effective_ra), s.ra, flat(ref.vis), flat(ref.weight), pos)
    t = RebinGradientCorrection()
    t.setup(ref)
    out = t.process(s)
    assert out is s and "effective_ra" not in s and s.vis.on_device and s.weight.on_device and s.vis._host is None
    x, nw = flat(s.vis), flat(s.weight)
    _check_vis(x, tv, gold[f"gradient/{gname}/vis"], gold[f"gradient/{gname}/e_ref"], gname)
    ref_w = gold[f"gradient/{gname}/vis_weight"].reshape(-1, 48)
    assert np.array_equal(nw, ref_w) and np.array_equal(nw, tw.astype(np.float32)), "the weight is kept or zeroed, nothing else"
    assert (nw == 0).sum() > (w_in == 0).sum() and np.array_equal(nw[0], w_in[0]) and not w_in[0].any()
    assert np.array_equal(x[0], gold[f"gradient/{gname}/in/vis"].reshape(-1, 48)[0]), "a fully masked row is untouched"
    if gname == "equal_positions":  # the two gradients that divide by an interval of zero length are flagged
        assert nw[1, 19] == 0 and nw[1, 20] == 0 and nw[7, 0] == 0 and nw[7, 1] == 0
    if gname == "wrap":  # a flagged first sample flags the last one's gradient, and the other way round
        assert w_in[1, 0] == 0 and nw[1, 47] == 0 and w_in[2, 47] == 0 and nw[2, 0] == 0


@pytest.mark.parametrize("cname", ["c37", "c11", "c150", "c48", "c1100"])
def test_interpolators(gold, cname):
    import rebin_twin as twin
    from draco_amd.analysis import sidereal

    lsd, vis, w, nra = gold[f"rebin/{cname}/lsd"], gold[f"rebin/{cname}/vis"], gold[f"rebin/{cname}/weight"], int(gold[f"rebin/{cname}/samples"])
    classes = {"nearest": sidereal.SiderealRegridderNearest, "linear": sidereal.SiderealRegridderLinear, "cubic": sidereal.SiderealRegridderCubic}
    for kind, cls in classes.items():
        t = cls(samples=nra)
        t.start, t.end = LSD, LSD + 1
        grid, v, nw = t._regrid(np.ascontiguousarray(vis), np.ascontiguousarray(w), lsd)
        assert v.is_cuda and nw.is_cuda and tuple(v.shape) == vis.shape[:-1] + (nra,)
        v, nw = v.cpu().numpy(), nw.cpu().numpy()
        key = f"interp/{cname}/{kind}"
        assert np.array_equal(grid, gold[f"{key}/grid"])
        tv, tw = twin.interp_twin(kind, vis.reshape(-1, len(lsd)), w.reshape(-1, len(lsd)), lsd, nra, float(LSD), float(LSD + 1))
        _check_vis(v, tv, gold[f"{key}/vis"], gold[f"{key}/e_ref"], f"{cname}/{kind}")
        _check_weight(nw, tw, gold[f"{key}/vis_weight"], f"{cname}/{kind}")
        if kind == "nearest":
            assert np.array_equal(v, gold[f"{key}/vis"]) and np.array_equal(nw, gold[f"{key}/vis_weight"]), "nearest copies"
        if cname == "c150":  # the kept samples cover [10:120] of 150: the ends of the day are flagged
            assert not nw[..., :3].any() and not nw[..., -10:].any() and nw[1, 1].any()


@pytest.mark.parametrize("kind", ["linear", "cubic"])
def test_down_mix(gold, mixgold, kind):
    import regrid_twin
    import rebin_twin as twin
    from draco_amd.analysis import sidereal

    lsd, vis, w = gold["mix/lsd"], gold["mix/vis"], gold["mix/weight"]
    prod = mixgold["task/prodstack"]
    data, src = _stream(gold, lsd, vis, w, "time", prod=prod, input=4)
    obs = _Observer(gold, mixgold)
    cls = {"linear": sidereal.SiderealRegridderLinear, "cubic": sidereal.SiderealRegridderCubic}[kind]
    t = cls(samples=64, down_mix=True)
    t.setup(obs)
    sd = t.process(data)
    assert sd.vis.on_device and sd.vis._host is None and sd.attrs["tag"] == "lsd_312"
    fm = obs.feedmask[prod["input_a"], prod["input_b"]]
    pin = regrid_twin.fringe_phase(data.freq, obs.baselines[:, 0], fm, obs.latitude, src).reshape(8, -1)
    pout = regrid_twin.fringe_phase(data.freq, obs.baselines[:, 0], fm, obs.latitude, LSD + np.arange(64) / 64).reshape(8, -1)
    tv, tw = twin.interp_twin(kind, vis.reshape(8, -1), w.reshape(8, -1), src, 64, float(LSD), float(LSD + 1), pin, pout)
    _check_vis(sd.vis[:], tv, gold[f"mix/{kind}/vis"], gold[f"mix/{kind}/e_ref"], f"mix/{kind}")
    _check_weight(sd.weight[:], tw, gold[f"mix/{kind}/vis_weight"], f"mix/{kind}")
    assert not sd.vis[:][:, 2].any() and not sd.weight[:][:, 2].any(), "the baseline with a masked feed is flagged"


def test_two_runs_are_bit_identical(gold):
    from draco_amd.analysis.sidereal import RebinGradientCorrection, SiderealRebinner

    lsd, vis, w = gold["rebin/c1100/lsd"], gold["rebin/c1100/vis"], gold["rebin/c1100/weight"]
    runs = []
    for _ in range(2):
        data, _src = _stream(gold, lsd, vis, w)
        t = SiderealRebinner(samples=512)
        t.setup(_Observer(gold))
        sd = t.process(data)
        first = [np.array(sd.datasets[k][:]) for k in ("vis", "vis_weight", "nsample", "effective_ra")]
        g = RebinGradientCorrection()
        g.setup(sd)
        g.process(sd)
        runs.append(first + [np.array(sd.vis[:]), np.array(sd.weight[:])])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    assert np.abs(runs[0][0]).max() > 0 and not np.array_equal(runs[0][0], runs[0][4])


def test_chain_rebin_correct_stack_mmodes(gold):
    """TimeStream -> SiderealRebinner -> RebinGradientCorrection (on itself) -> SiderealStacker, twice -> MModeTransform:
    everything stays on the device, and two identical days stack to the twin's rebinned, corrected day."""
    import torch

    import rebin_twin as twin
    from draco_amd.analysis.sidereal import RebinGradientCorrection, SiderealRebinner, SiderealStacker
    from draco_amd.analysis.transform import MModeTransform

    lsd, vis, w, nra = gold["rebin/c150/lsd"], gold["rebin/c150/vis"], gold["rebin/c150/weight"], 64
    stacker = SiderealStacker()
    for _ in range(2):
        data, src = _stream(gold, lsd, vis, w)
        rb = SiderealRebinner(samples=nra)
        rb.setup(_Observer(gold))
        sd = rb.process(data)
        gc = RebinGradientCorrection()
        gc.setup(sd)
        sd = gc.process(sd)
        assert sorted(sd.datasets) == ["nsample", "vis", "vis_weight"] and all(ds.on_device for ds in sd.datasets.values())
        stacker.process(sd)
    stack = stacker.process_finish()
    assert all(isinstance(ds._dev_t, torch.Tensor) for ds in stack.datasets.values())
    mm = MModeTransform()
    mm.setup(None)
    m = mm.process(stack)
    assert m.vis.on_device and torch.isfinite(torch.view_as_real(m.vis._dev)).all()

    tv, tw, tn, te = twin.rebin_twin(vis.reshape(10, -1), w.reshape(10, -1), src, nra, float(LSD), "inverse_variance")
    # the correction reads the rebinned day as the device holds it: complex64 / float32 datasets
    tv32, tw32, te32 = tv.astype(np.complex64), tw.astype(np.float32), te.astype(np.float32)
    cv, cw = twin.gradient_twin(tv32, tw32, te32, np.linspace(0, 360, nra, endpoint=False), tv32, tw32, te32)
    cv = cv * (cw > 0)  # a sample without weight adds nothing to the stack: its mean stays zero
    x, nw = stack.vis[:].reshape(10, -1), stack.weight[:].reshape(10, -1)
    for k in range(10):
        err, top = np.abs(x[k] - cv[k]).max(), np.abs(cv[k]).max()
        print(f"chain row {k}: err {err:.3e} of max {top:.3e} (bound {4 * EPS32 * top:.3e})")
        assert err <= 4 * EPS32 * top, k
    assert np.all(np.abs(nw - 2 * cw) <= 4 * EPS32 * 2 * cw) and np.array_equal(nw == 0, cw == 0), "two equal days: twice the weight"
    assert np.array_equal(stack.nsample[:].reshape(10, -1), 2 * np.floor(tn).astype(np.uint16) * (cw > 0))
    assert list(stack.attrs["lsd"]) == [LSD, LSD]
