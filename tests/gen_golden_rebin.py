"""Generate tests/golden/rebin.npz by EXECUTING the reference's own ``rebin_matrix``, ``grad_1d``,
``SiderealRebinner.process``, ``RebinGradientCorrection.process`` and the ``_regrid`` of ``SiderealRegridderNearest`` /
``Linear`` / ``Cubic`` from source (through ``oracle._refstub``), on stand-in containers.  Only the data is committed;
run where the reference checkout exists:

    python tests/gen_golden_rebin.py

Per case the file records ``e_ref`` = max |reference - twin| / max |twin| of the visibilities (``tests/rebin_twin.py``):
the reference multiplies visibilities and weights in complex64, and differences float32 positions in the gradient
correction; the tests' tolerance against the reference vectors is built from that measured distance.

``nsample`` is compared exactly, and a uint16 store truncates: the generator asserts that every positive bin sum of
every stream case either is the same exact integer summed in either order or lies more than 1e-6 from any integer,
and refuses to write the file otherwise.
"""

import importlib
import os
import sys
import types

import numpy as np
import scipy.constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rebin_twin as twin  # noqa: E402
import regrid_twin  # noqa: E402
from gen_golden_regrid import DS, Observer, make_task  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
LSD = 312
CADENCE = 0.0137  # offset of the first sample, in bins


class Fake:
    """Stand-in for TimeStream / SiderealStream / HybridVisStream."""

    last = "ra"
    lead = ("freq", "stack")
    wlead = ("freq", "stack")
    ns_dtype = np.uint16

    def __init__(self, ra=None, axes_from=None, attrs_from=None, **axes):
        self.index_map = {k: v for k, v in (axes_from.index_map.items() if axes_from is not None else ()) if k not in ("time", "ra")}
        self.index_map.update({k: np.asarray(v) for k, v in axes.items()})
        if ra is not None:
            self.index_map["ra"] = np.linspace(0.0, 360.0, ra, endpoint=False) if isinstance(ra, int) else np.asarray(ra, dtype=np.float64)
        self.attrs = dict(attrs_from.attrs) if attrs_from is not None else {}
        self.prodstack = getattr(axes_from, "prodstack", None)
        self.datasets = {}
        self.add_dataset("vis")
        self.add_dataset("vis_weight")

    def add_dataset(self, name):
        axes, dt = {
            "vis": (self.lead + (self.last,), np.complex64),
            "vis_weight": (self.wlead + (self.last,), np.float32),
            "nsample": (self.wlead + (self.last,), self.ns_dtype),
            "effective_ra": (self.wlead + (self.last,), np.float32),
        }[name]
        self.datasets[name] = DS(np.zeros([len(self.index_map[a]) for a in axes], dtype=dt), axes)

    def _get(self, name):
        if name in self.datasets:
            return self.datasets[name]
        raise KeyError(f"Dataset '{name}' not initialised.")

    vis = property(lambda s: s.datasets["vis"])
    weight = property(lambda s: s.datasets["vis_weight"])
    nsample = property(lambda s: s._get("nsample"))
    effective_ra = property(lambda s: s._get("effective_ra"))
    ra = property(lambda s: s.index_map["ra"])
    time = property(lambda s: s.index_map["time"])
    freq = property(lambda s: s.index_map["freq"])

    def __delitem__(self, name):
        del self.datasets[name]

    def redistribute(self, axis):
        pass


class FakeTime(Fake):
    last = "time"


class FakeSidereal(Fake):
    pass


class FakeHybrid(Fake):
    lead = ("pol", "freq", "ew", "el")
    wlead = ("pol", "freq", "ew")
    ns_dtype = np.float32


def cadence(nt, nra, keep=None):
    """Sample LSDs: LSD + CADENCE / nra + k 1.003 / nt, kept while inside the day."""
    t = LSD + CADENCE / nra + np.arange(nt) * 1.003 / nt
    t = t[t < LSD + 1]
    return t[keep] if keep is not None else t


def make_data(rng, lsd, lead, wlead, special=True):
    """Smooth fringes plus noise; weights with 20 % zeros, weight row 0 all zero, one row with a single sample."""
    nt = len(lsd)
    x = (lsd - LSD)[None, :]
    nrow, nw = int(np.prod(lead)), int(np.prod(wlead))
    fr, ph, am = rng.uniform(1.0, 6.0, (nrow, 1)), rng.uniform(0, 2 * np.pi, (nrow, 1)), rng.uniform(0.5, 2.0, (nrow, 1))
    vis = am * np.exp(1j * (2 * np.pi * fr * x + ph)) + 0.05 * (rng.normal(size=(nrow, nt)) + 1j * rng.normal(size=(nrow, nt)))
    w = rng.uniform(0.5, 2.0, (nw, nt)).astype(np.float32)
    w[rng.uniform(size=w.shape) < 0.2] = 0.0
    if special:
        w[0] = 0.0
        w[nw - 2] = 0.0
        w[nw - 2, nt // 2] = 1.25
    return vis.astype(np.complex64).reshape(*lead, nt), w.reshape(*wlead, nt)


def check_nsample_safe(R, w, name):
    m = (w.reshape(-1, w.shape[-1]) > 0).astype(np.float64)
    nearest = np.inf
    for row in m:
        for g in range(R.shape[0]):
            nz = np.flatnonzero(R[g] * row)
            if not len(nz):
                continue
            fwd = bwd = 0.0
            for j in nz:
                fwd += R[g, j] * row[j]
            for j in nz[::-1]:
                bwd += R[g, j] * row[j]
            exact = fwd == bwd and fwd == np.round(fwd)
            dist = abs(fwd - np.round(fwd))
            if not exact:
                nearest = min(nearest, dist)
            assert exact or dist > 1e-6, f"{name}: bin {g} sums to {fwd!r}: within 1e-6 of an integer without being one"
    print(f"  {name}: smallest inexact distance of a bin count from an integer {nearest:.3e}")


def main():
    _refstub.load_reference()
    sidereal = importlib.import_module("draco.analysis.sidereal")
    ref_regrid = importlib.import_module("draco.util.regrid")
    sidereal.constants = types.SimpleNamespace(c=scipy.constants.c)
    sidereal.containers = types.SimpleNamespace(TimeStream=FakeTime, SiderealStream=FakeSidereal, HybridVisStream=FakeHybrid)
    sidereal.tools.invert_no_zero = _refstub._invert_no_zero

    out = {}
    rng = np.random.default_rng(20261019)
    t0, day = 1.6e9, 86164.0905
    freq2 = np.array([600.0, 612.5])
    out["lsd"], out["obs"] = np.array(LSD), np.array([t0, day])

    # ---- host functions
    for name, (nt, nra, wt) in {"m37": (37, 16, None), "m11": (11, 16, None), "m48": (48, 48, None), "m40_nearest": (40, 16, 0)}.items():
        lsd = cadence(nt, nra)
        target = np.linspace(LSD, LSD + 1, nra, endpoint=False)
        width_t = np.median(np.abs(np.diff(lsd))) if wt is None else wt
        out[f"matrix/{name}/tra"], out[f"matrix/{name}/ra"], out[f"matrix/{name}/width_t"] = lsd, target, np.array(width_t)
        out[f"matrix/{name}/R"] = ref_regrid.rebin_matrix(lsd, target, width_t=width_t)
    out["matrix/names"] = np.array(["m37", "m11", "m48", "m40_nearest"])
    n = 24
    si = np.sort(np.linspace(0, 360, n, endpoint=False) + rng.uniform(0, 10, n))
    si[7] = si[6]  # two equal adjacent positions
    x = (np.exp(2j * np.pi * si / 360) + 0.1 * rng.normal(size=n)).astype(np.complex128)
    mask = rng.uniform(size=n) < 0.15
    for key, per in (("periodic", 360.0), ("open", None)):
        g, mk = ref_regrid.grad_1d(x.copy(), si.copy(), mask.copy(), period=per)
        out[f"grad/{key}/grad"], out[f"grad/{key}/mask"] = g, mk
    out["grad/x"], out["grad/si"], out["grad/mask"] = x, si, mask

    # ---- SiderealRebinner.process
    cases = {"c37": (37, 16, None, (2, 5)), "c11": (11, 16, None, (2, 5)), "c150": (150, 64, slice(10, 120), (2, 5)), "c48": (48, 48, None, (2, 5)),
             "c1100": (1100, 512, None, (1, 3)), "c2600": (2600, 64, None, (1, 3))}
    names = []
    rebinned = {}
    for cname, (nt, nra, keep, lead) in cases.items():
        lsd = cadence(nt, nra, keep)
        vis, w = make_data(rng, lsd, lead, lead, special=lead == (2, 5))
        if lead == (1, 3):
            w[0, 1] = 0.0
        out[f"rebin/{cname}/lsd"], out[f"rebin/{cname}/vis"], out[f"rebin/{cname}/weight"], out[f"rebin/{cname}/samples"] = lsd, vis, w, np.array(nra)
        forms = ["time"] + (["ra"] if cname == "c37" else [])
        for form in forms:
            for mode in ("uniform", "inverse_variance"):
                if form == "time":
                    data = FakeTime(freq=freq2[: lead[0]], stack=np.arange(lead[1]), time=t0 + lsd * day)
                else:
                    data = FakeSidereal(freq=freq2[: lead[0]], stack=np.arange(lead[1]), ra=(lsd - LSD) * 360.0)
                data.attrs["lsd"] = LSD
                data.vis[:] = vis
                data.weight[:] = w
                task = make_task(sidereal.SiderealRebinner, samples=nra, weight=mode, observer=Observer(0, None, None, 0.0, t0, day))
                sd = task.process(data)
                src = task.observer.unix_to_lsd(data.time) if form == "time" else LSD + data.ra / 360.0
                if mode == "uniform":
                    R = ref_regrid.rebin_matrix(src, np.linspace(LSD, LSD + 1, nra, endpoint=False), width_t=np.median(np.abs(np.diff(src))))
                    check_nsample_safe(R, w, f"{cname}/{form}")
                tv, tw, tn, te = twin.rebin_twin(vis.reshape(-1, len(lsd)), w.reshape(-1, len(lsd)), src, nra, float(LSD), mode)
                rv = np.asarray(sd.vis[:]).reshape(tv.shape)
                e_ref = np.abs(rv - tv).max() / np.abs(tv).max()
                key = f"rebin/{cname}/{form}/{mode}"
                print(f"{key}: e_ref={e_ref:.3e} weight rel={np.abs(np.asarray(sd.weight[:]).reshape(tw.shape) - tw).max() / tw.max():.3e} "
                      f"era abs={np.abs(np.asarray(sd.effective_ra[:]).reshape(te.shape) - te).max():.3e} nsample max {np.asarray(sd.nsample[:]).max()}")
                assert np.array_equal(np.asarray(sd.nsample[:]).reshape(tn.shape), np.floor(tn).astype(np.uint16)), "the twin's counts differ from the reference's"
                for k in ("vis", "vis_weight", "nsample", "effective_ra"):
                    out[f"{key}/{k}"] = np.asarray(sd.datasets[k][:])
                out[f"{key}/e_ref"] = e_ref
                if form == "ra":
                    out[f"rebin/{cname}/ra_axis"] = np.asarray(data.ra)
                rebinned[(cname, form, mode)] = sd
        names.append(cname)
    out["rebin/names"] = np.array(names)

    # ---- hybrid form
    for cname, (nt, nra) in {"h37": (37, 16), "h11": (11, 16)}.items():
        lsd = cadence(nt, nra)
        vis, w = make_data(rng, lsd, (2, 2, 3, 5), (2, 2, 3))
        out[f"hybrid/{cname}/lsd"], out[f"hybrid/{cname}/vis"], out[f"hybrid/{cname}/weight"], out[f"hybrid/{cname}/samples"] = lsd, vis, w, np.array(nra)
        for mode in ("uniform", "inverse_variance"):
            data = FakeHybrid(pol=np.arange(2), freq=freq2, ew=np.arange(3), el=np.arange(5), ra=(lsd - LSD) * 360.0)
            data.attrs["lsd"] = LSD
            data.vis[:] = vis
            data.weight[:] = w
            sd = make_task(sidereal.SiderealRebinner, samples=nra, weight=mode).process(data)
            tv, tw, tn, te = twin.rebin_twin(vis.reshape(-1, len(lsd)), w.reshape(-1, len(lsd)), LSD + data.ra / 360.0, nra, float(LSD), mode)
            e_ref = np.abs(np.asarray(sd.vis[:]).reshape(tv.shape) - tv).max() / np.abs(tv).max()
            print(f"hybrid/{cname}/{mode}: e_ref={e_ref:.3e}")
            for k in ("vis", "vis_weight", "nsample", "effective_ra"):
                out[f"hybrid/{cname}/{mode}/{k}"] = np.asarray(sd.datasets[k][:])
            out[f"hybrid/{cname}/{mode}/e_ref"] = e_ref
        out[f"hybrid/{cname}/ra_axis"] = np.asarray(data.ra)
    out["hybrid/names"] = np.array(["h37", "h11"])

    # ---- RebinGradientCorrection.process on the rebinned 48 -> 48 day
    def clone(sd, with_era=True):
        c = FakeSidereal(ra=np.asarray(sd.ra), axes_from=sd, attrs_from=sd)
        c.vis[:] = sd.vis[:]
        c.weight[:] = sd.weight[:]
        if with_era:
            c.add_dataset("effective_ra")
            c.effective_ra[:] = sd.effective_ra[:]
        return c

    base = rebinned[("c48", "time", "inverse_variance")]
    gnames = []
    for gname in ("self", "fixed_ra", "other_mask", "equal_positions", "wrap"):
        s = clone(base)
        if gname == "wrap":  # flagged first and last samples: the wrapped neighbours carry the flag across the boundary
            s.weight[0, 1, 0] = s.weight[0, 2, -1] = s.weight[1, 1, 0] = s.weight[1, 1, -1] = 0.0
        ref = s
        if gname == "fixed_ra":
            ref = clone(base, with_era=False)
        elif gname == "other_mask":
            ref = clone(base)
            ref.weight[:][rng.uniform(size=ref.weight[:].shape) < 0.15] = 0.0
            ref.vis[:] = ref.vis[:] * np.complex64(1.01)
        elif gname == "equal_positions":
            ref = clone(base)
            ref.effective_ra[0, 1, 20] = ref.effective_ra[0, 1, 19]
            ref.effective_ra[1, 2, 0] = ref.effective_ra[1, 2, 1]
        key = f"gradient/{gname}"
        for k in ("vis", "vis_weight", "effective_ra"):
            out[f"{key}/in/{k}"] = np.array(s.datasets[k][:])
            if ref is not s and k in ref.datasets:
                out[f"{key}/ref/{k}"] = np.array(ref.datasets[k][:])
        pos = np.array(ref.effective_ra[:]).reshape(-1, 48) if "effective_ra" in ref.datasets else np.asarray(ref.ra)
        tv, tw = twin.gradient_twin(np.array(s.vis[:]).reshape(-1, 48), np.array(s.weight[:]).reshape(-1, 48), np.array(s.effective_ra[:]).reshape(-1, 48), np.asarray(s.ra),
                                    np.array(ref.vis[:]).reshape(-1, 48), np.array(ref.weight[:]).reshape(-1, 48), pos)
        task = make_task(sidereal.RebinGradientCorrection)
        task.setup(ref)
        res = task.process(s)
        assert "effective_ra" not in res.datasets
        rv, rw = np.asarray(res.vis[:]).reshape(tv.shape), np.asarray(res.weight[:]).reshape(tw.shape)
        e_ref = np.abs(rv - tv).max() / np.abs(tv).max()
        assert np.array_equal(rw == 0, tw == 0), gname
        print(f"{key}: e_ref={e_ref:.3e} flagged by the correction {int((rw == 0).sum() - (out[f'{key}/in/vis_weight'] == 0).sum())}")
        out[f"{key}/vis"], out[f"{key}/vis_weight"], out[f"{key}/e_ref"] = np.asarray(res.vis[:]), np.asarray(res.weight[:]), e_ref
        gnames.append(gname)
    out["gradient/names"] = np.array(gnames)
    out["gradient/ra"] = np.asarray(base.ra)

    # ---- the three direct interpolators: _regrid on every small cadence and the two-tile one
    classes = {"nearest": sidereal.SiderealRegridderNearest, "linear": sidereal.SiderealRegridderLinear, "cubic": sidereal.SiderealRegridderCubic}
    inames = []
    for cname in ("c37", "c11", "c150", "c48", "c1100"):
        lsd, vis, w, nra = out[f"rebin/{cname}/lsd"], out[f"rebin/{cname}/vis"], out[f"rebin/{cname}/weight"], int(out[f"rebin/{cname}/samples"])
        for kind, cls in classes.items():
            task = make_task(cls, samples=nra, start=LSD, end=LSD + 1)
            grid, sts, ni = task._regrid(vis.copy(), w.copy(), lsd.copy())
            tv, tw = twin.interp_twin(kind, vis.reshape(-1, len(lsd)), w.reshape(-1, len(lsd)), lsd, nra, float(LSD), float(LSD + 1))
            e_ref = np.abs(sts.reshape(tv.shape) - tv).max() / np.abs(tv).max()
            nz = tw != 0
            e_w = (np.abs(ni.reshape(tw.shape) - tw)[nz] / tw[nz]).max() if nz.any() else 0.0
            assert np.array_equal(ni.reshape(tw.shape) == 0, tw == 0), (cname, kind)
            print(f"interp/{cname}/{kind}: e_ref={e_ref:.3e} weight rel={e_w:.3e} flagged grid points {int((~ni.reshape(tw.shape)[1].astype(bool)).sum())}")
            key = f"interp/{cname}/{kind}"
            out[f"{key}/grid"], out[f"{key}/vis"], out[f"{key}/vis_weight"], out[f"{key}/e_ref"] = grid, sts, ni, e_ref
        inames.append(cname)
    out["interp/names"] = np.array(inames)

    # ---- down_mix through process, on the observer of the regridder's fixture
    with np.load(os.path.join(GOLDEN, "regrid.npz")) as z:
        baselines, feedmask, prodstack, freq = z["task/baselines"], z["task/feedmask"], z["task/prodstack"], z["task/freq"]
        latitude = float(z["task/obs"][2])
    obs = Observer(4, baselines, feedmask, latitude, t0, day)
    lsd = cadence(150, 64)
    vis, w = make_data(rng, lsd, (2, 4), (2, 4), special=False)
    fm = feedmask[prodstack["input_a"], prodstack["input_b"]]
    ph = regrid_twin.fringe_phase(freq, baselines[:, 0], np.ones(4), latitude, lsd)
    vis = (vis * 0.3 + np.conj(ph)).astype(np.complex64)
    out["mix/lsd"], out["mix/vis"], out["mix/weight"], out["mix/samples"] = lsd, vis, w, np.array(64)
    for kind in ("linear", "cubic"):
        data = FakeTime(freq=freq, stack=np.arange(4), time=t0 + lsd * day)
        data.prodstack = prodstack
        data.attrs["lsd"] = LSD
        data.vis[:] = vis
        data.weight[:] = w
        sidereal.containers.SiderealStream = FakeSidereal
        task = make_task(classes[kind], samples=64, down_mix=True, observer=obs)
        sd = task.process(data)
        src = obs.unix_to_lsd(data.time)
        grid = LSD + np.arange(64) / 64
        pin = regrid_twin.fringe_phase(freq, baselines[:, 0], fm, latitude, src).reshape(8, -1)
        pout = regrid_twin.fringe_phase(freq, baselines[:, 0], fm, latitude, grid).reshape(8, -1)
        tv, tw = twin.interp_twin(kind, vis.reshape(8, -1), w.reshape(8, -1), src, 64, float(LSD), float(LSD + 1), pin, pout)
        e_ref = np.abs(np.asarray(sd.vis[:]).reshape(8, -1) - tv).max() / np.abs(tv).max()
        print(f"mix/{kind}: e_ref={e_ref:.3e}")
        out[f"mix/{kind}/vis"], out[f"mix/{kind}/vis_weight"], out[f"mix/{kind}/e_ref"] = np.asarray(sd.vis[:]), np.asarray(sd.weight[:]), e_ref

    path = os.path.join(GOLDEN, "rebin.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
