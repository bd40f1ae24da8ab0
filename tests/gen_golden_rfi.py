"""Generate tests/golden/rfi.npz by EXECUTING the reference's own ``sumthreshold_py``, ``scale_invariant_rank``, ``mad``,
``tv_channels_flag``, ``RFISensitivityMask.process``, ``RFIMask.process`` and ``ApplyTimeFreqMask.process`` from source
(through ``oracle._refstub``), on stand-in containers.  Only the data is committed; run where the reference checkout
exists:

    python tests/gen_golden_rfi.py

caput is not installed, so the twin's median functions (``tests/rfi_twin.py``, the conventions of DESIGN.md section 7i)
are patched into the stubbed ``caput.algorithms.median``.  The generator refuses to write a case unless

* every threshold comparison of the case (the static-channel test, MAD, the TV fraction against ``f``, every
  SumThreshold step) leaves a relative margin above 1e-9 against the larger of its two sides -- comparisons with both
  sides exactly zero or one side not finite are exempt, they come out the same in any summation order -- and
* no moving-median window of the case is empty, so that the reference-executed vectors do not rest on the NaN
  convention.  One exception, which the outcome does not depend on: the sensitivity case has a channel without any
  weight, whose quantile over time is NaN by the n = 0 convention; the channel is flagged before the quantile is taken,
  takes no part in the medians over frequency, and a NaN comparison leaves it as it was.

The margins are measured on the twin's replay of the case, whose mask must equal the reference's exactly; the smallest
margin of every case is recorded in the file.
"""

import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rfi_twin as twin  # noqa: E402
from gen_golden_regrid import DS, LA, make_task  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-9
EMPTY = {"n": 0}


class MP(LA):
    """ndarray with the MPIArray calls the mask tasks make."""

    def __new__(cls, shape, axis=0, dtype=np.float64, comm=None):
        return np.zeros(shape, dtype=dtype).view(cls)

    local_offset = (0, 0, 0, 0)

    def enumerate(self, axis):
        return [(i, i) for i in range(self.shape[axis])]

    def redistribute(self, axis):
        return self

    def allgather(self):
        return self.view(np.ndarray)

    @classmethod
    def wrap(cls, arr, axis):
        return np.asarray(arr).view(cls)


class DSM(DS):
    def __init__(self, arr, axis):
        super().__init__(arr, axis)
        self.arr = self.arr.view(MP)


class Cont:
    """Stand-in container: axes, datasets with an ``axis`` attribute, ``copy(shared=...)``."""

    spec = {}

    def __init__(self, axes_from=None, attrs_from=None, copy_from=None, **axes):
        src = axes_from if axes_from is not None else copy_from
        need = {a for ax, _ in self.spec.values() for a in ax}
        self.index_map = {k: v for k, v in (src.index_map.items() if src is not None else ()) if k in need}
        self.index_map.update({k: np.asarray(v) for k, v in axes.items()})
        self.attrs = {}
        self.comm = types.SimpleNamespace(rank=0, allgather=lambda x: [x], Bcast=lambda *a, **k: None)
        self.datasets = {n: DSM(np.zeros([len(self.index_map[a]) for a in ax], dtype=dt), ax) for n, (ax, dt) in self.spec.items()}

    def __getattr__(self, name):
        d = self.__dict__
        if name in d.get("index_map", {}):
            return d["index_map"][name]
        ds = d.get("datasets", {})
        if name in ds:
            return ds[name]
        if name == "weight" and "vis_weight" in ds:
            return ds["vis_weight"]
        raise AttributeError(name)

    def redistribute(self, axis):
        pass

    def copy(self, shared=()):
        out = type(self).__new__(type(self))
        out.__dict__.update(self.__dict__)
        out.datasets = {n: (d if n in shared else DSM(np.array(d.arr), d.attrs["axis"])) for n, d in self.datasets.items()}
        return out


class Sens(Cont):
    spec = {k: (("freq", "pol", "time"), np.float32) for k in ("measured", "radiometer", "weight")}


class RFIMaskC(Cont):
    spec = {"mask": (("freq", "time"), bool)}


class RFIMaskByPolC(RFIMaskC):
    spec = {"mask": (("pol", "freq", "time"), bool)}


class SidMaskC(Cont):
    spec = {"mask": (("freq", "ra"), bool)}


class SidMaskByPolC(SidMaskC):
    spec = {"mask": (("pol", "freq", "ra"), bool)}


class TimeStreamC(Cont):
    spec = {"vis": (("freq", "stack", "time"), np.complex64), "vis_weight": (("freq", "stack", "time"), np.float32)}


class SidStreamC(Cont):
    spec = {"vis": (("freq", "stack", "ra"), np.complex64), "vis_weight": (("freq", "stack", "ra"), np.float32)}


class HybridC(Cont):
    spec = {"vis": (("pol", "freq", "ew", "el", "ra"), np.complex64), "vis_weight": (("pol", "freq", "ew", "ra"), np.float32)}


def _counting(fn):
    def wrapped(x, w, *a):
        out = fn(x, w, *a)
        EMPTY["n"] += int(np.isnan(out).sum())
        return out

    return wrapped


def load():
    _refstub.load_reference()
    median = importlib.import_module("caput.algorithms.median")
    median.moving_weighted_median = _counting(twin.moving_weighted_median)
    median.quantile = twin.quantile
    median.weighted_median = twin.weighted_median
    alg = importlib.import_module("caput.algorithms")
    alg.median = median
    flagging = importlib.import_module("draco.analysis.flagging")
    ref_rfi = importlib.import_module("draco.util.rfi")
    flagging.median = median
    flagging.filters.algorithms = alg
    flagging.tools.invert_no_zero = _refstub._invert_no_zero
    flagging.mpiarray = types.SimpleNamespace(MPIArray=MP)
    flagging.containers = types.SimpleNamespace(RFIMask=RFIMaskC, RFIMaskByPol=RFIMaskByPolC, SiderealRFIMask=SidMaskC, SiderealRFIMaskByPol=SidMaskByPolC)
    return flagging, ref_rfi


def check(name, margins, out):
    m = min(margins) if margins else np.inf
    assert m > MARGIN, f"{name}: a comparison has a relative margin of {m:.3e}: refusing to write the case"
    out[f"{name}/margin"] = np.array(m)
    return m


def sensitivity_case(rng, nf=40, nt=96, npol=2):
    """Radiometer ratio near 1 with 5 % noise: a bad channel, a broadband burst, a faint block, single spikes, a
    zero-weight row and two zero-weight columns.  The frequencies span seven TV channels, each with an odd number of
    rows: a fraction of bad samples then never equals ``tv_fraction = 0.5``, a comparison without any margin."""
    freq = 638.0 - 0.8 * np.arange(nf)
    rad = rng.uniform(0.8, 1.2, (nf, npol, nt)).astype(np.float32)
    ratio = 1.0 + 0.05 * rng.normal(size=(nf, npol, nt))
    ratio[12] += 0.6
    ratio[:, :, 30:33] += 0.45
    ratio[20:27, :, 60:76] += 0.09
    for _ in range(12):
        ratio[rng.integers(nf), rng.integers(npol), rng.integers(nt)] += rng.uniform(0.5, 1.5)
    meas = (ratio * rad).astype(np.float32)
    w = rng.uniform(0.5, 2.0, (nf, npol, nt)).astype(np.float32)
    w[5] = 0.0
    w[:, :, 50:52] = 0.0
    w[rng.uniform(size=w.shape) < 0.03] = 0.0
    time = 1.6e9 + 10.0 * np.arange(nt)
    return freq, time, meas, rad, w


def main():
    flagging, ref_rfi = load()
    rng = np.random.default_rng(20261019)
    out = {}

    # ---- sumthreshold_py
    nf, nt = 24, 40
    data = rng.normal(size=(nf, nt))
    data[3, 0] += 9.0  # hits at the first and at the last sample
    data[7, nt - 1] -= 9.0
    data[0, 17] += 8.0
    data[nf - 1, 5] += 8.0
    data[10:13, 20:24] += 2.5
    data[15, 8:30] += 1.6
    data[20, 3] = np.nan
    data[21, 30] = np.inf
    start = rng.uniform(size=(nf, nt)) < 0.1
    var = rng.uniform(0.5, 2.0, (nf, nt))
    var_nan = var.copy()
    var_nan[start] = np.nan  # a NaN variance under flags
    out["st/data"], out["st/start"], out["st/var"], out["st/var_nan"] = data, start, var, var_nan
    st_cases = {
        "m1": dict(max_m=1, threshold1=3.0),
        "m8": dict(max_m=8, threshold1=3.0, start_flag=start),
        "m64": dict(max_m=64, threshold1=3.0, start_flag=start),  # both axes are shorter than 64
        "m8_axes01": dict(max_m=8, threshold1=3.0, axes=(0, 1)),
        "m8_axis0": dict(max_m=8, threshold1=3.0, axes=0),
        "m8_var": dict(max_m=8, threshold1=3.0, variance=var, remove_median=False, start_flag=start),
        "m8_var_nan": dict(max_m=8, threshold1=3.0, variance=var_nan, remove_median=False, start_flag=start, rho=1.0),
        "m8_positive": dict(max_m=8, threshold1=3.0, only_positive=True),
        "m8_nomissing": dict(max_m=8, threshold1=3.0, correct_for_missing=False, start_flag=start),
        "m16_default": dict(),
    }
    for name, kw in st_cases.items():
        ref = ref_rfi.sumthreshold_py(data, **kw)
        margins = []
        tw = twin.sumthreshold(data, margins=margins, **kw)
        assert np.array_equal(ref, tw), f"st/{name}: the twin differs from the reference"
        m = check(f"st/{name}", margins, out)
        out[f"st/{name}/mask"] = ref
        print(f"st/{name}: flagged {ref.mean():.3f} margin {m:.2e}")
    out["st/names"] = np.array(list(st_cases))

    # ---- scale_invariant_rank
    base = rng.uniform(size=(nf, nt)) < 0.12
    base[4] = np.tile([False, False, False, False, True], nt // 5)  # exact ties at eta 0.2
    out["sir/base"] = base
    sir_cases = {"eta0": (0.0, -1), "eta02": (0.2, -1), "eta1": (1.0, -1), "eta02_ax0": (0.2, 0), "both": (0.2, (0, -1)), "tuple": ((0.1, 0.3), (0, -1))}
    for name, (eta, axis) in sir_cases.items():
        ref = ref_rfi.scale_invariant_rank(base.copy(), eta=eta, axis=axis)
        assert np.array_equal(ref, twin.scale_invariant_rank(base, eta=eta, axis=axis)), f"sir/{name}: the twin differs from the reference"
        out[f"sir/{name}/mask"] = ref
        print(f"sir/{name}: flagged {ref.mean():.3f} (base {base.mean():.3f})")
    out["sir/names"] = np.array(list(sir_cases))

    # ---- mad and tv_channels_flag
    freq, time, meas, rad, w = sensitivity_case(rng)
    x = (meas[:, 0] / rad[:, 0]).astype(np.float64)
    xc = (x + 1j * rng.normal(size=x.shape)).astype(np.complex64)
    mk = w[:, 0] == 0
    EMPTY["n"] = 0
    out["mad/x"], out["mad/xc"], out["mad/mask"], out["mad/freq"] = x, xc, mk, freq
    out["mad/real"] = flagging.mad(x, mk, base_size=(5, 3), mad_size=(7, 9))
    out["mad/complex"] = flagging.mad(xc, mk, base_size=(5, 3), mad_size=(7, 9))
    assert EMPTY["n"] == 0, "mad: an empty median window"
    dev = np.where(np.isnan(out["mad/real"]), 10.0, out["mad/real"])
    mask, frac = flagging.tv_channels_flag(dev, freq, sigma=3.0, f=0.3, debug=True)
    margins = []
    assert np.array_equal(mask, twin.tv_channels_flag(dev, freq, sigma=3.0, f=0.3, margins=margins))
    check("tv", margins, out)
    out["tv/x"], out["tv/mask"], out["tv/frac"] = dev, mask, frac
    out["tv/thresholds"] = np.array([t for _, t in twin.tv_thresholds(freq, 3.0, 0.3)])
    out["tv/thresholds_ref"] = np.array([flagging.p_to_sigma(flagging.inverse_binom_cdf_prob(int(0.3 * len(r)), len(r), 1 - flagging.sigma_to_p(3.0))) for r, _ in twin.tv_thresholds(freq, 3.0, 0.3)])

    # ---- RFISensitivityMask.process
    sens = Sens(freq=freq, pol=np.array(["XX", "YY"]), time=time)
    sens.measured[:], sens.radiometer[:], sens.weight[:] = meas, rad, w
    out["sens/freq"], out["sens/time"], out["sens/measured"], out["sens/radiometer"], out["sens/weight"] = freq, time, meas, rad, w
    static = np.zeros(len(freq), dtype=bool)
    static[33] = True
    mixed = np.zeros((len(freq), len(time)), dtype=bool)
    mixed[:, 20:45] = True
    mixed[8:16, 70:] = True
    out["sens/static"], out["sens/mixed"] = static, mixed
    cfg = dict(include_pol=None, nsigma_1d=5.0, quantile_1d=0.15, win_f_1d=9, nsigma=5.0, niter=5, rho=1.5, base_size=(7, 15), mad_size=(11, 5), tv_fraction=0.5,
               max_m=64, eta=0.2, only_time=False)
    sens_cases = {}
    for mt in ("mad", "sumthreshold", "combine"):
        for sir in (False, True):
            sens_cases[f"{mt}_sir{int(sir)}"] = dict(mask_type=mt, sir=sir)
    sens_cases["combine_mixed_sir0"] = dict(mask_type="combine", sir=False, mixed=True, static=True)
    sens_cases["combine_mixed_sir1"] = dict(mask_type="combine", sir=True, mixed=True, static=True, only_time=True)
    sens_cases["mad_pol_global"] = dict(mask_type="mad", sir=False, include_pol=["YY"], win_f_1d=None)
    for name, case in sens_cases.items():
        case = dict(case)
        use_mixed, use_static = case.pop("mixed", False), case.pop("static", False)
        c = dict(cfg, **case)
        task = make_task(flagging.RFISensitivityMask, **c)
        if use_mixed:
            task._combine_st_mad_hook = lambda times, freq: mixed
        if use_static:
            task._static_rfi_mask_hook = lambda freq, timestamp=None: ~static
        task.setup()
        EMPTY["n"] = 0
        ref = np.asarray(task.process(sens).mask[:])
        assert EMPTY["n"] == 0, f"sens/{name}: {EMPTY['n']} empty median windows"
        margins = []
        inc = None if c["include_pol"] is None else [p in c["include_pol"] for p in ("XX", "YY")]
        tw = twin.sensitivity_mask(meas, rad, w, freq, mask_type=c["mask_type"], include=inc, static=static if use_static else None, madtimes=mixed if use_mixed else None,
                                   nsigma_1d=c["nsigma_1d"], quantile_1d=c["quantile_1d"], win_f_1d=c["win_f_1d"], nsigma=c["nsigma"], niter=c["niter"], rho=c["rho"],
                                   base_size=c["base_size"], mad_size=c["mad_size"], tv_fraction=c["tv_fraction"], max_m=c["max_m"], sir=c["sir"], eta=c["eta"],
                                   only_time=c["only_time"], margins=margins)
        assert np.array_equal(ref, tw), f"sens/{name}: the twin differs from the reference in {int((ref != tw).sum())} samples"
        m = check(f"sens/{name}", margins, out)
        out[f"sens/{name}/mask"] = ref
        out[f"sens/{name}/flags"] = np.array([use_mixed, use_static, c["sir"], c["only_time"], c["win_f_1d"] is None, c["include_pol"] is not None])
        out[f"sens/{name}/mask_type"] = np.array(c["mask_type"])
        print(f"sens/{name}: masked {100 * ref.mean():.1f} % margin {m:.2e}")
    out["sens/names"] = np.array(list(sens_cases))

    # ---- RFIMask.process
    nstack = 3
    vis = (rng.normal(size=(len(freq), nstack, len(time))) + 1j * rng.normal(size=(len(freq), nstack, len(time)))).astype(np.complex64)
    vis[:, 1] += (3.0 * (meas[:, 0] / rad[:, 0] - 1.0) / 0.05 * (rng.uniform(size=meas[:, 0].shape) < 0.5)).astype(np.complex64)
    vw = rng.uniform(0.5, 2.0, vis.shape).astype(np.float32)
    vw[:, :, 50:52] = 0.0
    vw[5] = 1e-7
    out["rfimask/vis"], out["rfimask/weight"] = vis, vw
    for kind, cls, ax in (("time", TimeStreamC, dict(time=time)), ("ra", SidStreamC, dict(ra=np.linspace(0, 360, len(time), endpoint=False)))):
        ts = cls(freq=freq, stack=np.arange(nstack), **ax)
        ts.vis[:], ts.weight[:] = vis, vw
        EMPTY["n"] = 0
        res = make_task(flagging.RFIMask, sigma=5.0, tv_fraction=0.5, stack_ind=1).process(ts)
        assert EMPTY["n"] == 0, "rfimask: an empty median window"
        assert type(res) is (RFIMaskC if kind == "time" else SidMaskC)
        ref = np.asarray(res.mask[:])
        margins = []
        assert np.array_equal(ref, twin.rfi_mask(vis[:, 1], vw[:, 1], freq, 5.0, 0.5, margins=margins)), "rfimask: the twin differs from the reference"
        m = check(f"rfimask/{kind}", margins, out)
        out[f"rfimask/{kind}/mask"] = ref
        print(f"rfimask/{kind}: masked {100 * ref.mean():.1f} % margin {m:.2e}")

    # ---- ApplyTimeFreqMask.process
    mask2 = rng.uniform(size=(len(freq), len(time))) < 0.2
    maskp = rng.uniform(size=(2, len(freq), len(time))) < 0.2
    out["apply/mask"], out["apply/mask_pol"] = mask2, maskp
    ts = TimeStreamC(freq=freq, stack=np.arange(nstack), time=time)
    ts.vis[:], ts.weight[:] = vis, vw
    rm = RFIMaskC(freq=freq, time=time)
    rm.mask[:] = mask2
    res = make_task(flagging.ApplyTimeFreqMask, share="none", collapse_pol=False, match_axes=True).process(ts, rm)
    assert np.array_equal(np.asarray(ts.weight[:]), vw), "share='none' modified its input"
    out["apply/time/weight"] = np.asarray(res.weight[:])
    # a mask on a sub-range of the time axis, match_axes off
    sub = slice(10, 70)
    rm = RFIMaskC(freq=freq, time=time[sub])
    rm.mask[:] = mask2[:, sub]
    res = make_task(flagging.ApplyTimeFreqMask, share="vis", collapse_pol=False, match_axes=False).process(ts, rm)
    assert res.datasets["vis"] is ts.datasets["vis"]
    out["apply/time_sub/weight"], out["apply/time_sub/range"] = np.asarray(res.weight[:]), np.array([sub.start, sub.stop])
    # a by-pol mask collapsed onto a sidereal stream
    ra = np.linspace(0, 360, len(time), endpoint=False)
    ss = SidStreamC(freq=freq, stack=np.arange(nstack), ra=ra)
    ss.vis[:], ss.weight[:] = vis, vw
    rp = SidMaskByPolC(freq=freq, pol=np.array(["XX", "YY"]), ra=ra)
    rp.mask[:] = maskp
    res = make_task(flagging.ApplyTimeFreqMask, share="none", collapse_pol=True, match_axes=True).process(ss, rp)
    out["apply/ra_pol/weight"] = np.asarray(res.weight[:])
    # a by-pol mask applied per polarisation to a hybrid stream's weight
    hw = rng.uniform(0.5, 2.0, (2, len(freq), 3, len(time))).astype(np.float32)
    hs = HybridC(pol=np.array(["XX", "YY"]), freq=freq, ew=np.arange(3), el=np.arange(2), ra=ra)
    hs.weight[:] = hw
    res = make_task(flagging.ApplyTimeFreqMask, share="none", collapse_pol=False, match_axes=True).process(hs, rp)
    out["apply/hybrid/in"], out["apply/hybrid/weight"] = hw, np.asarray(res.weight[:])

    path = os.path.join(GOLDEN, "rfi.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
