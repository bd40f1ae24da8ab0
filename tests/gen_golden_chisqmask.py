"""Generate tests/golden/chisqmask.npz by EXECUTING the reference's own ``RFIMaskChisqHighDelay.process``, ``mask_1d``,
``mask_2d``, ``mask_2d_sumthreshold``, ``ReduceChisq.reduction``, ``ReduceVar.reduction`` and ``tools.arPLS_1d`` from
source (through ``oracle._refstub``), on stand-in containers.  Only the data is committed; run where the reference
checkout exists:

    python tests/gen_golden_chisqmask.py

caput is not installed, so the twin's medians (``tests/chisqmask_twin.py``, the conventions of DESIGN.md section 7s) are
patched into the stubbed ``caput.algorithms.median``; ``weighted_median`` gives 0.0 for an empty row.  The generator
refuses to write unless

* every weight is a non-negative integer below 2^10, so that every weight sum is exact in float32, float64 and long
  double and no tie of a median depends on rounding;
* the first moving median of every plane has at least 20 windows that split exactly between two different samples, at
  least 20 that do not, at least 5 empty windows, and duplicate sample values;
* the twin's replay of the case, fed the reference's own float32 collapse, gives the reference's mask exactly;
* every threshold comparison of that replay leaves a margin of more than 16 times the largest difference, at that
  comparison, to a second replay fed a long-double collapse (the reference collapses in the input's float32, the
  device in float64), and of at least 1e-9 relative; comparisons with both sides zero or a side not finite are exempt;
* every masked fraction lies strictly between 0 and 1.

The smallest relative margin of every case is recorded in the file.
"""

import importlib
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import chisqmask_twin as twin  # noqa: E402
from gen_golden_regrid import make_task  # noqa: E402
from gen_golden_rfi import DSM, MP, HybridC, RFIMaskByPolC, RFIMaskC, SidMaskByPolC, SidMaskC, SidStreamC, TimeStreamC  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-9
NF, NT = 24, 160
CALLS = []  # (x, w, size) of every moving median the reference asks for


class MPX(MP):
    """An MPIArray's ``reshape`` takes None for the distributed axis."""

    def reshape(self, *shape):
        return np.ndarray.reshape(self, *[-1 if n is None else n for n in shape])


class DSX(DSM):
    def __init__(self, arr, axis):
        super().__init__(arr, axis)
        self.arr = self.arr.view(MPX)

    @property
    def shape(self):
        return self.arr.shape


class _Data:
    def __init__(self, **axes):
        super().__init__(**axes)
        self.datasets = {n: DSX(d.arr, d.attrs["axis"]) for n, d in self.datasets.items()}

    @property
    def data(self):
        return self.datasets["vis"]


class TS(_Data, TimeStreamC):
    pass


class SS(_Data, SidStreamC):
    pass


class HS(_Data, HybridC):
    pass


def load():
    _refstub.load_reference()
    median = importlib.import_module("caput.algorithms.median")

    def moving(x, w, size):
        CALLS.append((np.array(x), np.array(w), tuple(size)))
        return twin.moving_weighted_median(x, w, size)

    median.moving_weighted_median = moving
    median.weighted_median = twin.weighted_median
    flagging = importlib.import_module("draco.analysis.flagging")
    transform = importlib.import_module("draco.analysis.transform")
    tools = importlib.import_module("draco.util.tools")
    flagging.median = median
    for mod in (flagging.tools, transform, tools):
        mod.invert_no_zero = _refstub._invert_no_zero
    flagging.containers = types.SimpleNamespace(RFIMask=RFIMaskC, RFIMaskByPol=RFIMaskByPolC, SiderealRFIMask=SidMaskC, SiderealRFIMaskByPol=SidMaskByPolC)
    return flagging, transform, tools


# ---- inputs


def statistic(rng, lead, nstack):
    """A chi-squared per degree of freedom ``[*lead, NF, nstack, NT]`` float32 and its integer degrees of freedom: a
    smooth level over frequency, a high channel, bursts, a channel and a stretch of time without weight, scattered
    samples without weight, four channels of one weight throughout (their windows split exactly whenever they hold an
    even number of samples), and columns that repeat another column (equal values)."""
    shape = (*lead, NF, nstack, NT)
    ndof = rng.integers(40, 200, size=shape).astype(np.float64)
    ndof[..., 1:5, :, :] = 64.0
    lost = rng.uniform(size=(*lead, NF, 1, NT)) < 0.08
    ndof = ndof * ~lost
    ndof[..., 9, :, :] = 0.0
    ndof[..., :, :, 70:100] = 0.0
    level = 1.0 + 0.1 * np.sin(np.arange(NF) / 5.0)
    x = level[:, None, None] + np.sqrt(2.0 / np.maximum(ndof, 1.0)) * rng.normal(size=shape)
    x[..., 15, :, :] += 0.9
    x[..., :, :, 30:32] += 1.2
    x[..., 5:8, :, 120:128] += 0.9
    for _ in range(10):
        x[..., rng.integers(NF), :, rng.integers(NT)] += rng.uniform(1.0, 3.0)
    for a, b in ((10, 11), (40, 44), (130, 150), (5, 155)):
        x[..., b], ndof[..., b] = x[..., a], ndof[..., a]
    assert np.all(ndof == np.round(ndof)) and ndof.min() >= 0 and ndof.max() < 2**10
    return x.astype(np.float32), ndof.astype(np.float32)


def collapse32(x, w, axsum, wfactor):
    """The reference's expressions on the inputs' own types."""
    wsum = wfactor * np.sum(w, axis=axsum)
    return np.sum(w * x, axis=axsum) * _refstub._invert_no_zero(wsum), wsum


def fixtures_ok(name, x, w, size):
    detail = {}
    twin.moving_weighted_median(x, w, size, detail)
    kept = x[w > 0]
    n_exact, n_empty = int(detail["exact"].sum()), int(detail["empty"].sum())
    n_plain = int((~detail["exact"] & ~detail["empty"]).sum())
    assert n_exact >= 20 and n_plain >= 20, f"{name}: {n_exact} exactly split windows, {n_plain} others"
    assert n_empty >= 5, f"{name}: {n_empty} empty windows"
    assert len(np.unique(kept)) < kept.size, f"{name}: no duplicate values"
    return n_exact, n_empty


def compare_traces(name, ta, tb):
    assert len(ta) == len(tb), f"{name}: the two replays make different numbers of comparisons"
    for k, ((a1, b1), (a2, b2)) in enumerate(zip(ta, tb)):
        ok = np.isfinite(a1) & np.isfinite(b1) & np.isfinite(a2) & np.isfinite(b2) & (np.maximum(np.abs(a1), np.abs(b1)) > 0)
        if not ok.any():
            continue
        diff = float((np.abs(a1 - a2) + np.abs(b1 - b2))[ok].max())
        gap = float(np.abs(a1 - b1)[ok].min())
        assert gap > 16.0 * diff, f"{name}: comparison {k} has a margin of {gap:.3e} against a difference of {diff:.3e} between the replays"
    m = twin.trace_margin(ta)
    assert m > MARGIN, f"{name}: a comparison has a relative margin of {m:.3e}"
    return m


DAY = (np.arange(NT) >= 100) & (np.arange(NT) < 112)
SOURCES = np.zeros((NF, NT), dtype=bool)
SOURCES[5:8, 40:50] = True

# name -> (input, config, extras)
BASE = dict(reg_arpls=1e5, nsigma_1d=5.0, win_t=21, win_f=1, nsigma_2d=5.0, estimate_var=False, only_positive=False, separate_pol=False, mask_type="mad", niter=5,
            rho=1.5, max_m=32, flag_ew=None)
CASES = {
    "mad_t21": ("ts", dict()),
    "mad_t601": ("ts", dict(win_t=601)),
    "mad_var": ("ts", dict(estimate_var=True, win_f=3)),
    "mad_positive": ("ts", dict(only_positive=True)),
    "st_t21": ("ts", dict(mask_type="sumthreshold")),
    "st_t601": ("ts", dict(mask_type="sumthreshold", win_t=601)),
    "st_var_positive": ("ts", dict(mask_type="sumthreshold", estimate_var=True, only_positive=True)),
    "stack1": ("ts1", dict()),
    "hybrid_bypol": ("hyb", dict(separate_pol=True, flag_ew=np.array([1.0, 0.0]))),
    "hybrid_all": ("hyb", dict(flag_ew=np.array([0.0, 1.0]))),
    "sidereal_scalar": ("sid", dict(hooks=True, lsd=4321)),
    "sidereal_vector": ("sid", dict(hooks=True, lsd=np.array([4321, 4322, 4324]))),
}


def main():
    flagging, transform, tools = load()
    rng = np.random.default_rng(20261021)
    out = {}

    # ---- the reductions
    red_shapes = {"s3x5x70": ((3, 5, 70), (3, 5, 70), (1,)), "s2x1x65": ((2, 1, 65), (2, 1, 65), (1,)), "s1x193x2": ((1, 193, 2), (1, 193, 2), (1,)),
                  "hybrid": ((2, 3, 4, 33), (2, 3, 1, 33), (1, 2))}
    for sname, (shape, wshape, axis) in red_shapes.items():
        x = (rng.normal(size=shape) + 1j * rng.normal(size=shape)) * 3.0 + (2.0 - 1.0j)
        w = rng.integers(0, 8, size=wshape).astype(np.float32)
        w[..., 0] = 0.0  # a column without weight
        if shape[-1] > 2:
            w[..., 1] = 0.0
            w[(slice(None),) + (0,) * (len(wshape) - 2) + (1,)] = 3.0  # exactly one positive weight
        out[f"red/{sname}/x"], out[f"red/{sname}/w"], out[f"red/{sname}/axis"] = x, w, np.array(axis)
        wb = np.broadcast_to(w, shape)
        for dname, dt in (("f32", np.float32), ("f64", np.float64), ("c64", np.complex64), ("c128", np.complex128)):
            arr = (x if np.dtype(dt).kind == "c" else x.real).astype(dt)
            v, num = make_task(transform.ReduceChisq).reduction(arr, wb, axis)
            out[f"red/{sname}/{dname}/chisq"], out[f"red/{sname}/{dname}/chisq_w"] = np.asarray(v), np.asarray(num)
            for weighting in ("none", "masked", "weighted"):
                v, ws = make_task(transform.ReduceVar, weighting=weighting).reduction(arr, wb, axis)
                out[f"red/{sname}/{dname}/var_{weighting}"], out[f"red/{sname}/{dname}/var_{weighting}_w"] = np.asarray(v), np.asarray(ws)
            y, s = collapse32(arr.real, wb, axis, 1.0)
            out[f"red/{sname}/{dname}/wmean"], out[f"red/{sname}/{dname}/wmean_w"] = np.asarray(y), np.asarray(s)
    out["red/shapes"] = np.array(list(red_shapes))

    # ---- arPLS
    fr = np.arange(64)
    for k, (lam, nmask) in enumerate(((1e5, 6), (1e2, 0), (1e5, 64))):
        y = 1.0 + 0.2 * np.sin(fr / 9.0) + 0.02 * rng.normal(size=64)
        y[[7, 30, 31]] += 1.5
        m = np.zeros(64, dtype=bool)
        m[rng.choice(64, nmask, replace=False)] = True
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            z = tools.arPLS_1d(y, mask=m, lam=lam)
        out[f"arpls/{k}/y"], out[f"arpls/{k}/mask"], out[f"arpls/{k}/lam"], out[f"arpls/{k}/z"] = y, m, np.array(lam), z
    out["arpls/n"] = np.array(3)

    # ---- the mask task
    x_ts, w_ts = statistic(rng, (), 3)
    x_h, w_h5 = statistic(rng, (2,), 4)  # [pol, freq, ew * el, ra]
    x_h = x_h.reshape(2, NF, 2, 2, NT)
    w_h = w_h5.reshape(2, NF, 2, 2, NT)[:, :, :, 0]
    out["in/ts/x"], out["in/ts/w"], out["in/hyb/x"], out["in/hyb/w"] = x_ts, w_ts, x_h, w_h
    freq = 800.0 - 0.4 * np.arange(NF)
    time = 1.6e9 + 10.0 * np.arange(NT)
    ra = np.linspace(0.0, 360.0, NT, endpoint=False)
    out["in/freq"], out["in/time"], out["in/ra"], out["in/day"], out["in/sources"] = freq, time, ra, DAY, SOURCES

    def imag(x):  # the statistic is the real part: the imaginary part must not matter
        return x[..., ::-1].copy()

    def stream(kind):
        if kind in ("ts", "ts1"):
            ns = 3 if kind == "ts" else 1
            s = TS(freq=freq, stack=np.arange(ns), time=time)
            s.datasets["vis"][:], s.datasets["vis_weight"][:] = (x_ts + 1j * imag(x_ts))[:, :ns], w_ts[:, :ns]
        elif kind == "sid":
            s = SS(freq=freq, stack=np.arange(3), ra=ra)
            s.datasets["vis"][:], s.datasets["vis_weight"][:] = x_ts + 1j * imag(x_ts), w_ts
        else:
            s = HS(pol=np.array(["XX", "YY"]), freq=freq, ew=np.arange(2), el=np.arange(2), ra=ra)
            s.datasets["vis"][:], s.datasets["vis_weight"][:] = x_h + 1j * imag(x_h), w_h
        return s

    tel = types.SimpleNamespace(lsd_to_unix=lambda lsd: 1.5e9 + 86164.0905 * np.asarray(lsd))
    for name, (kind, case) in CASES.items():
        case = dict(case)
        hooks, lsd = case.pop("hooks", False), case.pop("lsd", None)
        cfg = dict(BASE, **case)
        task = make_task(flagging.RFIMaskChisqHighDelay, **cfg)
        task.setup()
        s = stream(kind)
        if kind in ("sid", "hyb"):
            task.telescope = tel
            s.attrs["lsd"] = 4321 if lsd is None else lsd
        if hooks:
            task._day_flag_hook = lambda times: DAY
            task._source_flag_hook = lambda times, fq: SOURCES
        CALLS.clear()
        res = task.process(s)
        ref = np.asarray(res.mask[:])
        bypol = cfg["separate_pol"]
        want = {("ts", False): RFIMaskC, ("ts1", False): RFIMaskC, ("sid", False): SidMaskC, ("hyb", False): SidMaskC, ("hyb", True): SidMaskByPolC}[(kind, bypol)]
        assert type(res) is want, f"{name}: the reference returned a {type(res).__name__}"

        # the two collapses and the twin's replays
        xs, ws = np.asarray(s.data[:]).real, np.asarray(s.weight[:])
        if kind == "hyb":
            wb = ws[:, :, :, None, :]
            if cfg["flag_ew"] is not None:
                wb = wb * cfg["flag_ew"][None, None, :, None, None]
            axsum, wfactor = ((2, 3) if bypol else (0, 2, 3)), 2
        else:
            wb, axsum, wfactor = ws, (1,), 1.0
        c32, s32 = collapse32(xs, wb, axsum, wfactor)
        cld, sld = twin.reduce_wmean(xs, wb, axsum)  # (the twin sums the broadcast weight: the factor is in the sum)
        assert np.array_equal(np.asarray(s32, dtype=np.float64), np.asarray(sld, dtype=np.float64)), f"{name}: the weight sums are not exact"
        day = DAY if (hooks and np.isscalar(s.attrs["lsd"])) else None
        src = SOURCES if hooks else None
        kw = dict(mask_sources=src, mask_daytime=day, mask_type=cfg["mask_type"], nsigma_1d=cfg["nsigma_1d"], reg_arpls=cfg["reg_arpls"], win=(cfg["win_f"], cfg["win_t"]),
                  nsigma_2d=cfg["nsigma_2d"], estimate_var=cfg["estimate_var"], only_positive=cfg["only_positive"], niter=cfg["niter"], rho=cfg["rho"], max_m=cfg["max_m"],
                  baseline=lambda y, m: tools.arPLS_1d(y, mask=m, lam=cfg["reg_arpls"]))
        planes32 = c32 if bypol else c32[None]
        planesld = cld if bypol else cld[None]
        sums = s32 if bypol else s32[None]
        first = [c for c in CALLS]
        margins, tw = [], []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for p in range(len(planes32)):
                ta, tb = [], []
                tw.append(twin.chisq_mask(np.asarray(planes32[p], dtype=np.float64), sums[p], trace=ta, **kw))
                other = twin.chisq_mask(np.asarray(planesld[p], dtype=np.float64), sums[p], trace=tb, **kw)
                assert np.array_equal(tw[-1], other), f"{name}: the replays on the two collapses differ"
                margins.append(compare_traces(f"{name}[{p}]", ta, tb))
        tw = np.stack(tw) if bypol else tw[0]
        assert np.array_equal(ref, tw), f"{name}: the twin differs from the reference in {int((ref != tw).sum())} samples"
        assert 0.0 < ref.mean() < 1.0, f"{name}: masked fraction {ref.mean()}"
        # the first moving median of every plane carries the fixtures
        per_plane = len(first) // len(planes32)
        for p in range(len(planes32)):
            fixtures_ok(f"{name}[{p}]", *first[p * per_plane])
        out[f"case/{name}/mask"], out[f"case/{name}/margin"] = ref, np.array(min(margins))
        out[f"case/{name}/input"] = np.array(kind)
        out[f"case/{name}/lsd"] = np.asarray(-1 if lsd is None else lsd)
        out[f"case/{name}/hooks"] = np.array(hooks)
        out[f"case/{name}/flag_ew"] = np.asarray(cfg["flag_ew"] if cfg["flag_ew"] is not None else [])
        for k in ("win_t", "win_f", "estimate_var", "only_positive", "separate_pol", "mask_type"):
            out[f"case/{name}/{k}"] = np.array(cfg[k])
        print(f"case/{name}: masked {100 * ref.mean():.1f} % margin {min(margins):.2e}")

        if name in ("mad_t21", "st_t21"):  # the three public steps on their own, on the reference's own collapse
            y = np.asarray(c32, dtype=np.float64)
            m0 = np.asarray(s32) == 0
            w2 = ~m0 * np.asarray(s32, dtype=np.float64) / 2.0
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out[f"step/{name}/mask_1d"] = np.asarray(task.mask_1d(y, m0))
            out[f"step/{name}/mask_2d"] = np.asarray(task.mask_2d(y, w2))
            if cfg["mask_type"] == "sumthreshold":
                out[f"step/{name}/mask_2d_sumthreshold"] = np.asarray(task.mask_2d_sumthreshold(y, w2))
            out[f"step/{name}/y"], out[f"step/{name}/w"], out[f"step/{name}/m"] = y, w2, m0
    out["case/names"] = np.array(list(CASES))

    path = os.path.join(GOLDEN, "chisqmask.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 768 * 1024


if __name__ == "__main__":
    main()
