"""Generate tests/golden/vismask.npz by EXECUTING the reference's own ``RFITransientVisMask.process``, ``stokes_I`` and
``highpass_weighted_convolution_filter`` from source (through ``oracle._refstub``), on stand-in containers.  Only the
data is committed; run where the reference checkout exists:

    python tests/gen_golden_vismask.py

Three things the reference imports are not installed and are stubbed: ``caput.algorithms.fft.fft`` is
``scipy.fft.fft``, the medians are the twin's (``tests/rfi_twin.py``), and
``skimage.filters.apply_hysteresis_threshold`` is the twin's (``tests/vismask_twin.py``).

The telescope is a ``pair_rule="halfplane"`` one of 2 cylinders x 4 feeds x 2 polarisations (under "canonical" every
baseline has three polarisation pairs and ``stokes_I`` keeps nothing): 43 stack entries, 11 Stokes-I baselines (a prime:
Bluestein), the zero separation an all-zero row.  6 frequencies from 400 MHz, 160 samples at 10 s (31 taps).  One
frequency has no weight, one is masked by the static hook; every baseline has zero-weight gaps of 1 to 3 samples, one
gap of 3 samples is common to all; bursts of several shapes are injected, and six graded runs (``make_input``) that let
SIR add samples even under a MAD window of 7.

The reference's low-pass runs through ``oaconvolve``, which transforms a complex64 input in single precision: over a
window without weight its ``ww`` is rounding noise, not zero.  Such windows are kept out of the
fixtures.  The generator refuses to write unless

* conditioning: on every row that is not all zero, ``min |ww| >= 0.05 max weight``;
* replay: the twin's replay of every case, fed the reference's own high-pass output, gives the reference's mask exactly;
* margins: every ``> sigma_low`` / ``> sigma_high`` comparison of that replay leaves a margin above 16 times the
  difference, at that comparison, to a replay fed the long-double high-pass, and of at least 1e-9 relative (NaN
  comparisons are exempt);
* coverage: every case has a masked fraction strictly between 0 and 1, at least 20 samples set by the hysteresis that
  are not above ``sigma_high``, at least 20 set only by SIR, and a ``frac_samples * nbeam`` that is not an integer; the
  ``frac_samples = 0.3`` case has a (freq, time) whose beam count is non-zero yet below the threshold.

The seed is the first one that passes; it and the smallest margin of every case are recorded in the file.
"""

import importlib
import os
import sys
import types

import numpy as np
import scipy.fft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_golden_rfi as base  # noqa: E402
import vismask_twin as twin  # noqa: E402
from gen_golden_regrid import make_task  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-9
NF, NT, CADENCE = 6, 160, 10.0
MASKED_FREQ, STATIC_FREQ = 1, 4
TEL = dict(ncyl=2, nfeed_cyl=4, npol_feed=2, pair_rule="halfplane", latitude=49.3, longitude=0.0, lsd_start=1.5e9)
LSD = 1160
GRADED = ((0, 28), (0, 128), (2, 100), (3, 48), (5, 118), (5, 20))  # (frequency, first sample) of the graded runs


class MPV(base.MP):
    @property
    def global_shape(self):
        return self.shape


def _zeros(shape, dtype=np.float64, axis=0):
    return MPV(tuple(shape), axis=axis, dtype=dtype)


class DSV(base.DSM):
    def __init__(self, arr, axis):
        super().__init__(arr, axis)
        self.arr = self.arr.view(MPV)

    @property
    def global_shape(self):
        return self.arr.shape

    shape = global_shape


class _Data:
    def __init__(self, **axes):
        super().__init__(**axes)
        self.datasets = {n: DSV(d.arr, d.attrs["axis"]) for n, d in self.datasets.items()}


class TS(_Data, base.TimeStreamC):
    pass


class SS(_Data, base.SidStreamC):
    pass


def load():
    flagging, _ = base.load()
    mp = types.SimpleNamespace(MPIArray=MPV, zeros=_zeros)
    flagging.mpiarray = mp
    flagging.transform.mpiarray = mp
    flagging.cfft = types.SimpleNamespace(fft=scipy.fft.fft)
    flagging.apply_hysteresis_threshold = twin.hysteresis
    flagging.constants = types.SimpleNamespace(c=twin.SPEED_OF_LIGHT)
    return flagging


def telescope(freq):
    from draco_amd.core.products import TransitTelescope

    return TransitTelescope(freq, lmax=1, **TEL)


def make_input(rng, tel):
    """``vis [NF, nprod, NT]`` complex64 and ``weight`` float32."""
    nprod = len(tel.uniquepairs)
    bl = np.around(tel.baselines[:, 0] + 1j * tel.baselines[:, 1], 4)
    _, cls = np.unique(bl, return_inverse=True)  # the separation class of every product
    ncls = cls.max() + 1
    t = np.arange(NT)
    ra = 2 * np.pi * CADENCE * t / 86164.0905
    rate = rng.uniform(0.0, 20.0, ncls)[cls]  # fringe rates below the filter's cut of 45 per radian
    sky = rng.uniform(1.0, 3.0, (NF, nprod, 1)) * np.exp(1j * (rate[None, :, None] * ra[None, None, :] + rng.uniform(0, 2 * np.pi, (NF, nprod, 1))))
    vis = sky + 0.5 * (rng.normal(size=(NF, nprod, NT)) + 1j * rng.normal(size=(NF, nprod, NT)))
    for _ in range(14):  # bursts: a core with wings, on all baselines, coherent or with a phase per baseline
        f, t0 = rng.integers(NF), rng.integers(8, NT - 8)
        amp, width = rng.uniform(2.0, 9.0), rng.uniform(0.7, 2.5)
        phase = rng.uniform(0, 2 * np.pi, ncls)[cls] if rng.uniform() < 0.6 else 2 * np.pi * rng.integers(0, 11) * cls / 11.0
        nfr = rng.integers(1, 3)
        vis[f : f + nfr] += amp * np.exp(-0.5 * ((t - t0) / width) ** 2)[None, None, :] * np.exp(1j * phase)[None, :, None]
    weight = rng.integers(2, 5, size=(NF, nprod, 1)).astype(np.float64) * np.ones((1, 1, NT))
    for c in range(ncls):  # gaps per baseline
        for _ in range(3):
            f, t0, n = rng.integers(NF), rng.integers(20, NT - 24), rng.integers(1, 4)
            weight[f, cls == c, t0 : t0 + n] = 0.0
    weight[:, :, 77:80] = 0.0  # a gap on all baselines
    # Graded runs, for the small windows.  With a MAD window of 7 samples a line can carry five flagged samples out of
    # six -- what SIR along time needs to add one -- only if each of them stands well above the fourth smallest deviation
    # of its own window: levels 240, 100, -, 300, 20, 4.  The three large ones sit in zero-weight gaps (of 2 and 1
    # samples, on every baseline but one), so that the low-pass does not smear them over the small ones.  The pattern over
    # baselines is a Zadoff-Chu sequence: its transform is flat, every beam sees the run.
    zc = np.exp(-1j * np.pi * np.arange(ncls) * (np.arange(ncls) + 1) / ncls)[cls]
    levels = np.array([240.0, 100.0, 0.0, 300.0, 20.0, 4.0])
    for f, t0 in GRADED:
        for j, lev in enumerate(levels):
            if lev:
                vis[f, cls != ncls - 1, t0 + j] = 0.5 * lev * zc[cls != ncls - 1]
            if lev > 50:
                weight[f, cls != ncls - 1, t0 + j] = 0.0
    weight[MASKED_FREQ] = 0.0
    return vis.astype(np.complex64), weight.astype(np.float32)


CASES = {
    "defaults": dict(),
    "all_pol": dict(stokes_i=False),
    "small_windows": dict(mad_base_size=[1, 11], mad_dev_size=[1, 7]),
    "frac30": dict(frac_samples=0.3),
    "sidereal": dict(sidereal=True),
}
BASE = dict(stokes_i=True, mad_base_size=[1, 101], mad_dev_size=[1, 51], sigma_high=8.0, sigma_low=2.0, frac_samples=0.01)


def attempt(flagging, seed):
    rng = np.random.default_rng(seed)
    freq = 400.0 + 0.390625 * np.arange(NF)[::-1]
    tel = telescope(freq)
    vis, weight = make_input(rng, tel)
    time = TEL["lsd_start"] + 86164.0905 * (LSD + 0.31) + CADENCE * np.arange(NT)
    ra = 360.0 * ((tel.unix_to_lsd(time)) % 1.0)
    static = np.zeros(NF, dtype=bool)
    static[STATIC_FREQ] = True
    out = {"in/vis": vis, "in/weight": weight, "in/freq": freq, "in/time": time, "in/ra": ra, "in/lsd": np.array(LSD), "in/static": static, "meta/seed": np.array(seed)}
    for k, v in TEL.items():
        out[f"tel/{k}"] = np.array(v)

    class Task(flagging.RFITransientVisMask):
        def _static_rfi_mask_hook(self, fq, timestamp=None):
            return static.copy()

    def stream(sidereal):
        if sidereal:
            s = SS(freq=freq, stack=np.arange(vis.shape[1]), ra=ra)
            s.attrs["lsd"] = LSD
        else:
            s = TS(freq=freq, stack=np.arange(vis.shape[1]), time=time)
        s.datasets["vis"][:], s.datasets["vis_weight"][:] = vis, weight
        return s

    # ---- Stokes I and the high-pass, on their own
    vi, wi, ubase = flagging.transform.stokes_I(stream(False), tel)
    vi, wi = np.asarray(vi), np.asarray(wi)
    out["stokes/vis"], out["stokes/weight"], out["stokes/ubase"] = vi, wi, ubase
    times_ra = np.unwrap(tel.unix_to_lsa(time), period=360.0) * np.pi / 180.0
    cut = freq.min() * 1e6 / twin.SPEED_OF_LIGHT * ubase[:, 0].max() / np.cos(np.deg2rad(tel.latitude))
    taps = twin.design(times_ra, cut)
    assert len(taps) == 31, len(taps)
    ref_hp = np.stack([flagging.filters.highpass_weighted_convolution_filter(vi[f], wi[f], times_ra, cut, axis=-1) for f in range(NF)])
    truth = twin.wconv(vi, wi, taps, highpass=True)
    e_ref = float(np.abs(ref_hp - truth).max())
    out["hp/ref"], out["hp/e_ref"], out["hp/scale"] = ref_hp, np.array(e_ref), np.array(float(np.abs(truth).max()))

    def conditioning(w):
        h = taps.astype(np.longdouble)
        c = (len(h) - 1) // 2
        wp = np.pad(w.astype(np.longdouble), [(0, 0), (0, 0), (2 * c, 2 * c)])
        ww = sum(h[j] * wp[..., 3 * c - j : 3 * c - j + NT] for j in range(len(h)))
        rows = w.any(axis=-1)
        return float(np.abs(ww[rows]).min() / w.max())

    cond = min(conditioning(wi), conditioning(weight))
    if cond < 0.05:
        return None, f"conditioning {cond:.3f}"
    out["hp/cond"] = np.array(cond)

    for name, case in CASES.items():
        case = dict(case)
        sidereal = case.pop("sidereal", False)
        cfg = dict(BASE, **case)
        task = make_task(Task, **cfg)
        task.telescope = tel
        s = stream(sidereal)
        res = task.process(s)
        assert type(res) is (base.SidMaskC if sidereal else base.RFIMaskC)
        ref = np.asarray(res.mask[:])

        if cfg["stokes_i"]:
            v, w, bl = vi, wi, ubase
        else:
            v, w, bl = vis, weight, tel.baselines
        mask0 = (w == 0).all(axis=1) | static[:, None]
        tm = tel.lsd_to_unix(LSD + ra / 360.0) if sidereal else time
        kw = dict(mad_base_size=cfg["mad_base_size"], mad_dev_size=cfg["mad_dev_size"], sigma_high=cfg["sigma_high"], sigma_low=cfg["sigma_low"], frac_samples=cfg["frac_samples"])
        ta, tb, stages = [], [], {}
        got = twin.transient_mask(v, w, mask0, freq, bl, tm, tel.unix_to_lsa, tel.latitude, trace=ta, stages=stages,
                                  hp=lambda ii, d, wt, r, c: flagging.filters.highpass_weighted_convolution_filter(d, wt, r, c, axis=-1), **kw)
        if not np.array_equal(got, ref):
            return None, f"{name}: the replay differs from the reference in {int((got != ref).sum())} samples"
        other = twin.transient_mask(v, w, mask0, freq, bl, tm, tel.unix_to_lsa, tel.latitude, trace=tb, **kw)
        if not np.array_equal(other, ref):
            return None, f"{name}: the replay on the long-double high-pass differs in {int((other != ref).sum())} samples"
        margin = np.inf
        for a, b in zip(ta, tb):
            ok = np.isfinite(a) & np.isfinite(b)
            if (np.isfinite(a) != np.isfinite(b)).any():
                return None, f"{name}: the two replays differ in where the ratio is finite"
            a, b = np.where(ok, a, 0.0), np.where(ok, b, 0.0)
            for thr in (cfg["sigma_low"], cfg["sigma_high"]):
                gap, diff = np.abs(a - thr)[ok], np.abs(a - b)[ok]
                if not (gap > 16.0 * diff).all():
                    return None, f"{name}: a comparison with {thr} has a margin of {gap[gap <= 16 * diff].min():.3e} against a difference of {diff.max():.3e}"
                margin = min(margin, float((gap / np.maximum(np.abs(a[ok]), thr)).min()))
        if margin <= MARGIN:
            return None, f"{name}: relative margin {margin:.3e}"
        nbeam = v.shape[1]
        frac = float(ref.mean())
        n_hyst = int((stages["hyst"] & ~stages["high"] & ~mask0[:, None, :]).sum())
        n_sir = int((stages["final"] & ~stages["hyst"]).sum())
        thr_count = cfg["frac_samples"] * nbeam
        checks = [0.0 < frac < 1.0, n_hyst >= 20, n_sir >= 20, thr_count != np.round(thr_count)]
        if name == "frac30":
            checks.append(bool(((stages["count"] > 0) & (stages["count"] / nbeam <= cfg["frac_samples"]) & ~mask0).any()))
        if not all(checks):
            return None, f"{name}: coverage {checks} (fraction {frac:.3f}, hysteresis {n_hyst}, SIR {n_sir})"
        out[f"case/{name}/mask"], out[f"case/{name}/margin"] = ref, np.array(margin)
        out[f"case/{name}/sidereal"] = np.array(sidereal)
        for k, val in cfg.items():
            out[f"case/{name}/{k}"] = np.array(val)
        print(f"  case/{name}: masked {100 * frac:.1f} % hysteresis-only {n_hyst} SIR-only {n_sir} margin {margin:.2e}")
    out["case/names"] = np.array(list(CASES))
    print(f"  high-pass: e_ref {e_ref:.3e} on a scale of {float(out['hp/scale']):.3f}, conditioning {cond:.3f}")
    return out, "ok"


def main():
    flagging = load()
    for seed in range(20261021, 20261021 + 40):
        out, why = attempt(flagging, seed)
        print(f"seed {seed}: {why}")
        if out is not None:
            break
    else:
        raise SystemExit("no seed passed")
    path = os.path.join(GOLDEN, "vismask.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < 1000 * 1024


if __name__ == "__main__":
    main()
