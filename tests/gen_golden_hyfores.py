"""Generate tests/golden/hyfores.npz and tests/golden/hyfores_apply.npz by EXECUTING the reference's own ``process``
methods from source, unmodified, through ``oracle._refstub`` on fake containers, as ``gen_golden_dayenu_hybrid.py``
does: ``ApplyDelayFilterHybridVis`` (``draco/analysis/dayenu.py:606-739``) and the five estimators and the clean task of
``draco/analysis/hyforesbandpass.py``.  Only data is committed; run where the reference checkout exists:

    python tests/gen_golden_hyfores.py

What the stubs do not supply is given here: ``task.comm`` with an ``Allreduce`` that copies (one process),
``task.min_ysep``, the speed of light, ``invert_no_zero`` and two small classes in place of the reference's
``VisBandpassWindowBaseline`` and ``VisBandpassCompensateBaseline``.

Per case the files hold the inputs (``vis`` as int16 and ``pf_hv.vis`` as int8 multiples of 1/8; the filter as one
matrix per distinct mask, ``dayenu_twin.filter_truth`` rounded to float64, plus a ``[pol, ew, ra]`` index, so that the
reference, the twin and the device read the same bits), the reference's outputs (``bandpass``, ``window`` and the
``comp_bandpass`` datasets whole, ``vis`` and ``freq_cov`` at the sampled ``(ew, ra)`` positions ``pos``) and, per
dataset, ``e_ref = max |reference - truth| / max |truth|`` with the truth of ``tests/hyfores_twin.py`` (long double,
rounded to the dataset's dtype).  ``hyfores.npz`` has the inputs and the estimators' outputs, ``hyfores_apply.npz``
those of the apply and clean tasks.

Cases: Y33 (2 x 33 x 2 x 5 x 40: all five estimators, clean with cutoff 0.1 and 0, apply with and without
``copy_weight``; three masks within 32 adjacent RA, per-polarisation flags, a skipped, a zero-filter and a
missing-frequency sample, two aliased elevations of five, a pixel mask with a whole (pol, freq) plane, a source mask),
Y70 (1 x 70 x 1 x 1 x 33: default epsilon and the attenuation flag, its seed searched as H70's), Y6 (2 x 6 x 2 x 17 x
130: ``HyFoReSBandpassHybridVis`` and apply with ``copy_tag``).

Asserted before anything is written: every float64 ``allow`` is at most 1e-9 of its dataset's largest modulus, every
``e_ref`` is at most 1e-3, no singular value of a window lies within a factor 1.25 of the cutoff, and ``allow_g``, the
Wedin bound ``3 |W+|^2 (n u sigma_max) |y|`` of the compensated gains, is at most 1e-9 relative.
"""

import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dayenu_hybrid_twin as dhtwin  # noqa: E402
import dayenu_twin  # noqa: E402
import gen_golden_dayenu_hybrid as gh  # noqa: E402
import hyfores_twin as twin  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "hyfores.npz")
GOLDEN_APPLY = os.path.join(ROOT, "tests", "golden", "hyfores_apply.npz")
DF = gh.DF
U = twin.U


class Stream(gh.HybridVisStream):
    """The fake stream with the axis properties the tasks read (``ra``, ``pol``, ``ew``)."""

    def __getattr__(self, name):
        d = self.__dict__
        if name in d.get("index_map", {}):
            return d["index_map"][name]
        return super().__getattr__(name)


class Mask(gh.Fake):
    pass


class Comm:
    def Allreduce(self, a, b, op=None):
        b[...] = a


def _small(names):
    class Small:
        def __init__(self, pol, ew, freq):
            shape = (len(pol), len(ew), len(freq))
            self.attrs = {}
            self.datasets = {names[0]: gh.DS(np.zeros(shape, dtype=np.complex128)), names[1]: gh.DS(np.zeros(shape + ((len(freq),) if names[1] == "window" else ()), dtype=np.complex128))}

        def __getattr__(self, name):
            d = self.__dict__
            if name in d.get("datasets", {}):
                return d["datasets"][name]
            raise AttributeError(name)

    return Small


def stream(c, vis, weight, **extra):
    npol, nfreq, new, nel, nra = vis.shape
    imap = {"pol": np.arange(npol), "freq": c["freq"], "ew": np.arange(new), "el": c["el"], "ra": np.arange(nra)}
    return Stream(imap, dict(vis=vis, weight=weight, **extra), attrs={"tag": "hv"})


def build_filter(freq, src_weight, tauw, eps):
    """One ``filter_truth`` matrix (rounded to float64) per distinct all-polarisation mask of ``src_weight`` and the
    ``[pol, ew, ra]`` index (-1 where no channel is valid)."""
    flag = dhtwin.sample_mask(src_weight)  # [freq, ew, ra]
    nfreq, new, nra = flag.shape
    mats, keys = [], {}
    index = np.full((src_weight.shape[0], new, nra), -1, dtype=np.int32)
    for x in range(new):
        for t in range(nra):
            fl = flag[:, x, t]
            if not fl.any():
                continue
            key = fl.tobytes()
            if key not in keys:
                keys[key] = len(mats)
                mats.append(dayenu_twin.filter_truth(freq, fl, tauw, eps).astype(np.float64))
            index[:, x, t] = keys[key]
    return np.stack(mats), index


def check_allow(name, t):
    for k in ("yN", "D", "N", "y", "W"):
        top = float(np.abs(t[k]).max())
        a = float(np.max(t[f"allow_{k}"]))
        assert a <= 1e-9 * top, (name, k, a, top)


def run_estimator(hy, out, name, kind, c):
    task = gh.make_task(getattr(hy, kind), atten_threshold=c["atten_threshold"])
    task.comm, task.min_ysep = Comm(), c["min_ysep"]
    src = stream(c, c["vis"].copy(), c["src_weight"].copy(), filter=c["filter"].copy())
    hv = stream(c, c["vis"].copy(), c["weight"].copy(), filter=c["filter"].copy())
    args = [hv]
    if kind.startswith("DelayFilter"):
        args.append(src)
    else:
        args.append(stream(c, c["pf_vis"].copy(), c["pf_weight"].copy()))
    imap = {"pol": hv.index_map["pol"], "freq": c["freq"], "ra": hv.index_map["ra"], "el": c["el"]}
    if "Mask" in kind:
        args.append(Mask(imap, dict(mask=c["mask"].copy())))
    if kind.endswith("KeepSource"):
        args.append(Mask(imap, dict(mask=c["masks"].copy())))
    bp = task.process(*args)
    assert np.array_equal(hv.vis[:], c["vis"]) and np.array_equal(hv.weight[:], c["weight"])  # (the inputs are not changed)
    y, w = np.array(bp.bandpass[:]), np.array(bp.window[:])
    t = twin.estimator(kind, c, truth=True)
    check_allow(f"{name}/{kind}", t)
    e = {"bandpass": twin.rel_err(y, t["y"].astype(np.complex128)), "window": twin.rel_err(w, t["W"].astype(np.complex128))}
    f64 = twin.estimator(kind, c)
    for k, tk in (("bandpass", "y"), ("window", "W")):
        assert e[k] <= 1e-3, (name, kind, k, e[k])
        out[f"{name}/{kind}/{k}"] = {"bandpass": y, "window": w}[k]
        out[f"{name}/{kind}/e_ref_{k}"] = np.array(e[k])
        assert np.all(np.abs(f64[tk] - t[tk]) <= t[f"allow_{tk}"]), (name, kind, k)  # the f64 twin is within the bound
    assert np.array_equal(t["D"] == 0, np.abs(y) == 0) or np.all(y[t["D"] == 0] == 0)
    print(f"{name} {kind}: e_ref bandpass {e['bandpass']:.3e} window {e['window']:.3e}, D = 0 at {int((t['D'] == 0).sum())} entries")
    return y, w


def run_apply(dayenu, out, name, label, c, **cfg):
    task = gh.make_task(dayenu.ApplyDelayFilterHybridVis, **cfg)
    src_extra = dict(filter=c["filter"].copy())
    if cfg.get("copy_weight") and cfg.get("calculate_cov"):
        src_extra["freq_cov"] = np.random.default_rng(5).normal(size=c["filter"].shape)
    src = stream(c, c["vis"].copy(), c["src_weight"].copy(), **src_extra)
    src.attrs["tag"] = "source"
    hv = stream(c, c["vis"].copy(), c["weight"].copy())
    assert task.process(hv, src) is hv
    rv, rw = np.array(hv.vis[:]), np.array(hv.weight[:])
    assert hv.attrs["tag"] == ("source" if cfg.get("copy_tag") else "hv")
    own = not cfg.get("copy_weight", False)
    tv, tw, tc, st = twin.apply_filter(c["vis"], c["weight"], c["filter"], atten_threshold=cfg.get("atten_threshold", 0.0) if own else 0.0,
                                       calculate_cov=cfg.get("calculate_cov", False) and own, truth=True)
    e = {"vis": twin.rel_err(rv, tv.astype(np.complex64))}
    pos = c["pos"]
    out[f"{name}/{label}/vis"] = np.ascontiguousarray(twin.at_positions("vis", rv, pos))
    if own:
        e["weight"] = twin.rel_err(rw, tw.astype(np.float32))
        assert np.array_equal(rw == 0, tw.astype(np.float32) == 0)
        out[f"{name}/{label}/weight"] = rw
        if cfg.get("calculate_cov"):
            rc = np.array(hv.freq_cov[:])
            e["freq_cov"] = twin.rel_err(rc, tc.astype(np.float64))
            out[f"{name}/{label}/freq_cov"] = np.ascontiguousarray(twin.at_positions("freq_cov", rc, pos))
    else:  # the weight and the covariance are the source's, bit for bit
        assert np.array_equal(rw, c["src_weight"])
        if cfg.get("calculate_cov"):
            assert np.array_equal(np.array(hv.freq_cov[:]), src_extra["freq_cov"])
    for k, v in e.items():
        assert v <= 1e-3, (name, label, k, v)
        out[f"{name}/{label}/e_ref_{k}"] = np.array(v)
    print(f"{name} {label}: e_ref " + " ".join(f"{k} {v:.3e}" for k, v in e.items()) + f", status counts {np.bincount(st.ravel(), minlength=4)}")
    return e, st, rw


def run_clean(hy, out, name, label, c, y, w, **cfg):
    task = gh.make_task(hy.DelayFilterHyFoReSBandpassHybridVisClean, **cfg)
    src = stream(c, c["vis"].copy(), c["src_weight"].copy(), filter=c["filter"].copy())
    hv = stream(c, c["vis"].copy(), c["weight"].copy())
    bp = types.SimpleNamespace(bandpass=gh.DS(y.copy()), window=gh.DS(w.copy()))
    hv2, comp = task.process(hv, src, bp)
    assert hv2 is hv
    rg, rs, rank = np.array(comp.comp_bandpass[:]), np.array(comp.sval[:]), np.array(comp.attrs["rank"])
    cutoff = cfg["cutoff"]
    assert comp.attrs["cutoff"] == cutoff
    tg, ts, trank = twin.compensate_window(w, y, cutoff)
    assert np.array_equal(rank, trank)
    allow_g = 0.0
    if cutoff > 0.0:
        n = y.shape[-1]
        for p in range(y.shape[0]):
            for x in range(y.shape[1]):
                s = ts[p, x]
                assert not np.any((s > cutoff / 1.25) & (s < cutoff * 1.25)), (name, label, p, x, s)
                kept = s[s > cutoff]
                pinv_norm = 1.0 / kept.min() if kept.size else 0.0
                allow_g = max(allow_g, 3.0 * pinv_norm**2 * (n * U * s.max()) * float(np.linalg.norm(y[p, x])))
        assert allow_g <= 1e-9 * np.abs(tg).max(), (name, label, allow_g)
        assert np.abs(rg - tg).max() <= allow_g and np.abs(rs - ts).max() <= allow_g
    else:
        assert np.array_equal(rg, y) and not rs.any() and not rank.any()
    out[f"{name}/{label}/comp_bandpass"], out[f"{name}/{label}/sval"], out[f"{name}/{label}/rank"] = rg, rs, rank
    out[f"{name}/{label}/allow_g"], out[f"{name}/{label}/cutoff"] = np.array(allow_g), np.array(cutoff)
    rv, rw = np.array(hv.vis[:]), np.array(hv.weight[:])
    tv, tw, tc, _ = twin.apply_filter(c["vis"], c["weight"], c["filter"], gain=tg, atten_threshold=cfg.get("atten_threshold", 0.0), calculate_cov=cfg.get("calculate_cov", False), truth=True)
    e = {"vis": twin.rel_err(rv, tv.astype(np.complex64)), "weight": twin.rel_err(rw, tw.astype(np.float32))}
    assert np.array_equal(rw == 0, tw.astype(np.float32) == 0)
    pos = c["pos"]
    out[f"{name}/{label}/vis"], out[f"{name}/{label}/weight"] = np.ascontiguousarray(twin.at_positions("vis", rv, pos)), rw
    if cfg.get("calculate_cov"):
        rc = np.array(hv.freq_cov[:])
        e["freq_cov"] = twin.rel_err(rc, tc.astype(np.float64))
        out[f"{name}/{label}/freq_cov"] = np.ascontiguousarray(twin.at_positions("freq_cov", rc, pos))
    for k, v in e.items():
        assert v <= 1e-3, (name, label, k, v)
        out[f"{name}/{label}/e_ref_{k}"] = np.array(v)
    print(f"{name} {label}: rank {rank.ravel()}, allow_g {allow_g:.3e}, e_ref " + " ".join(f"{k} {v:.3e}" for k, v in e.items()))
    return e


def pf_of(c):
    """A filtered stream for the estimators that take one: the truth of the apply, ``vis`` as multiples of 1/8 (int8)."""
    tv, tw, _, _ = twin.apply_filter(c["vis"], c["weight"], c["filter"], keep_input=False, truth=True)
    q = np.stack([np.clip(np.rint(tv.real.astype(np.float64) * 8), -127, 127), np.clip(np.rint(tv.imag.astype(np.float64) * 8), -127, 127)], axis=-1).astype(np.int8)
    return q, tw.astype(np.float32)


def store_inputs(out, name, c, mats, index, q, pq=None):
    for k in ("freq", "el", "weight", "src_weight", "pos"):
        out[f"{name}/{k}"] = c[k]
    out[f"{name}/min_ysep"], out[f"{name}/atten_threshold"] = np.array(c["min_ysep"]), np.array(c["atten_threshold"])
    out[f"{name}/tauw"], out[f"{name}/epsilon"] = np.array(c["tauw"]), np.array(c["epsilon"])
    out[f"{name}/vis_q"], out[f"{name}/filter_mats"], out[f"{name}/filter_index"] = q, mats, index
    if pq is not None:
        out[f"{name}/pf_vis_q"], out[f"{name}/pf_weight"] = pq, c["pf_weight"]
    if "mask" in c:
        out[f"{name}/mask"], out[f"{name}/masks"] = c["mask"], c["masks"]


def main():
    _refstub.load_reference()
    dayenu = importlib.import_module("draco.analysis.dayenu")
    dayenu.tools.invert_no_zero = _refstub._invert_no_zero
    hy = importlib.import_module("draco.analysis.hyforesbandpass")
    hy.tools.invert_no_zero = _refstub._invert_no_zero
    hy.constants = types.SimpleNamespace(c=twin.C_LIGHT)
    hy.containers.VisBandpassWindowBaseline = _small(("bandpass", "window"))
    hy.containers.VisBandpassCompensateBaseline = _small(("comp_bandpass", "sval"))
    out = {}

    # ---- Y33
    rng = np.random.default_rng(33041)
    shape = (2, 33, 2, 5, 40)
    freq = 600.0 + DF * np.arange(33)
    q, src_weight = gh.inputs(rng, freq, shape, 0.4 / 3.0)
    src_weight[:, [3, 4, 17], :, 8:16] = 0.0  # mask B, every ew
    src_weight[:, 20:26, 1, 16:24] = 0.0  # mask C on ew 1: ra 0 ... 31 of ew 1 hold A, B and C
    src_weight[1, 7, 0, 24] = 0.0  # a channel missing in one polarisation only: the per-polarisation flags differ
    src_weight[:, :, 1, 30] = 0.0  # no valid channel: skipped (and no filter)
    src_weight[:, :, 1, 31] = 0.0  # no filter ...
    weight = src_weight.copy()
    weight[:, :, 1, 31] = rng.uniform(0.5, 1.5, size=(2, 33)).astype(np.float32)  # ... for a sample with positive weight
    weight[0, 10, 0, 5] = 0.0  # a channel the filter took as valid: a missing frequency in polarisation 0
    el = np.linspace(-1.0, 1.0, 5)
    min_ysep = twin.C_LIGHT / (freq.max() * 1e6 * 1.75)  # the horizon aliases at |el| = 0.75: two of five are out
    assert twin.el_mask(el, freq, min_ysep).sum() == 3
    mats, index = build_filter(freq, src_weight, 0.4, 1e-3)
    mask = rng.uniform(size=(2, 33, 40, 5)) < 0.1
    mask[1, 12] = True  # a whole (pol, freq) plane: D = 0 and a zero row of W
    masks = (rng.uniform(size=mask.shape) < 0.05) | (mask & (rng.uniform(size=mask.shape) < 0.5))  # overlaps the pixel mask
    masks[1, 12] = False
    pos = np.array([(0, 0), (1, 39), (0, 8), (1, 16), (0, 24), (1, 30), (1, 31), (0, 5)], dtype=np.int32)
    c = dict(freq=freq, el=el, min_ysep=min_ysep, atten_threshold=0.0, tauw=0.4, epsilon=1e-3, vis=gh.vis_of(q), weight=weight, src_weight=src_weight,
             filter=twin.expand_filter(mats, index), mask=mask, masks=masks, pos=pos)
    st = twin.sample_status(weight, c["filter"])
    assert st[0, 1, 30] == twin.SKIPPED and st[0, 1, 31] == twin.ZERO_FILTER and st[0, 0, 5] == twin.MISSING_FREQ and st[1, 0, 5] == twin.OK
    assert len(mats) >= 4 and len({index[0, 1, t] for t in range(32)}) >= 3
    pq, c["pf_weight"] = pf_of(c)
    c["pf_vis"] = gh.vis_of(pq.astype(np.float64))
    store_inputs(out, "Y33", c, mats, index, q, pq)
    # the reference's own filter of the source stream: how far a filter built by the task may be from the stored one
    task = gh.make_task(dayenu.DayenuDelayFilterHybridVis, tauw=0.4, tauc=0.0, epsilon=1e-3, apply_filter=False, save_filter=True)
    s = stream(c, c["vis"].copy(), src_weight.copy())
    task.process(s)
    out["Y33/e_ref_filter"] = np.array(twin.rel_err(np.array(s.filter[:]), c["filter"]))
    print(f"Y33: {len(mats)} filters, e_ref filter {float(out['Y33/e_ref_filter']):.3e}")
    res = {k: run_estimator(hy, out, "Y33", k, c) for k in twin.KINDS}
    y, w = res[twin.KINDS[0]]
    assert np.all(res[twin.KINDS[1]][0][1, :, 12] == 0) and not res[twin.KINDS[1]][1][1, :, 12].any()
    run_clean(hy, out, "Y33", "clean", c, y, w, cutoff=0.1, calculate_cov=True)
    run_clean(hy, out, "Y33", "clean0", c, y, w, cutoff=0.0)
    run_apply(dayenu, out, "Y33", "apply", c, calculate_cov=True)
    run_apply(dayenu, out, "Y33", "apply_copy", c, calculate_cov=True, copy_weight=True)

    # ---- Y70: the attenuation flag at the default epsilon
    for seed in range(200):
        rng = np.random.default_rng(7100 + seed)
        shape = (1, 70, 1, 1, 33)
        freq = 600.0 + DF * np.arange(70)
        q, src_weight = gh.inputs(rng, freq, shape, 0.4 / 3.0)
        for t0, t1 in ((0, 12), (12, 25), (25, 33)):  # flagged stretches that leave isolated channels: the poorly attenuated ones
            start = int(rng.integers(6, 50))
            src_weight[0, start : start + 9, 0, t0:t1] = 0.0
            src_weight[0, start + 4, 0, t0:t1] = 1.0
            src_weight[0, rng.integers(0, 70, size=3), 0, t0:t1] = 0.0
        mats, index = build_filter(freq, src_weight, 0.4, 1e-12)
        c = dict(freq=freq, el=np.zeros(1), min_ysep=0.3, atten_threshold=0.1, tauw=0.4, epsilon=1e-12, vis=gh.vis_of(q), weight=src_weight.copy(), src_weight=src_weight,
                 filter=twin.expand_filter(mats, index), pos=np.array([(0, 0), (0, 12), (0, 25), (0, 32)], dtype=np.int32))
        tmp = {}
        e, _, rw = run_apply(dayenu, tmp, "Y70", "apply", c, atten_threshold=0.1)
        emax = max(e.values())
        ok = all(gh.diag_clear_of_threshold(m, 0.1, 10 * emax) for m in mats)
        removed = (rw == 0) & (src_weight > 0)
        print(f"  seed {7100 + seed}: clear of the threshold {ok}, channels removed by the attenuation flag {int(removed.any(axis=-1).sum())}")
        if not (ok and removed.any() and (rw != 0).any()):
            continue
        try:
            store_inputs(tmp, "Y70", c, mats, index, q)
            y, w = run_estimator(hy, tmp, "Y70", twin.KINDS[0], c)
            run_clean(hy, tmp, "Y70", "clean", c, y, w, cutoff=0.1, atten_threshold=0.1)
        except AssertionError as exc:
            print(f"  seed {7100 + seed}: {exc}")
            continue
        out.update(tmp)
        break
    else:
        raise RuntimeError("no seed keeps the diagonal clear of the attenuation threshold")

    # ---- Y6: RA two waves plus two
    rng = np.random.default_rng(6130)
    shape = (2, 6, 2, 17, 130)
    freq = 600.0 + DF * np.arange(6)
    q, src_weight = gh.inputs(rng, freq, shape, 0.4 / 3.0, amp=10.0)
    src_weight[:, 2, 0, 10:40] = 0.0
    src_weight[0, 4, 1, 63:] = 0.0
    src_weight[:, :, 1, 5] = 0.0
    mats, index = build_filter(freq, src_weight, 0.4, 1e-3)
    c = dict(freq=freq, el=np.linspace(-0.8, 0.8, 17), min_ysep=twin.C_LIGHT / (freq.max() * 1e6 * 1.65), atten_threshold=0.0, tauw=0.4, epsilon=1e-3, vis=gh.vis_of(q),
             weight=src_weight.copy(), src_weight=src_weight, filter=twin.expand_filter(mats, index), pos=np.array([(0, 0), (1, 129), (0, 10), (1, 63), (1, 5)], dtype=np.int32))
    pq, c["pf_weight"] = pf_of(c)
    c["pf_vis"] = gh.vis_of(pq.astype(np.float64))
    store_inputs(out, "Y6", c, mats, index, q, pq)
    run_estimator(hy, out, "Y6", "HyFoReSBandpassHybridVis", c)
    run_apply(dayenu, out, "Y6", "apply", c, copy_tag=True)

    est = {k: v for k, v in out.items() if k.split("/")[1] not in ("apply", "apply_copy", "clean", "clean0")}
    app = {k: v for k, v in out.items() if k not in est}
    for path, blob in ((GOLDEN, est), (GOLDEN_APPLY, app)):
        np.savez_compressed(path, **blob)
        print(path, os.path.getsize(path))
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
