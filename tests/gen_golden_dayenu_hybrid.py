"""Generate tests/golden/dayenu_hybrid.npz by EXECUTING the reference's own ``DayenuDelayFilterHybridVis.process``
(``draco/analysis/dayenu.py:450-572``) and ``RADependentWeights.process`` (``draco/analysis/ringmapmaker.py:1208-1315``)
from source, unmodified, through ``oracle._refstub`` on fake containers, as ``gen_golden_dayenu.py`` does.  Only the
data is committed; run where the reference checkout exists:

    python tests/gen_golden_dayenu_hybrid.py

Per case the file holds the inputs, the reference's outputs and ``e_ref = max |reference - truth| / max |truth|`` per
dataset, the truth from ``tests/dayenu_hybrid_twin.py`` (long double, rounded to the dataset's dtype).  The input
visibilities are multiples of 1/8 stored as int16.  The large outputs do not fit a committed file: ``vis`` of H33 and
every ``filter`` and ``freq_cov`` are stored at a sample of ``(ew, ra)`` positions (``pos``: one per distinct mask,
plus the first and the last RA), the ring map's datasets at a sample of RA (``rpos``).  The tests recompute the truth
with the twin and check the device against it everywhere, and against the reference at those positions.

Cases (the issue's table): H33 (apply + save + cov, order across a 16-tile and a 32-row block, mixed masks within 32
adjacent RA, a skipped sample, a single-channel sample, a channel missing in one polarisation), H70 (default epsilon,
attenuation mask, order across a 64-tile, RA one past a stripe), H6 (save only, RA one past a wave), H20 (two stop
bands), and R: ``RADependentWeights`` on H33's output for the three schemes and ``exclude_cyl`` [] and [1].
"""

import importlib
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dayenu_hybrid_twin as twin  # noqa: E402
import dayenu_twin  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "dayenu_hybrid.npz")
DF = 0.390625
_MAT5 = ["pol", "freq", "freq_sum", "ew", "ra"]
_MAT4 = ["pol", "freq", "freq_sum", "ra"]
SCHEMES = ("natural", "uniform", "inverse_variance")


class Arr(np.ndarray):
    """ndarray with the few MPIArray attributes the tasks touch."""

    local_array = property(lambda s: s.view(np.ndarray))
    local_shape = property(lambda s: s.shape)


class DS:
    def __init__(self, arr, axis=None):
        self.arr = np.asarray(arr).view(Arr)
        self.attrs = {"axis": axis}

    def __getitem__(self, k):
        return self.arr[k]

    def __setitem__(self, k, v):
        self.arr[k] = v

    shape = property(lambda s: s.arr.shape)
    local_shape = property(lambda s: s.arr.shape)


class Fake:
    OPTIONAL = {}

    def __init__(self, index_map, datasets, attrs=None):
        self.index_map, self.attrs = dict(index_map), dict(attrs or {})
        self.datasets = {k: DS(v) for k, v in datasets.items()}

    def add_dataset(self, name):
        ax, dtype = self.OPTIONAL[name]
        self.datasets[name] = DS(np.zeros(tuple(len(self.index_map[a if a != "freq_sum" else "freq"]) for a in ax), dtype=dtype), ax)

    def __contains__(self, name):
        return name in self.datasets

    def __getitem__(self, name):
        return self.datasets[name]

    def __getattr__(self, name):
        d = self.__dict__
        if name in d.get("datasets", {}):
            return d["datasets"][name]
        raise AttributeError(name)

    def redistribute(self, axis):
        pass

    @property
    def freq(self):
        return self.index_map["freq"]


class HybridVisStream(Fake):
    OPTIONAL = {"filter": (_MAT5, np.float64), "freq_cov": (_MAT5, np.float64)}


class RingMap(Fake):
    OPTIONAL = {"filter": (_MAT4, np.float64), "freq_cov": (_MAT4, np.float64)}


def hybrid(freq, vis, weight, **extra):
    npol, nfreq, new, nel, nra = vis.shape
    imap = {"pol": np.arange(npol), "freq": freq, "ew": np.arange(new), "el": np.arange(nel), "ra": np.arange(nra)}
    return HybridVisStream(imap, dict(vis=vis, weight=weight, **extra))


def make_task(cls, **cfg):
    t = cls()
    t.log = logging.getLogger("gen")
    for k, v in cfg.items():
        setattr(t, k, v)
    return t


def inputs(rng, freq, shape, tau, amp=1000.0):
    """Unit complex noise plus a smooth component ``amp`` times brighter at delay ``tau``, in multiples of 1/8 (int16),
    and float32 weights in 0.5 ... 1.5."""
    npol, nfreq, new, nel, nra = shape
    noise = (rng.normal(size=shape) + 1j * rng.normal(size=shape)) / np.sqrt(2)
    phase = np.exp(2j * np.pi * rng.uniform(size=(npol, 1, new, nel, nra)))
    v = noise + amp * phase * np.exp(2j * np.pi * freq[None, :, None, None, None] * tau)
    q = np.stack([np.rint(v.real * 8), np.rint(v.imag * 8)], axis=-1)
    assert np.abs(q).max() < 32767
    weight = rng.uniform(0.5, 1.5, size=(npol, nfreq, new, nra)).astype(np.float32)
    return q.astype(np.int16), weight


def vis_of(q):
    return ((q[..., 0] + 1j * q[..., 1]) / 8.0).astype(np.complex64)


def positions(weight):
    """One ``(ew, ra)`` per distinct mask (the skipped samples' empty mask included), plus the first and last RA."""
    flag = twin.sample_mask(weight)
    nfreq, new, nra = flag.shape
    seen, pos = set(), [(0, 0), (new - 1, nra - 1)]
    for x in range(new):
        for t in range(nra):
            key = flag[:, x, t].tobytes()
            if key not in seen:
                seen.add(key)
                if (x, t) not in pos:
                    pos.append((x, t))
    return np.array(pos, dtype=np.int32), len(seen)


def run_hybrid(dayenu, out, name, freq, q, weight, sample_vis, **cfg):
    vis = vis_of(q)
    task = make_task(dayenu.DayenuDelayFilterHybridVis, tauc=0.0, **cfg)
    task.setup()
    s = hybrid(freq, vis.copy(), weight.copy())
    task.process(s)
    rv, rw = np.array(s.vis[:]), np.array(s.weight[:])
    assert rv.dtype == np.complex64 and rw.dtype == np.float32
    kw = dict(tauw=cfg["tauw"], epsilon=cfg["epsilon"], atten_threshold=cfg.get("atten_threshold", 0.0), apply_filter=cfg.get("apply_filter", True),
              save_filter=cfg.get("save_filter", False), calculate_cov=cfg.get("calculate_cov", False))
    tv, tw_, tf, tc = twin.filter_hybrid(freq, vis, weight, truth=True, **kw)
    tv, tw_ = tv.astype(np.complex64), tw_.astype(np.float32)
    pos, nmask = positions(weight)
    e = {"vis": twin.rel_err(rv, tv), "weight": twin.rel_err(rw, tw_)}
    assert np.array_equal(rw == 0, tw_ == 0)
    blob = dict(freq=freq, vis_q=q, weight=weight, pos=pos, ref_weight=rw, tauw=np.atleast_1d(cfg["tauw"]).astype(np.float64),
                epsilon=np.atleast_1d(cfg["epsilon"]).astype(np.float64),
                cfg=np.array([kw["atten_threshold"], kw["apply_filter"], kw["save_filter"], kw["calculate_cov"]], dtype=np.float64))
    px, pt = pos[:, 0], pos[:, 1]
    blob["ref_vis"] = np.ascontiguousarray(np.moveaxis(rv[:, :, px, :, pt], 0, 0)) if sample_vis else rv  # ([npos, pol, freq, el] when sampled)
    res = {"vis": rv, "weight": rw}
    if kw["save_filter"]:
        rf = np.array(s.filter[:])
        assert all(np.array_equal(rf[0], rf[p]) for p in range(rf.shape[0]))
        e["filter"] = twin.rel_err(rf, tf.astype(np.float64))
        blob["ref_filter"] = np.ascontiguousarray(rf[0][:, :, px, pt])  # [freq, freq_sum, npos]
        res["filter"] = rf
    if kw["calculate_cov"]:
        rc = np.array(s.freq_cov[:])
        e["freq_cov"] = twin.rel_err(rc, tc.astype(np.float64))
        blob["ref_freq_cov"] = np.ascontiguousarray(rc[:, :, :, px, pt])  # [pol, freq, freq_sum, npos]
        res["freq_cov"] = rc
    print(f"{name}: {nmask} distinct masks, {len(pos)} positions, e_ref " + " ".join(f"{k} {v:.3e}" for k, v in e.items()))
    for k, v in e.items():
        blob[f"e_ref_{k}"] = np.array(v)
    for k, v in blob.items():
        out[f"{name}/{k}"] = v
    truth = {"vis": tv, "weight": tw_, "filter": None if tf is None else tf.astype(np.float64), "freq_cov": None if tc is None else tc.astype(np.float64)}
    return res, truth, e


def diag_clear_of_threshold(nf, thr, margin):
    d = np.diag(nf)
    t = thr * np.median(d[d > 0])
    return bool(np.all(np.abs(d[d > 0] - t) > margin * t))


def main():
    _refstub.load_reference()
    dayenu = importlib.import_module("draco.analysis.dayenu")
    dayenu.tools.invert_no_zero = _refstub._invert_no_zero
    rmm = importlib.import_module("draco.analysis.ringmapmaker")
    rmm.tools.invert_no_zero = _refstub._invert_no_zero
    out = {}

    # ---- H33
    rng = np.random.default_rng(33040)
    shape = (2, 33, 3, 5, 40)
    freq = 600.0 + DF * np.arange(33)
    q, weight = inputs(rng, freq, shape, 0.4 / 3.0)
    weight[:, [3, 4, 17], :, 8:16] = 0.0  # mask B, every ew
    weight[:, 20:26, 1, 16:24] = 0.0  # mask C on ew 1: ra 0 ... 31 of ew 1 hold A, B and C
    weight[1, 7, 0, 24] = 0.0  # a channel missing in one polarisation only: ra 0 ... 31 of ew 0 hold A, B and this one
    weight[:, :, 2, 30] = 0.0  # no valid channel: skipped
    weight[:, :, 2, 31] = 0.0
    weight[:, 12, 2, 31] = 0.75  # a single valid channel
    cfg33 = dict(tauw=0.4, epsilon=1e-3, atten_threshold=0.0, apply_filter=True, save_filter=True, calculate_cov=True)
    ref33, truth33, _ = run_hybrid(dayenu, out, "H33", freq, q, weight, True, **cfg33)
    flag = twin.sample_mask(weight)
    for x in (0, 1):
        assert len({flag[:, x, t].tobytes() for t in range(32)}) == 3
    assert np.array_equal(ref33["vis"][:, :, 2, :, 30], vis_of(q)[:, :, 2, :, 30]) and not ref33["filter"][:, :, :, 2, 30].any()

    # ---- H70: attenuation mask at the default epsilon
    for seed in range(200):
        rng = np.random.default_rng(7000 + seed)
        shape = (1, 70, 1, 1, 33)
        freq = 600.0 + DF * np.arange(70)
        q, weight = inputs(rng, freq, shape, 0.4 / 3.0)
        for t0, t1 in ((0, 12), (12, 25), (25, 33)):  # flagged stretches that leave isolated channels: the poorly attenuated ones
            start = int(rng.integers(6, 50))
            weight[0, start : start + 9, 0, t0:t1] = 0.0
            weight[0, start + 4, 0, t0:t1] = 1.0
            weight[0, rng.integers(0, 70, size=3), 0, t0:t1] = 0.0
        cfg70 = dict(tauw=0.4, epsilon=1e-12, atten_threshold=0.1, apply_filter=True, save_filter=False, calculate_cov=False)
        tmp = {}
        ref, truth, e = run_hybrid(dayenu, tmp, "H70", freq, q, weight, False, **cfg70)
        flag = twin.sample_mask(weight)
        emax = max(e.values())
        ok = all(diag_clear_of_threshold(dayenu_twin.filter_truth(freq, flag[:, 0, t], 0.4, 1e-12).astype(np.float64), 0.1, 10 * emax) for t in (0, 12, 25))
        removed = (ref["weight"] == 0) & flag[np.newaxis]
        kept = ref["weight"] != 0
        print(f"  seed {7000 + seed}: clear of the threshold {ok}, channels removed by the attenuation mask {int(removed.any(axis=-1).sum())}")
        if ok and removed.any() and kept.any():
            out.update(tmp)
            break
    else:
        raise RuntimeError("no seed keeps the diagonal clear of the attenuation threshold")

    # ---- H6: the filter is saved and not applied
    rng = np.random.default_rng(6065)
    shape = (2, 6, 2, 17, 65)
    freq = 600.0 + DF * np.arange(6)
    q, weight = inputs(rng, freq, shape, 0.4 / 3.0, amp=10.0)
    weight[:, 2, 0, 10:40] = 0.0
    weight[0, 4, 1, 63:] = 0.0
    weight[:, :, 1, 5] = 0.0
    cfg6 = dict(tauw=0.4, epsilon=1e-12, atten_threshold=0.0, apply_filter=False, save_filter=True, calculate_cov=False)
    ref, _, _ = run_hybrid(dayenu, out, "H6", freq, q, weight, True, **cfg6)
    assert np.array_equal(ref["vis"], vis_of(q)) and np.array_equal(ref["weight"], weight)
    del out["H6/ref_vis"], out["H6/ref_weight"]  # (the inputs, bit for bit)

    # ---- H20: two stop bands
    rng = np.random.default_rng(2020)
    shape = (1, 20, 2, 2, 9)
    freq = 600.0 + DF * np.arange(20)
    q, weight = inputs(rng, freq, shape, 0.2 / 3.0)
    weight[0, [5, 6], 1, 3:] = 0.0
    weight[0, 15, :, 7] = 0.0
    cfg20 = dict(tauw=np.array([0.2, 0.6]), epsilon=np.array([1e-3, 1e-2]), atten_threshold=0.0, apply_filter=True, save_filter=False, calculate_cov=True)
    run_hybrid(dayenu, out, "H20", freq, q, weight, False, **cfg20)

    # ---- R: RADependentWeights on H33's output
    rng = np.random.default_rng(4033)
    npol, nfreq, new, nel, nra = 2, 33, 3, 5, 40
    freq = 600.0 + DF * np.arange(33)
    rw32 = rng.uniform(0.5, 1.5, size=(npol, nfreq, nra, nel)).astype(np.float32)
    rw32[0, 9, 4, :] = 0.0
    rpos = np.array([0, 24, 31, 39], dtype=np.int32)
    fpos = np.array([9, 31], dtype=np.int32)  # (the matrices are large: two RA, one of them with a zero-weight ew)
    out["R/ring_weight"], out["R/rpos"], out["R/fpos"] = rw32, rpos, fpos
    for scheme in SCHEMES:
        for excl in ([], [1]):
            name = f"R_{scheme}_{'x'.join(str(c) for c in excl) or 'none'}"
            hv = hybrid(freq, ref33["vis"], ref33["weight"].copy(), filter=ref33["filter"].copy(), freq_cov=ref33["freq_cov"].copy())
            imap = {"pol": np.arange(npol), "freq": freq, "ra": np.arange(nra), "el": np.arange(nel)}
            rm = RingMap(imap, dict(weight=rw32.astype(np.float64)), attrs={"weight_ew": scheme, "exclude_cyl": list(excl)})
            make_task(rmm.RADependentWeights).process(hv, rm)
            tw_, tf, tc = twin.ra_dependent_weights(truth33["weight"], rw32.astype(np.float64), scheme, excl, truth33["filter"], truth33["freq_cov"], truth=True)
            got = {"weight": np.array(rm.weight[:]), "filter": np.array(rm.filter[:])}
            want = {"weight": tw_.astype(np.float64), "filter": tf.astype(np.float64)}
            assert ("freq_cov" in rm) == (scheme != "inverse_variance")
            if "freq_cov" in rm:
                got["freq_cov"], want["freq_cov"] = np.array(rm.freq_cov[:]), tc.astype(np.float64)
            e = {k: twin.rel_err(got[k], want[k]) for k in got}
            print(f"{name}: e_ref " + " ".join(f"{k} {v:.3e}" for k, v in e.items()))
            for k, v in e.items():
                out[f"{name}/e_ref_{k}"] = np.array(v)
            out[f"{name}/ref_weight"] = np.ascontiguousarray(got["weight"][:, :, rpos, :])
            out[f"{name}/ref_filter"] = np.ascontiguousarray(got["filter"][..., fpos])
            if "freq_cov" in got:
                out[f"{name}/ref_freq_cov"] = np.ascontiguousarray(got["freq_cov"][..., fpos])

    np.savez_compressed(GOLDEN, **out)
    print(GOLDEN, os.path.getsize(GOLDEN))
    assert os.path.getsize(GOLDEN) < (1 << 20)


if __name__ == "__main__":
    main()
