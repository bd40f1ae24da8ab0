"""Generate tests/golden/dayenu.npz (and dayenu_ringmap.npz, dayenu_ringmap_ref.npz) by EXECUTING the reference's own ``delay_filter``,
``highpass_delay_filter``, ``DayenuDelayFilter.process`` and ``DayenuDelayFilterMap.process`` from source (through
``oracle._refstub``, unmodified; what its stubs lack, such as ``caput.astro.constants.c``, is patched on the imported
module at run time).  Only the data is committed; run where the reference checkout exists:

    python tests/gen_golden_dayenu.py

Per case the files hold the inputs, the reference's outputs, the truth (``tests/dayenu_twin.py``: long-double
Cholesky inverse, applied in long double, rounded to the container's dtype) and ``e_ref`` = max |reference - truth| /
max |truth|, for data and for weights.  The ring map's float64 arrays do not fit one committed file: its inputs
(stored as the float32 values they were drawn as) and ``e_ref`` go to ``dayenu_ringmap.npz``, its reference outputs to
``dayenu_ringmap_ref.npz``, and its truth is not stored (the tests recompute it once with the twin).

Stream A's entries 1 and 4 share separation, mask and input rows (so four of its five cutoffs are distinct): they
must share a filter and come out bit-identical.
"""

import logging
import os
import sys
import types

import numpy as np
import scipy.constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dayenu_twin as twin  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DF = 0.390625


class LA(np.ndarray):
    """ndarray with the few MPIArray attributes the tasks touch."""

    @property
    def local_shape(self):
        return self.shape

    @property
    def local_offset(self):
        return (0,) * self.ndim


class DS:
    def __init__(self, arr, axis):
        self.arr = np.asarray(arr).view(LA)
        self.attrs = {"axis": list(axis)}

    def __getitem__(self, k):
        return self.arr[k]

    local_shape = property(lambda s: s.arr.shape)
    local_offset = property(lambda s: (0,) * s.arr.ndim)


class FakeStream:
    def __init__(self, freq, prodstack, vis, weight):
        self.freq, self.prodstack = freq, prodstack
        self.vis = DS(vis, ("freq", "stack", "ra"))
        self.weight = DS(weight, ("freq", "stack", "ra"))

    def redistribute(self, axis):
        pass


class FakeRingMap:
    def __init__(self, freq, rmap, weight):
        self.freq = freq
        nb, npol, _, nra, nel = rmap.shape
        self.index_map = {"beam": np.arange(nb), "pol": np.array(["XX", "YY"])[:npol], "freq": freq, "ra": np.arange(nra), "el": np.linspace(-1, 1, nel)}
        self.map = DS(rmap, ("beam", "pol", "freq", "ra", "el"))
        self.weight = DS(weight, ("pol", "freq", "ra", "el"))

    def redistribute(self, axis):
        pass


def make_task(cls, **cfg):
    t = cls()
    t.log = logging.getLogger("gen")
    for k, v in cfg.items():
        setattr(t, k, v)
    return t


def stream_inputs(rng, freq, cutoff, nra):
    """Unit complex noise plus a smooth component 1e4 times brighter at a third of each entry's cutoff."""
    nfreq, nstack = freq.size, len(cutoff)
    noise = (rng.normal(size=(nfreq, nstack, nra)) + 1j * rng.normal(size=(nfreq, nstack, nra))) / np.sqrt(2)
    amp = np.exp(2j * np.pi * rng.uniform(size=(1, nstack, nra)))
    smooth = 1e4 * amp * np.exp(2j * np.pi * freq[:, None, None] * (np.asarray(cutoff) / 3.0)[None, :, None])
    vis = (noise + smooth).astype(np.complex64)
    weight = rng.uniform(0.5, 1.5, size=(nfreq, nstack, nra)).astype(np.float32)
    return vis, weight


def run_stream(dayenu, out, name, freq, feedpos, prod, vis, weight, **cfg):
    tel = types.SimpleNamespace(feedpositions=feedpos)
    task = make_task(dayenu.DayenuDelayFilter, telescope=tel, single_mask=True, **cfg)
    cutoff = task._get_cut(prod)
    s = FakeStream(freq, prod, vis.copy(), weight.copy())
    task.process(s)
    rv, rw = np.array(s.vis[:]), np.array(s.weight[:])
    assert rv.dtype == np.complex64 and rw.dtype == np.float32
    tv, tw_ = twin.filter_stream(freq, cutoff, vis, weight, cfg["epsilon"], cfg.get("atten_threshold", 0.0), truth=True)
    e_v, e_w = twin.rel_err(rv, tv), twin.rel_err(rw, tw_)
    print(f"stream {name}: cutoffs {np.round(cutoff, 4)} e_ref vis {e_v:.3e} weight {e_w:.3e}  zero-weight channels ref {int((~rw.any(axis=2)).sum())} truth {int((~tw_.any(axis=2)).sum())}")
    assert np.array_equal(rw == 0, tw_ == 0)
    for k, v in dict(freq=freq, feedpos=feedpos, prod=prod, vis=vis, weight=weight, cutoff=cutoff, ref_vis=rv, ref_weight=rw, truth_vis=tv, truth_weight=tw_,
                     e_ref=np.array([e_v, e_w]), cfg=np.array([cfg["epsilon"], cfg.get("tauw", 0.1), cfg.get("za_cut", 1.0), cfg.get("atten_threshold", 0.0)]),
                     orientation=np.array(cfg.get("telescope_orientation", "NS"))).items():
        out[f"{name}/{k}"] = v
    return cutoff, max(e_v, e_w)


def prods(n):
    p = np.zeros(n, dtype=[("input_a", "<u2"), ("input_b", "<u2")])
    p["input_b"] = np.arange(1, n + 1)
    return p


def diag_clear_of_threshold(nf, thr, margin):
    d = np.diag(nf)
    t = thr * np.median(d[d > 0])
    return bool(np.all(np.abs(d[d > 0] - t) > margin * t))


def main():
    _refstub.load_reference()
    import importlib

    dayenu = importlib.import_module("draco.analysis.dayenu")
    dayenu.constants = types.SimpleNamespace(c=scipy.constants.c)
    dayenu.tools.invert_no_zero = _refstub._invert_no_zero
    out = {}

    # ---- stream A
    rng = np.random.default_rng(20250301)
    freq = 600.0 + DF * np.arange(64)
    feedpos = np.zeros((6, 2))
    feedpos[1:, 1] = [3.0, 12.2, 27.5, 40.0, 12.2]  # N-S separations of entries 0 .. 4 (4 repeats 1)
    feedpos[1:, 0] = [0.0, 22.0, 0.0, 22.0, 0.0]
    prod = prods(5)
    cfg = dict(epsilon=1e-12, tauw=0.1, za_cut=1.0, telescope_orientation="NS", atten_threshold=0.0)
    cut = 1e6 * np.abs(feedpos[1:, 1]) / scipy.constants.c + 0.1
    vis, weight = stream_inputs(rng, freq, cut, 40)
    weight[[3, 4, 17, 30, 31, 50], 1, :] = 0.0  # six channels flagged at all times
    weight[22, 2, 11] = 0.0  # one sample: the single mask removes the channel everywhere
    weight[:, 3, :] = 0.0  # skipped
    vis[:, 4], weight[:, 4] = vis[:, 1], weight[:, 1]
    run_stream(dayenu, out, "A", freq, feedpos, prod, vis, weight, **cfg)

    # ---- stream B: attenuation mask, full baseline length
    for seed in range(100):
        rng = np.random.default_rng(7100 + seed)
        freq = 600.0 + DF * np.arange(96)
        feedpos = np.zeros((4, 2))
        feedpos[1:] = [[22.0, 5.0], [0.0, 18.0], [44.0, 30.0]]
        prod = prods(3)
        cfg = dict(epsilon=1e-10, tauw=0.1, za_cut=1.0, telescope_orientation="none", atten_threshold=0.1)
        cut = 1e6 * np.sqrt((feedpos[1:] ** 2).sum(axis=1)) / scipy.constants.c + 0.1
        vis, weight = stream_inputs(rng, freq, cut, 24)
        for bb in range(3):  # flagged stretches that leave isolated channels: those are the poorly attenuated ones
            start = int(rng.integers(8, 70))
            weight[start : start + 9, bb, :] = 0.0
            weight[start + 4, bb, :] = 1.0
            weight[rng.integers(0, 96, size=4), bb, :] = 0.0
        weight[rng.integers(0, 96), 1, rng.integers(0, 24)] = 0.0
        tmp = {}
        cutoff, e = run_stream(dayenu, tmp, "B", freq, feedpos, prod, vis, weight, **cfg)
        ok = True
        for bb in range(3):
            flag = np.all(weight[:, bb] > 0, axis=-1)
            ok = ok and diag_clear_of_threshold(twin.filter_truth(freq, flag, cutoff[bb], 1e-10).astype(np.float64), 0.1, 10 * e)
        nlow = int(((tmp["B/ref_weight"] == 0).all(axis=2) & (weight > 0).all(axis=2)).sum())
        print(f"  seed {7100 + seed}: clear of the threshold {ok}, channels zeroed by the attenuation mask {nlow}")
        if ok and nlow > 0:
            out.update(tmp)
            break
    else:
        raise RuntimeError("no seed keeps the diagonal clear of the attenuation threshold")

    # ---- stream C: odd order below one tile, well conditioned
    rng = np.random.default_rng(33017)
    freq = 700.0 + 1.5625 * np.arange(33)
    feedpos = np.zeros((3, 2))
    feedpos[1:, 1] = [6.1, 30.5]
    prod = prods(2)
    cfg = dict(epsilon=1e-6, tauw=0.1, za_cut=1.0, telescope_orientation="NS", atten_threshold=0.0)
    cut = 1e6 * np.abs(feedpos[1:, 1]) / scipy.constants.c + 0.1
    vis, weight = stream_inputs(rng, freq, cut, 17)
    weight[[0, 13, 32], 1, :] = 0.0
    weight[7, 0, 16] = 0.0
    run_stream(dayenu, out, "C", freq, feedpos, prod, vis, weight, **cfg)

    # ---- functions
    rng = np.random.default_rng(64006)
    freq = 600.0 + DF * np.arange(64)
    masks = np.ones((64, 3), dtype=bool)
    masks[[5, 6, 40], 1] = False
    masks[10:19, 2] = False
    masks[14, 2] = True
    flag = masks[:, [0, 1, 0, 2, 1, 0]]
    for name, (tw, eps) in {"hp": (0.15, 1e-12), "two": ([0.1, 0.25], [1e-12, 1e-6])}.items():
        if name == "hp":
            rp, rindex = dayenu.highpass_delay_filter(freq, tw, flag, epsilon=eps)
        else:
            rp, rindex = dayenu.delay_filter(freq, flag, tw, 0.0, eps)
        tp, tindex = twin.delay_filter_truth(freq, flag, tw, eps)
        assert len(rindex) == len(tindex) and all(np.array_equal(a, b) for a, b in zip(rindex, tindex))
        e = twin.rel_err(rp, tp)
        low = np.stack([twin.atten_flag(np.diag(p), 0.1) for p in rp])
        assert all(diag_clear_of_threshold(p.astype(np.float64), 0.1, 10 * e) for p in tp)
        assert np.array_equal(low, np.stack([twin.atten_flag(np.diag(p), 0.1) for p in tp]))
        print(f"functions {name}: nuniq {len(rindex)} e_ref {e:.3e} low-attenuation channels {int((~low & (np.diagonal(rp, axis1=1, axis2=2) > 0)).sum())}")
        idx = np.full(flag.shape[1], -1)
        for u, ind in enumerate(rindex):
            idx[ind] = u
        for k, v in dict(freq=freq, flag=flag, tw=np.atleast_1d(tw), eps=np.atleast_1d(eps), ref_pinv=rp, truth_pinv=tp.astype(np.float64), index=idx, e_ref=np.array(e), low=low).items():
            out[f"fn_{name}/{k}"] = v

    # ---- ring map
    rng = np.random.default_rng(50220)
    nfreq, nra, nel = 64, 24, 20
    freq = 600.0 + DF * np.arange(nfreq)
    noise = rng.normal(size=(1, 2, nfreq, nra, nel)).astype(np.float32)
    phase = rng.uniform(0, 2 * np.pi, size=(1, 2, 1, nra, nel))
    smooth = (1e4 * np.cos(2 * np.pi * freq[None, None, :, None, None] * (0.2 / 3.0) + phase)).astype(np.float32)
    rmap32 = (noise + smooth).astype(np.float32)
    w32 = rng.uniform(0.5, 1.5, size=(2, nfreq, nra, nel)).astype(np.float32)
    w32[0, [8, 9, 41], :, :] = 0.0
    w32[1, [20, 33, 34, 35, 60], :, :] = 0.0
    w32[0, 12, :, 3] = 0.0
    w32[1, [2, 47], :, 11] = 0.0
    w32[0, 55, 5, 17] = 0.0
    w32[1, :, :, 6] = 0.0  # a fully flagged (pol, el) column
    rmap, weight = rmap32.astype(np.float64), w32.astype(np.float64)
    task = make_task(dayenu.DayenuDelayFilterMap, epsilon=1e-12, filename=None, tauw=0.2, single_mask=True, atten_threshold=0.0)
    task.setup()
    rm = FakeRingMap(freq, rmap.copy(), weight.copy())
    task.process(rm)
    rv, rw = np.array(rm.map[:]), np.array(rm.weight[:])
    tv, tw_ = twin.filter_ringmap(freq, 0.2, rmap, weight, 1e-12, 0.0, truth=True)
    e_v, e_w = twin.rel_err(rv, tv), twin.rel_err(rw, tw_)
    print(f"ring map: e_ref map {e_v:.3e} weight {e_w:.3e}")
    assert np.array_equal(rw == 0, tw_ == 0) and np.array_equal(rv[0, 1, :, :, 6], rmap[0, 1, :, :, 6])
    rout = dict(freq=freq, map=rmap32, weight=w32, e_ref=np.array([e_v, e_w]), cfg=np.array([1e-12, 0.2]))

    for name, blob in (("dayenu.npz", out), ("dayenu_ringmap.npz", rout), ("dayenu_ringmap_ref.npz", dict(ref_map=rv, ref_weight=rw))):
        path = os.path.join(GOLDEN, name)
        np.savez_compressed(path, **blob)
        print(path, os.path.getsize(path))
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
