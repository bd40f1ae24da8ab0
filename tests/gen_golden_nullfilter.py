"""Generate tests/golden/nullfilter*.npz by EXECUTING the reference's own ``null_filter``, ``DelayFilter.process`` and
``DelayFilterBase.process`` from source (through ``oracle._refstub``, unmodified; what its stubs lack, such as
``caput.astro.constants.c`` and the container classes the second task tests with ``isinstance``, is patched on the
imported module at run time).  Only the data is committed; run where the reference checkout exists:

    python tests/gen_golden_nullfilter.py

Per case the files hold the inputs, the reference's outputs, the truth (``tests/nullfilter_twin.py``: long-double
one-sided Jacobi of the real form, projector and apply in long double, rounded once), the kept rank ``nkeep`` and the
singular values ``sig`` of every distinct matrix, and ``e_ref`` = max |reference - truth| / max |truth|, for the filter
matrices and for the filtered data.  The reference's filters are complex (their imaginary part is its rounding error):
``e_ref`` of a filter is taken from the complex difference, ``e_ref`` of real data from the real part the reference
stores.

Input condition, asserted for every distinct matrix of every case: no ``sig / sig.max()`` in ``[1e-8 / 1.5, 1.5e-8]``,
and the reference's kept count (``scipy.linalg.svd`` of the complex matrix, the cut of ``null_filter``) equals the
twin's.

Files (each below 1 MiB).  ``nullfilter.npz``: the function cases and the bookkeeping of the tasks; the matrices of
order 256 and 1024 (``nullfilter_fnbig.npz``) are stored, and their ``e_ref`` is taken, on 32 rows (``rows``).  Inputs are drawn on a grid of 1/64 and
stored as int16 (``*_q``).  ``nullfilter_stream.npz``: stream NS (complex64 and complex128), ``nullfilter_stream2.npz``:
streams EW and none (complex64).  ``nullfilter_ringmap.npz`` / ``nullfilter_ringmap64.npz``: the ring map in float32
(reference output) and float64 (reference output); the ring map's truth is not stored (the tests recompute it once with
the twin: six matrices of order 64).
"""

import importlib
import logging
import os
import sys
import types

import numpy as np
import scipy.constants
import scipy.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nullfilter_twin as twin  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DF = 0.390625
BAND = (1e-8 / 1.5, 1.5e-8)
RING_CUTS = (0.2, 0.25, 0.3)  # the subclass's _delay_cut: RING_CUTS[el % 3]


class Arr(np.ndarray):
    """ndarray with the few MPIArray attributes the tasks touch."""

    def enumerate(self, axis):
        return enumerate(range(self.shape[axis]))


class DS:
    def __init__(self, arr, axis):
        self.arr = np.asarray(arr).view(Arr)
        self.attrs = {"axis": list(axis)}

    def __getitem__(self, k):
        return self.arr[k]


class FreqContainer:
    def redistribute(self, axis):
        pass


class SiderealStream(FreqContainer):
    def __init__(self, freq, prodstack, vis, weight):
        self.freq, self.prodstack = freq, prodstack
        self.datasets = {"vis": DS(vis, ("freq", "stack", "ra")), "vis_weight": DS(weight, ("freq", "stack", "ra"))}

    vis = property(lambda s: s.datasets["vis"])
    weight = property(lambda s: s.datasets["vis_weight"])


class RingMap(FreqContainer):
    def __init__(self, freq, rmap, weight):
        self.freq = freq
        self.datasets = {"map": DS(rmap, ("beam", "pol", "freq", "ra", "el")), "weight": DS(weight, ("pol", "freq", "ra", "el"))}

    weight = property(lambda s: s.datasets["weight"])


class HybridVisMModes(FreqContainer):
    pass


class GridBeam(FreqContainer):
    pass


def make_task(cls, **cfg):
    t = cls()
    t.log = logging.getLogger("gen")
    for k, v in cfg.items():
        setattr(t, k, v)
    return t


def check_matrix(name, freq, cut, K, mask, window, sig, nkeep):
    """The input condition of one distinct matrix; returns the reference's kept count."""
    rel = np.asarray(sig / sig.max(), dtype=np.float64)
    near = rel[(rel >= BAND[0]) & (rel <= BAND[1])]
    assert near.size == 0, (name, cut, K, near)
    F = mask.astype(np.float64)[:, np.newaxis] * np.exp(2.0j * np.pi * np.linspace(-cut, cut, K)[np.newaxis, :] * freq[:, np.newaxis])
    if window:
        F *= np.asarray(twin.window_coef(freq, window), dtype=np.float64)[:, np.newaxis]
    s = scipy.linalg.svd(F, compute_uv=False, lapack_driver="gesvd")
    nref = int(np.sum(s > 1e-8 * s.max()))
    assert nref == nkeep, (name, cut, K, nref, nkeep)
    gap = np.abs(np.log10(rel[rel > 0]) + 8.0).min()
    print(f"    {name}: cut {cut:.4f} K {K} unmasked {int(mask.sum())} kept {nkeep}, nearest sig / sig.max to the cut: a factor {10 ** gap:.2f}")
    return nref


def quantised(rng, shape, scale):
    """Normal draws of standard deviation ``scale`` on a grid of 1/64, as int16."""
    return np.clip(np.rint(64.0 * scale * rng.normal(size=shape)), -32000, 32000).astype(np.int16)


def store_infos(out, name, infos):
    out[f"{name}/cut"] = np.array([i[0] for i in infos])
    out[f"{name}/num_modes"] = np.array([i[1] for i in infos])
    out[f"{name}/f_mask"] = np.stack([i[2] for i in infos])
    out[f"{name}/nkeep"] = np.array([i[3] for i in infos])
    kmax = max(i[1] for i in infos)
    sig = np.zeros((len(infos), kmax))
    for r, i in enumerate(infos):
        sig[r, : i[1]] = np.asarray(i[4], dtype=np.float64)
    out[f"{name}/sig"] = sig


def function_cases(filt, out):
    cases = {
        # name: (n, cutoff, num_modes, window, type_, mask kind)
        "n64_even": (64, 0.2, 20, True, "high", "random"),
        "n64_odd": (64, 0.35, 33, False, "high", "random"),
        "n64_low": (64, 0.25, 25, True, "low", "random"),
        "n64_ones": (64, 0.2, 20, False, "high", "ones"),
        "n64_few": (64, 0.35, 34, False, "high", "few"),
        "n80_hann": (80, 0.2, 25, "hann", "low", "random"),
        "n256": (256, 0.1, 40, True, "high", "random"),
        "n1024": (1024, 0.1, 160, False, "high", "random"),
    }
    for name, (n, cut, K, window, type_, kind) in cases.items():
        freq = 600.0 + DF * np.arange(n)
        for seed in range(50):
            rng = np.random.default_rng(1000 * n + seed)
            if kind == "ones":
                mask = np.ones(n, dtype=bool)
            elif kind == "few":  # more modes than unmasked channels
                mask = np.zeros(n, dtype=bool)
                mask[rng.choice(n, size=32, replace=False)] = True
            else:
                mask = rng.uniform(size=n) > 0.15
            truth, nkeep, sig = twin.null_filter_truth(freq, cut, mask, num_modes=K, window=window, type_=type_, full=True)
            try:
                check_matrix(f"fn {name} seed {seed}", freq, cut, K, mask, window, sig, nkeep)
                break
            except AssertionError as e:
                print(f"    fn {name}: seed {seed} violates the input condition: {e}")
                if kind == "ones":
                    raise
        else:
            raise RuntimeError(f"fn {name}: no seed satisfies the input condition")
        ref = filt.null_filter(freq, cut, mask.astype(np.float64), num_modes=K, window=window, type_=type_)
        rows = np.arange(n) if n <= 80 else (np.arange(32) * (n // 32 + 1)) % n
        truth64 = truth.astype(np.float64)
        e_ref = float(np.abs(ref[rows] - truth64[rows]).max() / np.abs(truth64[rows]).max())
        print(f"fn {name}: n {n} K {K} window {window} {type_} kept {nkeep} e_ref {e_ref:.3e} (imaginary part of the reference {np.abs(ref.imag).max():.2e})")
        for k, v in dict(samples=freq, cutoff=np.array(cut), num_modes=np.array(K), mask=mask, window=np.array("" if window is False else str(window)), type=np.array(type_), rows=rows,
                         ref=ref[rows], truth=truth64[rows], nkeep=np.array(nkeep), sig=np.asarray(sig, dtype=np.float64), e_ref=np.array(e_ref)).items():
            out[f"fn_{name}/{k}"] = v
    out["fn_names"] = np.array(list(cases))


def stream_inputs(seed, freq, nstack, nt):
    rng = np.random.default_rng(seed)
    nfreq = freq.size
    vis_q = quantised(rng, (nfreq, nstack, nt, 2), 1.0)
    # a smooth component 50 times brighter: a few low delays per entry
    tau = rng.uniform(-0.08, 0.08, size=(3, nstack, nt))
    amp = rng.uniform(20.0, 50.0, size=(3, nstack, nt))
    smooth = (amp[np.newaxis] * np.exp(2j * np.pi * freq[:, None, None, None] * tau[np.newaxis])).sum(axis=1)
    vis_q = vis_q + np.rint(64.0 * np.stack([smooth.real, smooth.imag], axis=-1)).astype(np.int16)
    weight = (0.5 + rng.integers(0, 65, size=(nfreq, nstack, nt)) / 64.0).astype(np.float32)
    weight[[3, 4, 17, 30, 31, 50], 0, :] = 0.0  # channels flagged at all times
    weight[:, 0, [7, 40]] = 0.0  # samples flagged at all frequencies
    weight[[8, 9, 41], 1, :] = 0.0
    weight[:, 1, 13] = 0.0
    # entry 2: a mask that does not factorise: the maximum rule decides
    weight[10, 2, 0:9] = 0.0  # the channel has fewer samples than the others: masked
    weight[20, 2, 5] = 0.0  # likewise, and sample 5 is one short of the fullest
    weight[33, 2, :] = 0.0
    weight[:, 2, 30] = 0.0
    weight[:, 3, :] = 0.0  # all zero: both masks stay full
    vis_q[:, 4], weight[:, 4] = vis_q[:, 1], weight[:, 1]
    return vis_q, weight


def run_stream(delay, out, name, freq, feedpos, prod, vis_q, weight, dtypes, **cfg):
    tel = types.SimpleNamespace(feedpositions=feedpos)
    base = vis_q[..., 0] / 64.0 + 1j * (vis_q[..., 1] / 64.0)
    ia, ib = prod["input_a"].astype(int), prod["input_b"].astype(int)
    bl = feedpos[ia] - feedpos[ib]
    sep = {"NS": np.abs(bl[:, 1]), "EW": np.abs(bl[:, 0]), "none": np.sqrt((bl**2).sum(axis=1))}[cfg["telescope_orientation"]]
    cuts = np.maximum(cfg["za_cut"] * sep / scipy.constants.c * 1e6 + cfg["extra_cut"], cfg["delay_cut"])
    assert len(np.unique(cuts)) == 3, cuts
    blob = dict(freq=freq, feedpos=feedpos, prod=prod, vis_q=vis_q, weight=weight, cuts=cuts, orientation=np.array(cfg["telescope_orientation"]),
                cfg=np.array([cfg["delay_cut"], cfg["za_cut"], cfg["extra_cut"]]), window=np.array(bool(cfg["window"])))
    infos = None
    for dt in dtypes:
        vis = base.astype(dt)
        task = make_task(delay.DelayFilter, telescope=tel, weight_tol=1e-4, **cfg)
        s = SiderealStream(freq, prod, vis.copy(), weight.copy())
        assert task.process(s) is s
        rv, rw = np.array(s.vis[:]), np.array(s.weight[:])
        assert rv.dtype == dt and rw.dtype == np.float32
        tv, tw_, infos = twin.filter_items(freq, cuts, vis, weight, cfg["window"])
        assert np.array_equal(rw, tw_)
        assert not rw[:, 3].any() and np.array_equal(rv[:, 1], rv[:, 4])
        e = twin.rel_err(rv, tv)
        tag = np.dtype(dt).name
        print(f"stream {name} {tag}: cuts {np.round(cuts, 4)} num_modes {[i[1] for i in infos]} kept {[i[3] for i in infos]} e_ref {e:.3e}")
        blob.update({f"ref_vis_{tag}": rv, f"truth_vis_{tag}": tv, f"e_ref_{tag}": np.array(e)})
        blob["ref_weight"] = rw
    for i in infos:
        check_matrix(f"stream {name}", freq, i[0], i[1], i[2], cfg["window"], i[4], i[3])
    for k, v in blob.items():
        out[f"{name}/{k}"] = v
    store_infos(out, name, infos)


def prods(n):
    p = np.zeros(n, dtype=[("input_a", "<u2"), ("input_b", "<u2")])
    p["input_b"] = np.arange(1, n + 1)
    return p


def ringmap_inputs(seed, freq, nbeam, npol, nra, nel):
    rng = np.random.default_rng(seed)
    nfreq = freq.size
    map_q = quantised(rng, (nbeam, npol, nfreq, nra, nel), 1.0)
    tau = rng.uniform(-0.08, 0.08, size=(nbeam, npol, 1, nra, nel))
    phase = rng.uniform(0, 2 * np.pi, size=(nbeam, npol, 1, nra, nel))
    map_q = map_q + np.rint(64.0 * 60.0 * np.cos(2 * np.pi * freq[None, None, :, None, None] * tau + phase)).astype(np.int16)
    w_q = rng.integers(32, 97, size=(npol, nfreq, nra, nel)).astype(np.int16)  # weight = w_q / 64
    w_q[0, [8, 9, 41], :, :] = 0
    w_q[1, [8, 9, 41, 20], :, :] = 0  # channel 20 has half the samples of the fullest in every el: masked
    w_q[0, 12, :, 3] = 0
    w_q[:, :, 5, 11] = 0  # an RA sample without weight in both polarisations of el 11
    w_q[1, 47, 2, 17] = 0  # one pixel: the channel and the sample fall short of the fullest
    w_q[:, :, :, 6] = 0  # an el without any weight: both masks stay full
    return map_q, w_q


def run_ringmap(delay, freq, map_q, w_q, dt, window):
    cuts = np.array([RING_CUTS[e % 3] for e in range(map_q.shape[-1])])

    class VaryingCut(delay.DelayFilterBase):
        def _delay_cut(self, ss, axis, ind):
            assert axis == "el"
            return RING_CUTS[ind % 3]

    rmap, weight = (map_q / 64.0).astype(dt), (w_q / 64.0).astype(dt)
    task = make_task(VaryingCut, delay_cut=0.1, window=window, axis=None, dataset=None)
    rm = RingMap(freq, rmap.copy(), weight.copy())
    assert task.process(rm) is rm
    rv, rw = np.array(rm.datasets["map"][:]), np.array(rm.datasets["weight"][:])
    assert rv.dtype == dt and rw.dtype == dt
    tv, tw_, infos = ringmap_truth(freq, cuts, rmap, weight, window)
    assert np.array_equal(rw, tw_)
    return cuts, rv, rw, tv, infos


def ringmap_truth(freq, cuts, rmap, weight, window):
    """The twin on a ring map: an item is one el, its samples the (pol, ra) of both polarisations (all beams share it)."""
    nbeam, npol, nfreq, nra, nel = rmap.shape
    data = np.moveaxis(rmap, (2, 4), (0, 1)).reshape(nfreq, nel, nbeam * npol * nra)  # [freq, el, (beam, pol, ra)]
    wgt = np.moveaxis(weight, (1, 3), (0, 1)).reshape(nfreq, nel, npol * nra)
    fd, fw, infos = twin.filter_items(freq, cuts, data, wgt, window)
    tv = np.moveaxis(fd.reshape(nfreq, nel, nbeam, npol, nra), (0, 1), (2, 4))
    tw_ = np.moveaxis(fw.reshape(nfreq, nel, npol, nra), (0, 1), (1, 3))
    return np.ascontiguousarray(tv), np.ascontiguousarray(tw_), infos


def save(name, blob):
    path = os.path.join(GOLDEN, name)
    np.savez_compressed(path, **blob)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20), name


def main():
    _refstub.load_reference()
    filt = importlib.import_module("draco.util.filters")
    delay = importlib.import_module("draco.analysis.delay")
    delay.constants = types.SimpleNamespace(c=scipy.constants.c)
    delay.containers = types.SimpleNamespace(FreqContainer=FreqContainer, SiderealStream=SiderealStream, HybridVisMModes=HybridVisMModes, RingMap=RingMap, GridBeam=GridBeam)

    out = {}
    function_cases(filt, out)

    # ---- streams: vis [64 freq, 5 stack, 48 ra]; entries 1 and 4 share baseline, mask and input rows
    freq = 600.0 + DF * np.arange(64)
    feedpos = np.zeros((6, 2))
    feedpos[1:] = [[40.0, 14.0], [0.0, 30.0], [20.0, 55.0], [40.0, 14.0], [0.0, 30.0]]
    prod = prods(5)
    vis_q, weight = stream_inputs(64005, freq, 5, 48)
    cfg = dict(delay_cut=0.2, za_cut=1.0, extra_cut=0.15, window=False)
    s1, s2 = {}, {}
    run_stream(delay, s1, "NS", freq, feedpos, prod, vis_q, weight, (np.complex64, np.complex128), telescope_orientation="NS", **cfg)
    run_stream(delay, s2, "EW", freq, feedpos, prod, vis_q, weight, (np.complex64,), telescope_orientation="EW", **{**cfg, "window": True})
    run_stream(delay, s2, "none", freq, feedpos, prod, vis_q, weight, (np.complex64,), telescope_orientation="none", **{**cfg, "extra_cut": 0.12})
    for blob in (s1, s2):  # the bookkeeping goes to the main file, for the host tests
        for k in list(blob):
            if k.split("/")[1] in ("freq", "feedpos", "prod", "cuts", "orientation", "cfg", "window", "cut", "num_modes", "f_mask", "nkeep", "sig", "weight", "ref_weight") or k.split("/")[1].startswith("e_ref"):
                out[f"stream_{k}"] = blob[k]
    save("nullfilter_stream.npz", s1)
    save("nullfilter_stream2.npz", s2)

    # ---- ring map [2 beam, 2 pol, 64 freq, 24 ra, 20 el]
    map_q, w_q = ringmap_inputs(50221, freq, 2, 2, 24, 20)
    r32, r64 = {}, {}
    for dt, blob in ((np.float32, r32), (np.float64, r64)):
        cuts, rv, rw, tv, infos = run_ringmap(delay, freq, map_q, w_q, dt, False)
        e = twin.rel_err(rv, tv)
        print(f"ring map {np.dtype(dt).name}: {len(infos)} distinct filters, num_modes {sorted({i[1] for i in infos})} e_ref {e:.3e}")
        blob["ref_map"] = rv
        out[f"ring/e_ref_{np.dtype(dt).name}"] = np.array(e)
    for i in infos:
        check_matrix("ring map", freq, i[0], i[1], i[2], False, i[4], i[3])
    store_infos(out, "ring", infos)
    out["ring/freq"], out["ring/cuts"], out["ring/ref_weight"] = freq, cuts, rw.astype(np.float32)
    r32["map_q"], r32["w_q"] = map_q, w_q
    save("nullfilter_ringmap.npz", r32)
    save("nullfilter_ringmap64.npz", r64)
    big = {k: out.pop(k) for k in list(out) if k.startswith(("fn_n256/", "fn_n1024/"))}
    save("nullfilter_fnbig.npz", big)
    save("nullfilter.npz", out)


if __name__ == "__main__":
    main()
