"""Generate tests/golden/mfilter.npz by EXECUTING the reference's own ``DayenuMFilter.process``,
``bandpass_mmode_filter``, ``lowpass_mmode_filter``, ``highpass_mmode_filter`` and ``instantaneous_m`` from source
(through ``oracle._refstub``, unmodified; ``caput.astro.constants.c`` is patched on the imported module at run time, as
``gen_golden_dayenu.py`` does).  Only the data is committed; run where the reference checkout exists:

    python tests/gen_golden_mfilter.py

Per stream case the file holds the inputs, the reference's outputs, the truth (``tests/mfilter_twin.py``: long-double
Cholesky inverse, mixer and apply in long double, rounded to complex64) and ``e_ref`` = max |reference - truth| /
max |truth|.  The large-order case stores no truth: at ``epsilon = 1e-4`` the reference is exact far below complex64
rounding, which a float64 Cholesky cross-check asserts here (<= 1e-9).  The functions' truth is not stored either (the
tests recompute it once with the twin); their ``e_ref`` is.

The cylinders are 2 m apart so that the cuts stay below the Nyquist rate of the short RA axes (the covariance is
positive definite only for ``a = dra m_cut / pi < 1``).
"""

import os
import sys
import types

import numpy as np
import scipy.constants
import scipy.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mfilter_twin as twin  # noqa: E402
from gen_golden_dayenu import DS, GOLDEN, make_task  # noqa: E402
from oracle import _refstub  # noqa: E402

SPACING, LATITUDE, DEC = 2.0, 49.3, 40.0


class FakeStream:
    def __init__(self, freq, ra, prodstack, vis, weight):
        self.freq, self.ra, self.prodstack = freq, ra, prodstack
        self.vis = DS(vis, ("freq", "stack", "ra"))
        self.weight = DS(weight, ("freq", "stack", "ra"))

    def redistribute(self, axis):
        pass


def make_prod(pairs):
    p = np.zeros(len(pairs), dtype=[("input_a", "<u2"), ("input_b", "<u2")])
    p["input_a"], p["input_b"] = np.array(pairs).T
    return p


def stream_inputs(rng, freq, ra_deg, sep, weight_shape):
    """Unit complex noise plus a component 1e3 times brighter at a fringe rate inside each entry's stop band."""
    ra = np.radians(ra_deg)
    nfreq, nstack, nra = weight_shape
    vis = (rng.normal(size=weight_shape) + 1j * rng.normal(size=weight_shape)) / np.sqrt(2)
    for ff, nu in enumerate(freq):
        m_cut = abs(twin.get_cut(nu, 0.5 * SPACING, LATITUDE, DEC))
        for ss, ub in enumerate(sep):
            m_stop = -0.5 * m_cut if abs(ub) < 0.5 * SPACING else twin.get_cut(nu, ub, LATITUDE, DEC) + 2.0 * m_cut
            vis[ff, ss] += 1e3 * np.exp(2j * np.pi * rng.uniform()) * np.exp(1j * m_stop * ra)
    weight = rng.uniform(0.5, 1.5, size=weight_shape).astype(np.float32)
    return vis.astype(np.complex64), weight


def run_stream(dayenu, out, name, freq, ra_deg, feedpos, prod, vis, weight, epsilon, with_truth=True):
    tel = types.SimpleNamespace(feedpositions=feedpos, cylinder_spacing=SPACING, latitude=LATITUDE)
    task = make_task(dayenu.DayenuMFilter, telescope=tel, dec=DEC, epsilon=epsilon, fkeep_intra=0.75, fkeep_inter=0.75)
    s = FakeStream(freq, ra_deg, prod, vis.copy(), weight.copy())
    task.process(s)
    rv, rw = np.array(s.vis[:]), np.array(s.weight[:])
    assert rv.dtype == np.complex64 and rw.dtype == np.float32
    sep = twin.ew_separation(feedpos, prod, SPACING)
    for ff in range(freq.size):  # no RA may sit on the 90 % threshold
        gb, flag = twin.ra_mask(weight[ff])
        if flag is not None:
            cnt = np.sum(weight[ff][gb] > 0, axis=0)
            assert np.all(np.abs(cnt - 0.90 * float(gb.size)) > 1e-6), (name, ff)
    cuts = np.array([[task._get_cut(nu, x) for x in np.concatenate([[0.5 * SPACING], sep])] for nu in freq])
    blob = dict(freq=freq, ra=ra_deg, feedpos=feedpos, prod=prod, vis=vis, weight=weight, ref_vis=rv, ref_weight=rw, cuts=cuts,
                cfg=np.array([epsilon, DEC, 0.75, 0.75, SPACING, LATITUDE]))
    if with_truth:
        tv, tw_ = twin.filter_stream(freq, ra_deg, feedpos, prod, SPACING, LATITUDE, vis, weight, DEC, epsilon, truth=True)
        e = twin.rel_err(rv, tv)
        print(f"stream {name}: e_ref {e:.3e}  max |truth| {np.abs(tv).max():.3e}")
        assert np.array_equal(rw, tw_) and np.array_equal(rv == 0, tv == 0)
        blob.update(truth_vis=tv, e_ref=np.array(e))
    for k, v in blob.items():
        out[f"{name}/{k}"] = v
    return task, rv, rw


def main():
    _refstub.load_reference()
    import importlib

    dayenu = importlib.import_module("draco.analysis.dayenu")
    dayenu.constants = types.SimpleNamespace(c=scipy.constants.c)
    out = {}

    # ---- A: three cylinders, 14 stack entries (11 with weight), both signs of the mixer, five kinds of frequency / RA
    rng = np.random.default_rng(20251001)
    nra = 70
    freq = np.array([600.0, 640.0, 680.0, 720.0])
    ra_deg = np.linspace(0.0, 360.0, nra, endpoint=False)
    feedpos = np.array([[0.0, 0.0], [0.02, 5.0], [2.0, 0.0], [2.01, 3.0], [4.0, 0.0], [3.99, 2.0]])
    pairs = [(0, 1), (2, 3), (0, 2), (2, 0), (4, 0), (1, 3), (3, 1), (5, 1), (0, 0), (2, 4), (4, 2), (2, 0), (3, 5), (1, 1)]
    prod = make_prod(pairs)
    sep = twin.ew_separation(feedpos, prod, SPACING)
    assert set(np.unique(sep)) == {-2.0, 0.0, 2.0, 4.0}
    vis, weight = stream_inputs(rng, freq, ra_deg, sep, (4, 14, nra))
    weight[:, [8, 12, 13], :] = 0.0  # outside gb, still filtered
    weight[:2, :, [5, 6, 40]] = 0.0  # masked for all
    weight[:2, 4, 20] = 0.0  # 1 of 11: kept
    weight[:2, [2, 9], 33] = 0.0  # 2 of 11: masked for everyone
    weight[2] = 0.0  # nothing to do
    weight[3, [0, 3], 0::2] = 0.0  # every RA misses 2 of 11: no RA passes
    weight[3, [1, 5], 1::2] = 0.0
    vis[:, 11], weight[:, 11] = vis[:, 3], weight[:, 3]
    _, rv, rw = run_stream(dayenu, out, "A", freq, ra_deg, feedpos, prod, vis, weight, 1e-10)
    assert np.array_equal(rv[2], vis[2]) and np.array_equal(rw[2], weight[2])
    assert np.array_equal(rv[3], vis[3]) and not rw[3].any() and rw[:2, :, 20].any() and not rv[:2, :, 33].any()
    assert np.array_equal(rv[:, 11].view(np.uint32), rv[:, 3].view(np.uint32))

    # ---- B: below one 32-row block, well conditioned
    rng = np.random.default_rng(20251002)
    nra = 24
    freq = np.array([400.0, 420.0])
    ra_deg = np.linspace(0.0, 360.0, nra, endpoint=False)
    feedpos = np.array([[0.0, 0.0], [0.0, 4.0], [2.0, 0.0]])
    prod = make_prod([(0, 1), (0, 2), (2, 1)])
    sep = twin.ew_separation(feedpos, prod, SPACING)
    vis, weight = stream_inputs(rng, freq, ra_deg, sep, (2, 3, nra))
    weight[:, :, 7] = 0.0
    weight[:, 1, 15] = 0.0
    run_stream(dayenu, out, "B", freq, ra_deg, feedpos, prod, vis, weight, 1e-6)

    # ---- C: odd order, epsilon 1e-12, a masked stretch with one kept RA
    rng = np.random.default_rng(20251003)
    nra = 161
    freq = np.array([600.0])
    ra_deg = np.linspace(0.0, 360.0, nra, endpoint=False)
    feedpos = np.array([[0.0, 0.0], [0.0, 4.0], [2.0, 0.0], [4.0, 1.0]])
    prod = make_prod([(0, 1), (0, 2), (3, 0), (2, 2)])
    sep = twin.ew_separation(feedpos, prod, SPACING)
    vis, weight = stream_inputs(rng, freq, ra_deg, sep, (1, 4, nra))
    weight[:, :, 60:69] = 0.0
    weight[:, :, 64] = 1.0
    run_stream(dayenu, out, "C", freq, ra_deg, feedpos, prod, vis, weight, 1e-12)

    # ---- large order: above 2048, off the 32 and 64 grids, well conditioned
    rng = np.random.default_rng(20251004)
    nra = 2100
    freq = np.array([600.0])
    ra_deg = np.linspace(0.0, 360.0, nra, endpoint=False)
    feedpos = np.array([[0.0, 0.0], [0.0, 4.0], [2.0, 0.0]])
    prod = make_prod([(0, 1), (0, 2), (2, 1)])
    sep = twin.ew_separation(feedpos, prod, SPACING)
    vis, weight = stream_inputs(rng, freq, ra_deg, sep, (1, 3, nra))
    weight[:, :, [3, 1000, 1001, 2077]] = 0.0
    _, rv, _ = run_stream(dayenu, out, "L", freq, ra_deg, feedpos, prod, vis, weight, 1e-4, with_truth=False)
    ra = np.radians(ra_deg)
    flag = np.all(weight[0] > 0, axis=0)
    sel = np.flatnonzero(flag)
    m_cut = abs(twin.get_cut(600.0, 0.5 * SPACING, LATITUDE, DEC))
    # the reference's own filters applied as process does, before the rounding to complex64, against a float64 Cholesky solve
    pinvs = {True: dayenu.bandpass_mmode_filter(ra, 0.625 * m_cut, 0.375 * m_cut, flag[np.newaxis, :], epsilon=1e-4)[0][0],
             False: dayenu.lowpass_mmode_filter(ra, 0.75 * m_cut, flag[np.newaxis, :], epsilon=1e-4)[0][0]}
    ref64, chol = np.zeros((3, nra), dtype=np.complex128), np.zeros((3, nra), dtype=np.complex128)
    for ss, ub in enumerate(sep):
        intra = bool(abs(ub) < 0.5 * SPACING)
        cov = twin.covariance(ra, "bandpass", 0.375 * m_cut, 0.625 * m_cut, 1e-4) if intra else twin.covariance(ra, "lowpass", 0.75 * m_cut, 0.0, 1e-4)
        mixer = np.ones(nra, dtype=np.complex128) if intra else np.exp(-1j * twin.get_cut(600.0, ub, LATITUDE, DEC) * ra)
        ref64[ss] = (pinvs[intra] @ (vis[0, ss] * mixer)) * mixer.conj()
        x = scipy.linalg.cho_solve(scipy.linalg.cho_factor(cov[np.ix_(sel, sel)]), (vis[0, ss] * mixer)[sel])
        chol[ss, sel] = x * mixer[sel].conj()
    assert np.abs(ref64 - rv[0]).max() <= 2.0**-22 * np.abs(rv).max()  # (process itself: the same numbers, rounded)
    e = float(np.abs(ref64 - chol).max() / np.abs(ref64).max())
    print(f"stream L: |reference - float64 Cholesky| / max |reference| {e:.3e} in float64")
    assert e <= 1e-9, e
    out["L/chol_check"] = np.array(e)

    # ---- functions
    nra = 96
    ra_deg = np.linspace(0.0, 360.0, nra, endpoint=False)
    ra = np.radians(ra_deg)
    m = np.ones((3, nra), dtype=bool)
    m[1, [5, 6, 40]] = False
    m[2, 10:19] = False
    m[2, 14] = True
    flag = np.stack([m[[0, 1, 0]], m[[2, 1, 0]]])
    assert flag.shape == (2, 3, nra)
    eps = 1e-10
    for kind, (mc, m0) in {"bandpass": (3.6, 6.0), "lowpass": (7.2, 0.0), "highpass": (7.2, 0.0)}.items():
        if kind == "bandpass":
            rp, rindex = dayenu.bandpass_mmode_filter(ra, m0, mc, flag, epsilon=eps)
        else:
            rp, rindex = getattr(dayenu, f"{kind}_mmode_filter")(ra, mc, flag, epsilon=eps)
        tp, tindex = twin.mmode_filter_truth(ra, kind, mc, m0, flag, eps)
        assert len(rindex) == len(tindex) == 3
        idx = np.full(flag.shape[:-1], -1)
        for u, (ind, tind) in enumerate(zip(rindex, tindex)):
            assert all(np.array_equal(a, b) for a, b in zip(ind, tind))
            idx[ind] = u
        e = twin.rel_err(rp, tp)
        print(f"functions {kind}: e_ref {e:.3e}")
        assert np.array_equal(rp == 0, tp == 0)
        for k, v in dict(ra=ra, flag=flag, par=np.array([mc, m0, eps]), ref_pinv=rp, index=idx, e_ref=np.array(e)).items():
            out[f"fn_{kind}/{k}"] = v

    # ---- instantaneous_m
    rng = np.random.default_rng(20251005)
    args = rng.uniform(-1.0, 1.0, size=(8, 6)) * np.array([np.pi, np.pi / 2, np.pi / 2, 50.0, 50.0, 5.0])
    args[0, [0, 4, 5]] = 0.0
    out["im/args"] = args
    out["im/ref"] = np.array([dayenu.instantaneous_m(*a) for a in args])

    path = os.path.join(GOLDEN, "mfilter.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
