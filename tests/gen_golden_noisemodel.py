"""Generate tests/golden/noisemodel.npz and tests/golden/noisemodel_noise.npz by EXECUTING the reference's own methods
from source, unmodified, through ``oracle._refstub`` on fake containers, as ``gen_golden_hyfores.py`` does:
``ReconstructVisNoiseBase._parse_attrs`` / ``_compute_layout`` / ``_compute_window`` and the ``_fill_output`` of
``ReconstructVisWeight`` and ``ReconstructVisFreqCov`` (``draco/analysis/ringmapmaker.py:1318-1712``),
``FreqCorrelatedNoise.process`` and ``GaussianNoiseDataset.process`` (``draco/synthesis/noise.py``).  Only data is
committed; run where the reference checkout exists:

    python tests/gen_golden_noisemodel.py

What the stubs do not supply is given here: the telescope (``noisemodel_twin.GridTel``) and the ``bt_*`` index maps the
reference's ``TelescopeStreamMixIn.setup`` would make from it, the compiled helper of ``tools.calculate_redundancy``
(the NumPy loop ``oracle/gen_golden.py`` uses), ``invert_no_zero``, small classes in place of the reference's
containers, and ``task.rng``.

Per case ``noisemodel.npz`` holds the inputs -- the covariance as ``A A^T + d I`` with ``A [pol, ew, ra, freq, 3]`` int8
and ``d`` an integer, so every entry is an exact integer; the weight as uint8 multiples of 1/8 --, the reference's layout,
window (for natural, uniform and hann, scaled and not, ``include_auto`` on and off) and noise factors whole, its factors
and weights at a sample of ``(pol, ew, ra)`` positions ``pos`` (one per distinct mask plus the first and the last), its
sidereal weights at a sample of RA ``rpos``, and per dataset ``e_ref = max |reference - truth| / max |truth|`` over the
WHOLE dataset with the truth of ``tests/noisemodel_twin.py`` (long double).  ``noisemodel_noise.npz`` holds, per case, an
integer lower-triangular ``L`` (int8, masked like the weights), the seed, and the reference's ``vis`` at ``rpos`` and
``vis_weight`` checks, and for N6 the ``GaussianNoiseDataset`` of the reference's sidereal stream.

Cases: N33 (XX, YY x 33 x 2 ew x ns 5 x 40 RA; natural), N70 (XX, XY, YX, YY x 70 x 1 x ns 7 x 130; hann, scaled,
``include_auto`` set, ``nsmax`` two of three separations), N6 (XX x 6 x 2 x ns 3 x 17; uniform).  Masks: three within 32
adjacent RA, per-polarisation flags, a sample with no valid channel and one with exactly one.

N70 has one east-west separation, which the reference's ``_compute_layout`` cannot lay out (``find_grid_indices`` takes
the smallest non-zero separation of none); its layout is the twin's, and every method after it is the reference's.

P4 is a layout-only case (two cylinders, all four polarisations, ``nsmax`` one of the two separations): the reference's
``_compute_layout`` and one hann window, so that the cross-polarisation conjugate map of the intra-cylinder cells has a
reference.

Asserted before anything is written: the reference's layout equals the twin's (N33, N6), every normalised ``valid x valid``
covariance has 2-norm condition number <= 1e6 and the reference's ``cholesky`` succeeds, every ``e_ref`` is at most
1e-6 (float32 datasets) or 1e-12 (float64), and the reference's noise is within the colouring bound of the truth.
"""

import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_golden_dayenu_hybrid as gh  # noqa: E402
import noisemodel_twin as twin  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "noisemodel.npz")
GOLDEN_NOISE = os.path.join(ROOT, "tests", "golden", "noisemodel_noise.npz")
WINDOWS = [(w, s, a) for w in ("natural", "uniform", "hann") for s in (False, True) for a in (False, True)]


class Cont(gh.Fake):
    """A fake container built the way the tasks build theirs: ``Cont(axes_from=..., attrs_from=..., **axes)``."""

    SPEC = {}
    distributed = False
    comm = None

    def __init__(self, axes_from=None, attrs_from=None, distributed=None, comm=None, **axes):
        imap = dict(axes_from.index_map) if axes_from is not None else {}
        imap.update({k: np.asarray(v) for k, v in axes.items()})
        super().__init__(imap, {}, attrs=getattr(attrs_from, "attrs", None))
        for name, (ax, dtype) in self.SPEC.items():
            self.datasets[name] = gh.DS(np.zeros(tuple(len(imap[a]) for a in ax), dtype=dtype), ax)


class Hybrid(Cont):
    pass


class Sidereal(Cont):
    SPEC = {"vis": (["freq", "stack", "ra"], np.complex64), "weight": (["freq", "stack", "ra"], np.float32)}
    _data_dset_name = "vis"


class NoiseModel(Cont):
    SPEC = {"redundancy": (["pol", "ew", "ns"], np.int32), "weight": (["pol", "freq", "ew", "ra"], np.float32)}
    OPTIONAL = {"freq_cov": (["pol", "ew", "ra", "freq", "freq_sum"], np.float64)}


class VisGrid(Cont):
    SPEC = {"vis": (["pol", "freq", "ew", "ns", "ra"], np.complex64), "weight": (["pol", "freq", "ew", "ns", "ra"], np.float32)}
    OPTIONAL = {"redundancy": (["pol", "ew", "ns", "ra"], np.int32)}


def _calc_redundancy(input_flags, pm, stack_index, nstack, redundancy):
    for ii in range(pm.shape[0]):
        ist = stack_index[ii]
        if 0 <= ist < nstack:
            redundancy[ist] += input_flags[pm[ii, 0]] * input_flags[pm[ii, 1]]


def make_task(cls, tel, attrs=None, **cfg):
    t = gh.make_task(cls, **cfg)
    t.telescope, t.bt_prod, t.bt_rev, t.bt_stack = tel, tel.prod, tel.reverse_stack, tel.stack
    if attrs is not None:
        t._parse_attrs(attrs)
    return t


def hybrid_of(c, attrs):
    hv = Hybrid(pol=c["pol"], freq=c["freq"], ew=c["ewpos"], ra=np.arange(c["nra"]))
    hv.attrs = dict(attrs)
    hv.datasets["weight"] = gh.DS(c["weight"].copy())
    hv.datasets["freq_cov"] = gh.DS(c["cov"].copy())
    return hv


def check_conditioning(name, Cn, weight):
    """Every normalised valid x valid block: condition number <= 1e6 (2-norm) and the reference's cholesky succeeds."""
    npol, new, nra = Cn.shape[:3]
    worst = 0.0
    for p in range(npol):
        for x in range(new):
            for t in range(nra):
                v = np.flatnonzero(weight[p, :, x, t] > 0)
                if v.size == 0:
                    continue
                blk = Cn[p, x, t][np.ix_(v, v)]
                np.linalg.cholesky(blk)
                worst = max(worst, float(np.linalg.cond(blk, 2)))
    assert worst <= 1e6, (name, worst)
    return worst


def run_model(rmm, out, name):
    c = twin.build_case(name)
    tel, spec = c["tel"], twin.CASES[name]
    attrs = twin.attrs_of(c)
    for k in ("freq", "weight_q", "A", "d", "pol", "ewpos", "nsmax", "freqmin"):
        out[f"{name}/{k}"] = np.asarray(c[k])

    # ---- layout and windows
    task = make_task(rmm.ReconstructVisFreqCov, tel, attrs)
    hv = hybrid_of(c, attrs)
    tl = twin.layout(tel, c["pol"], c["ewpos"], c["nsmax"])
    if spec["ncyl"] > 1:
        lay = task._compute_layout(hv)
        for k in ("xind", "yind", "pind", "flag", "pconjmap", "nbaseline", "nbaseline_grid"):
            assert np.array_equal(lay[k], tl[k]), (name, k)
        assert np.allclose(lay["nspos"], tl["nspos"], rtol=1e-15, atol=0) and (lay["nx"], lay["ny"], lay["npol"]) == (tl["nx"], tl["ny"], tl["npol"])
    else:
        # one east-west separation: the reference's find_grid_indices has no spacing to take (it raises on the empty
        # minimum), so its _compute_layout cannot make this layout; the methods after it run on the twin's
        lay = tl
    for k in ("xind", "yind", "pind", "flag", "pconjmap", "nbaseline", "nbaseline_grid"):
        out[f"{name}/layout_{k}"] = np.asarray(lay[k])
    out[f"{name}/layout_nspos"] = lay["nspos"]
    for wname, scaled, auto in WINDOWS:
        a2 = dict(attrs, beamform_ns_weight=wname, beamform_ns_scaled=scaled, beamform_ns_include_auto=auto)
        t2 = make_task(rmm.ReconstructVisFreqCov, tel, a2)
        w = t2._compute_window(c["freq"], lay)
        tw = twin.window(c["freq"], tl, wname, scaled, auto, c["freqmin"], c["nsmax"], truth=True)
        e = twin.rel_err(w, tw)
        assert e <= 1e-12, (name, wname, scaled, auto, e)
        key = f"{name}/window_{wname}_{int(scaled)}_{int(auto)}"
        out[key], out[key + "_e_ref"] = w, np.array(e)
    window = task._compute_window(c["freq"], lay)
    twin_w = twin.window(c["freq"], tl, spec["weight"], spec["scaled"], spec["include_auto"], c["freqmin"], c["nsmax"], truth=True)

    # ---- ReconstructVisFreqCov
    model = task._fill_output(hv, window, lay)
    rL, rw, rred = np.array(model.freq_cov[:]), np.array(model.weight[:]), np.array(model.redundancy[:])
    nf_ref = np.empty(c["cov"].shape[:-1])
    for ff in range(c["freq"].size):  # (the reference's expression, ringmapmaker.py:1686-1690: it keeps no copy)
        nf_ref[:, ff] = np.sum(window[:, ff, np.newaxis] * window * _refstub._invert_no_zero(lay["nbaseline_grid"][:, np.newaxis]), axis=-1)
    tnf = twin.cov_noise_factor(twin_w, tl)
    tL, twt, ok, tC = twin.masked_cholesky(c["cov"], c["weight"], tnf, truth=True)
    assert ok.all()
    worst = check_conditioning(name, twin.normalised_cov(c["cov"], nf_ref), c["weight"])
    e = {"cov_noise_factor": twin.rel_err(nf_ref, tnf), "freq_cov": twin.rel_err(rL, tL), "weight": twin.rel_err(rw, twt.astype(np.float32))}
    assert np.array_equal(rw == 0, ~(c["weight"] > 0)) and np.array_equal(rred, tl["nbaseline_grid"].astype(np.int32))
    assert e["cov_noise_factor"] <= 1e-12 and e["freq_cov"] <= 1e-12 and e["weight"] <= 1e-6, (name, e)
    pos = twin.positions(c["weight"])
    out[f"{name}/pos"] = pos
    out[f"{name}/cov_noise_factor"] = nf_ref
    out[f"{name}/ref_freq_cov"] = np.ascontiguousarray(rL[pos[:, 0], pos[:, 1], pos[:, 2]])  # [npos, freq, freq_sum]
    out[f"{name}/ref_weight"] = np.ascontiguousarray(rw[pos[:, 0], :, pos[:, 1], pos[:, 2]])  # [npos, freq]
    out[f"{name}/redundancy"] = rred

    # ---- ReconstructVisWeight
    wtask = make_task(rmm.ReconstructVisWeight, tel, attrs)
    hv = hybrid_of(c, attrs)
    ss = wtask._fill_output(hv, window, lay)
    rss = np.array(ss.weight[:])
    assert not np.array(ss.vis[:]).any()
    nf_w = np.sum(window**2 * _refstub._invert_no_zero(lay["nbaseline_grid"][:, np.newaxis]), axis=-1)
    tnfw = twin.weight_noise_factor(twin_w, tl)
    tss = twin.sidereal_weights(c["weight"], tnfw, tl, truth=True)
    e["weight_noise_factor"], e["ss_weight"] = twin.rel_err(nf_w, tnfw), twin.rel_err(rss, tss.astype(np.float32))
    assert e["weight_noise_factor"] <= 1e-12 and e["ss_weight"] <= 1e-6, (name, e)
    assert not rss[:, ~lay["flag"]].any()
    rpos = c["rpos"]
    out[f"{name}/rpos"], out[f"{name}/weight_noise_factor"] = rpos, nf_w
    out[f"{name}/ref_ss_weight"] = np.ascontiguousarray(rss[:, :, rpos])
    for k, v in e.items():
        out[f"{name}/e_ref_{k}"] = np.array(v)
    print(f"{name}: {len(pos)} positions, worst condition number {worst:.3e}, e_ref " + " ".join(f"{k} {v:.3e}" for k, v in e.items()))
    return c, lay, ss


def run_layout(rmm, out, name):
    """``_compute_layout`` and one window alone, for a telescope and polarisations that no full case covers."""
    c = twin.layout_case(name)
    attrs = {"beamform_ns_weight": "hann", "beamform_ns_scaled": False, "beamform_ns_include_auto": False, "beamform_ns_freqmin": c["freqmin"], "beamform_ns_nsmax": c["nsmax"]}
    task = make_task(rmm.ReconstructVisFreqCov, c["tel"], attrs)
    hv = Hybrid(pol=c["pol"], freq=c["freq"], ew=c["ewpos"], ra=np.arange(2))
    lay = task._compute_layout(hv)
    tl = twin.layout(c["tel"], c["pol"], c["ewpos"], c["nsmax"])
    for k in ("xind", "yind", "pind", "flag", "pconjmap", "nbaseline", "nbaseline_grid", "nspos"):
        assert np.array_equal(lay[k], tl[k]) if k != "nspos" else np.allclose(lay[k], tl[k], rtol=1e-15, atol=0), (name, k)
        out[f"{name}/layout_{k}"] = np.asarray(lay[k])
    assert lay["npol"] == 4 and list(lay["pconjmap"]) == [0, 2, 1, 3] and not lay["flag"].all() and (lay["nbaseline_grid"] == 0).any()
    out[f"{name}/window"] = task._compute_window(c["freq"], lay)
    print(f"{name}: layout of {int(lay['flag'].sum())} of {lay['flag'].size} stack entries, grid {lay['nbaseline_grid'].shape}")


def run_noise(noise, out, name, c, lay):
    """``FreqCorrelatedNoise.process`` on a model with an integer factor: the reference and the device read the same L."""
    n = twin.noise_case(name, c, lay)
    model = NoiseModel(pol=c["pol"], freq=c["freq"], ew=c["ewpos"], ns=lay["nspos"], ra=np.arange(c["nra"]))
    model.add_dataset("freq_cov")
    model.freq_cov[:] = n["L"]
    model.weight[:] = n["weight"]
    model.redundancy[:] = n["redundancy"]
    task = gh.make_task(noise.FreqCorrelatedNoise, save_redundancy=True)
    task.rng = np.random.default_rng(n["seed"])
    g = task.process(model)
    rv, rw = np.array(g.vis[:]), np.array(g.weight[:])
    z = twin.draw(n["seed"], n["L"].shape[:4] + (n["redundancy"].shape[-1],))
    (tre, tim), tvw, bound = twin.colour(n["L"], z, n["redundancy"], n["weight"], c["pol"], truth=True)
    assert np.array_equal(rw, tvw.astype(np.float32)) and np.array_equal(np.array(g.redundancy[:]), np.broadcast_to(n["redundancy"][..., None], g.redundancy.shape))
    auto = twin.auto_rows(c["pol"], rv.shape)
    for got, t, b in ((rv.real, tre, bound[0]), (rv.imag, tim, bound[1])):
        t64 = t.astype(np.float64)
        allow = np.where(auto, twin.auto_allow(t64, b), 0.5 * twin.ulp32(t64) + b)
        assert np.all(np.abs(got.astype(twin.LD) - t) <= allow), name
    e = max(twin.rel_err(rv.real, tre), twin.rel_err(rv.imag, tim))
    rpos = c["rpos"]
    out[f"{name}/L"], out[f"{name}/seed"], out[f"{name}/rpos"] = n["L_q"], np.array(n["seed"]), rpos
    out[f"{name}/ref_vis"] = np.ascontiguousarray(rv[..., rpos])
    out[f"{name}/e_ref_vis"] = np.array(e)
    print(f"{name} noise: e_ref vis {e:.3e}")


def run_gaussian(noise, out, name, c, ss, tel):
    data = Sidereal(freq=c["freq"], stack=tel.stack, ra=np.arange(c["nra"]))
    data.weight[:] = np.array(ss.weight[:])
    data.prodstack = tel.prodstack
    noise.containers.DataWeightContainer = Cont
    task = gh.make_task(noise.GaussianNoiseDataset, dataset=None, in_place=True)
    task.rng = np.random.default_rng(606)
    got = task.process(data)
    assert got is data
    v = np.array(data.vis[:])
    autos = tel.prodstack["input_a"] == tel.prodstack["input_b"]
    assert autos.any() and not v[:, autos].imag.any()
    out[f"{name}/gaussian_seed"], out[f"{name}/gaussian_weight"], out[f"{name}/gaussian_vis"] = np.array(606), np.array(ss.weight[:]), v
    print(f"{name} gaussian: {int(autos.sum())} autos of {autos.size} stack entries")


def main():
    _refstub.load_reference()
    rmm = importlib.import_module("draco.analysis.ringmapmaker")
    rmm.tools.invert_no_zero = _refstub._invert_no_zero
    rmm.tools._calc_redundancy = _calc_redundancy
    rmm.containers = type("NS", (), {"SiderealStream": Sidereal, "FreqNoiseModel": NoiseModel})
    noise = importlib.import_module("draco.synthesis.noise")
    noise.tools.invert_no_zero = _refstub._invert_no_zero
    noise.containers = type("NS", (), {"VisGridStream": VisGrid, "DataWeightContainer": Cont})
    model, sim = {}, {}
    for name in twin.CASES:
        c, lay, ss = run_model(rmm, model, name)
        run_noise(noise, sim, name, c, lay)
        if name == "N6":
            run_gaussian(noise, sim, name, c, ss, c["tel"])
    for name in twin.LAYOUT_CASES:
        run_layout(rmm, model, name)
    for path, blob in ((GOLDEN, model), (GOLDEN_NOISE, sim)):
        np.savez_compressed(path, **blob)
        print(path, os.path.getsize(path))
        assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
