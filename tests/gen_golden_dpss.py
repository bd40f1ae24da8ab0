"""Generate tests/golden/dpss.npz (and dpss_basis_f1024.npz, dpss_basis_r1100.npz) by EXECUTING the reference's own
``dpss.make_covariance``, ``get_basis``, ``project``, ``solve``, ``filter``, ``inpaint``, ``flag_above_cutoff`` and the
``process`` method of ``DPSSFilter``, ``DPSSFilterDelayStokesI`` and ``DPSSFilterMMode`` from source (through
``oracle._refstub``, unmodified).  On the imported modules the ``config.enum`` attributes (``axis``,
``telescope_orientation``) are set on the instances (the stub returns ``None`` for them), ``mpitools.allreduce`` is the
identity and ``constants`` carries SciPy's ``c``.  Only the data is committed; run where the reference checkout exists:

    python tests/gen_golden_dpss.py

Per case the file holds the inputs, the basis the reference used (float32), the reference's outputs, the truth
(``tests/dpss_twin.py`` in long double, rounded to complex64 / float32), ``e_ref`` (the reference against the truth) and
``e_f64`` (the float64 twin against the truth), for data (``max |got - truth| / max |truth|``) and for weights (largest
elementwise relative error where the truth is non-zero; the zero patterns are asserted equal).  The bases of the two
large function cases (1024 frequencies, 1100 right ascensions) take 0.9 MB each and go to files of their own.

Asserted here: for every cut the eigenvalues next to the ``1e-12 lambda_max`` cut lie a factor 3 from it on both sides
(the cut is searched for that; at orders 1024 and 1100 neighbouring eigenvalues are only a factor 5.7 apart there, so
the search asks for a factor 2.3 on both sides, the most there is); every cut lies below the Nyquist rate of its axis; no cutoff ``fc`` is an integer;
no PCHIP value lies within 1e-6 of zero relative to its column's largest; the variance identity of the library agrees
with the direct form in long double.
"""

import logging
import os
import sys
import types

import numpy as np
import scipy.constants
import scipy.linalg
from scipy.interpolate import PchipInterpolator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dpss_twin as twin  # noqa: E402
from oracle import _refstub  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DF = 0.390625
EPS = 1e-3


class LA(np.ndarray):
    """ndarray with the few MPIArray attributes the tasks touch (the stack axis is the distributed one)."""

    local_shape = property(lambda s: s.shape)
    local_bounds = property(lambda s: slice(0, s.shape[1]))
    local_array = property(lambda s: s)


class DS:
    def __init__(self, arr, axis):
        self.arr = np.asarray(arr).view(LA)
        self.attrs = {"axis": list(axis)}

    def __getitem__(self, k):
        return self.arr[k]

    local_shape = property(lambda s: s.arr.shape)


class FakeStream:
    def __init__(self, freq, ra, stack, prodstack, vis, weight):
        self.freq, self.ra, self.stack, self.prodstack = freq, ra, stack, prodstack
        self.vis = DS(vis, ("freq", "stack", "ra"))
        self.weight = DS(weight, ("freq", "stack", "ra"))

    def redistribute(self, axis):
        pass

    def copy(self):
        return FakeStream(self.freq, self.ra, self.stack, self.prodstack, np.array(self.vis.arr), np.array(self.weight.arr))


def make_task(cls, **cfg):
    t = cls()
    t.log = logging.getLogger("gen")
    for k, v in cfg.items():
        setattr(t, k, v)
    return t


def cut_margin(samples, hw):
    """``(k, lambda_k / cut, cut / lambda_{k+1})`` of the basis of one cut."""
    ev = np.sort(scipy.linalg.eigh(np.sinc(2.0 * hw * np.subtract.outer(samples, samples)), eigvals_only=True, check_finite=False, driver="evd"))[::-1]
    cut = 1e-12 * ev.max()
    k = int((ev > cut).sum())
    below = abs(ev[k]) if k < ev.size else 0.0
    return k, ev[k - 1] / cut, cut / max(below, 1e-300)


def search_cut(samples, hw, step, decimals, need=3.0):
    """The first cut at or above ``hw`` (on the grid the tasks round to) whose neighbours clear the cut by the factor
    ``need``."""
    nyq = 0.5 / np.median(np.abs(np.diff(samples)))
    for t in range(200):
        h = round(hw + t * step, decimals)
        assert h < nyq, (h, nyq)
        k, up, down = cut_margin(samples, h)
        if up >= need and down >= need:
            return h, k
    raise AssertionError("no cut found")


def make_columns(rng, n, ncol, samples, hw, fc, specials):
    """In-band tones plus 1 % noise, weights uniform in [0.5, 1.5], gaps 1 to 4 wide, and the special gaps / columns."""
    x = np.zeros((n, ncol), dtype=np.complex128)
    for _ in range(4):
        tau = rng.uniform(-0.8 * hw, 0.8 * hw, size=ncol)
        amp = rng.uniform(0.5, 2.0, size=ncol) * np.exp(2j * np.pi * rng.uniform(size=ncol))
        x += amp[np.newaxis, :] * np.exp(2j * np.pi * samples[:, np.newaxis] * tau[np.newaxis, :])
    x += 1.0 + 0.5j  # (a mean for step 1 to remove)
    x += 0.01 * (rng.normal(size=x.shape) + 1j * rng.normal(size=x.shape))
    w = rng.uniform(0.5, 1.5, size=(n, ncol)).astype(np.float32)
    for c in range(ncol):
        i = int(rng.integers(3, 9))
        while i < n - 8:
            width = int(rng.integers(1, 5))
            w[i : i + width, c] = 0.0
            i += width + int(rng.integers(6, 16))
    wide = int(np.floor(fc)) + 3
    assert wide < n // 2
    w[n // 2 : n // 2 + wide, 0] = 0.0  # wider than the cutoff
    w[n // 2 - 1, 0] = w[n // 2 + wide, 0] = 1.0
    c1 = min(1, ncol - 1)
    w[:3, c1] = 0.0  # a gap at each end of the axis
    w[-2:, c1] = 0.0
    c2 = min(2, ncol - 1)
    w[n // 3 - 1 : n // 3 + 2, c2] = [1.25, 0.0, 0.75]  # one isolated flagged sample
    if specials:
        assert ncol >= 8
        w[:, 5] = 0.0  # fully flagged
        w[:, 6] = 0.0  # a single valid sample
        w[n // 4, 6] = 1.0
        w[:, 7] = 0.0  # two valid samples
        w[[n // 5, n // 2 + 1], 7] = [0.6, 1.5]  # (its interpolant crosses zero between samples)
    return x.astype(np.complex64), w


def check_pchip(w):
    n = w.shape[0]
    for c in range(w.shape[1]):
        sel = w[:, c] > 0
        if sel.sum() < 2:
            continue
        p = PchipInterpolator(np.arange(n)[sel], 1.0 / w[sel, c].astype(np.float64), extrapolate=True)(np.arange(n))
        assert np.all(np.abs(p) > 1e-6 * np.abs(p).max()), c


def errors(name, rv, rw, tv, tw, fv, fw):
    e_ref_v, (e_ref_w, same_r) = twin.rel_err(rv, tv), twin.weight_err(rw, tw)
    e_f64_v, (e_f64_w, same_f) = twin.rel_err(fv, tv), twin.weight_err(fw, tw)
    print(f"{name}: e_ref vis {e_ref_v:.3e} weight {e_ref_w:.3e}   e_f64 vis {e_f64_v:.3e} weight {e_f64_w:.3e}")
    assert same_r and same_f, name
    return np.array([e_ref_v, e_ref_w]), np.array([e_f64_v, e_f64_w])


def function_case(dpss, out, name, seed, samples, hw, step, ncol, specials, basis_file=None, need=3.0):
    rng = np.random.default_rng(seed)
    n = samples.size
    hw, k = search_cut(samples, hw, step, 4, need)
    fs = 1.0 / np.median(np.abs(np.diff(samples)))
    fc = fs / hw
    assert abs(fc - round(fc)) > 1e-3, fc
    A = dpss.get_basis(dpss.make_covariance(samples, hw, 0.0))
    assert A.dtype == np.float32 and A.shape == (n, k)
    x, w = make_columns(rng, n, ncol, samples, hw, fc, specials)
    check_pchip(w)
    W = w > 0
    cond = []
    for c in range(ncol):
        if W[:, c].any():
            ev = np.linalg.eigvalsh((A.T.astype(np.float64) * w[:, c]) @ A.astype(np.float64) + EPS * np.eye(k))
            cond.append(ev.max() / ev.min())
    print(f"{name}: n {n} k {k} ncol {ncol} cut {hw} fc {fc:.3f} cond(C) <= {max(cond):.3e}")
    assert max(cond) < 1.5e3
    rxp = dpss.project(x, w, A)
    rsx, rsw = dpss.solve(rxp.copy(), w.copy(), A, EPS)
    rfx, rfw = dpss.filter(x.copy(), w.copy(), A, W, EPS)
    rix, riw = dpss.inpaint(x.copy(), w.copy(), A, W, EPS)
    rflag = dpss.flag_above_cutoff(W, fc)
    assert rfx.dtype == np.complex64 and rfw.dtype == np.float32
    assert np.array_equal(rflag, twin.flag_above_cutoff(W, fc))
    assert not rflag[n // 2 : n // 2 + int(np.floor(fc)) + 3, 0].any() and not rflag[:3, min(1, ncol - 1)].any()
    tv, tw = twin.filter_columns(x, w, A, W, EPS, ld=True)
    iv, iw = twin.filter_columns(x, w, A, W, EPS, ld=True, variance="identity")
    # the identity, in long double: both forms give the variance to a few u cond(C) |a_i|^2 / Si, u = 2**-64, |a_i| <= 1
    dvar = float(np.abs(twin.inz(iw) - twin.inz(tw)).max())
    print(f"{name}: identity against direct form in long double: variance {dvar:.3e} weight {twin.weight_err(iw, tw)[0]:.3e} vis {twin.rel_err(iv, tv):.3e}")
    assert dvar < 1e-15 / EPS and twin.rel_err(iv, tv) < 1e-15
    fv, fw = twin.filter_columns(x, w, A, W, EPS, ld=False)
    tv, tw, fv, fw = tv.astype(np.complex64), tw.astype(np.float32), fv.astype(np.complex64), fw.astype(np.float32)
    e_ref, e_f64 = errors(name, rfx, rfw, tv, tw, fv, fw)
    # the reference's inpaint is its filter with the input put back where W is set: not stored
    assert np.array_equal(rix[~W], rfx[~W]) and np.array_equal(riw[~W], rfw[~W]) and np.array_equal(rix[W], x[W]) and np.array_equal(riw[W], w[W])
    blob = dict(samples=samples, cut=np.array(hw), fc=np.array(fc), x=x, w=w, ref_filter_x=rfx, ref_filter_w=rfw, ref_flag=rflag, truth_x=tv, truth_w=tw, e_ref=e_ref, e_f64=e_f64)
    if basis_file is None:  # (the large cases do not store project and solve either: the file has to stay below 1 MiB)
        blob.update(A=A, ref_project=rxp, ref_solve_x=rsx, ref_solve_w=rsw)
    else:
        path = os.path.join(GOLDEN, basis_file)
        np.savez_compressed(path, A=A)
        print(path, os.path.getsize(path))
        assert os.path.getsize(path) < (1 << 20)
    for key, v in blob.items():
        out[f"{name}/{key}"] = v


def task_case(interp, out, name, cls_name, seed, freq, ra, axis, stack, prodstack, telescope, cfg, nshape):
    rng = np.random.default_rng(seed)
    samples = freq if axis == "freq" else ra
    cls = getattr(interp, cls_name)
    task = make_task(cls, inpaint=True, axis=axis, iter_axes=["stack", "el"], epsilon=EPS, cutoff_frac=1.0, copy=True, mask=None, telescope=telescope,
                     telescope_orientation="NS", **cfg)
    nfreq, nstack, nra = nshape
    n = samples.size
    # the cuts the task will use, each moved to the next one that clears the eigenvalue cut (through extra_cut / halfwidths)
    data = FakeStream(freq, ra, stack, prodstack, np.zeros(nshape, np.complex64), np.ones(nshape, np.float32))
    task._set_sel(data)
    modes, amap, cutoff = task._get_basis(samples)
    cuts = np.array(task.halfwidths if cls_name == "DPSSFilter" else np.unique(task._get_baseline_cuts()), dtype=np.float64)
    nyq = 0.5 / np.median(np.abs(np.diff(samples)))
    for h, A in zip(cuts, modes):
        k, up, down = cut_margin(samples, h)
        print(f"{name}: cut {h} k {k} margins {up:.2f} {down:.2f}")
        assert up >= 3.0 and down >= 3.0 and h < nyq and A.shape == (n, k), (name, h)
    assert abs(cutoff - round(cutoff)) > 1e-3, cutoff
    ncs = nra if axis == "freq" else nfreq
    vis, weight = np.zeros(nshape, np.complex64), np.zeros(nshape, np.float32)
    for s in range(nstack):
        x, w = make_columns(rng, n, ncs, samples, float(cuts[amap[s]]), cutoff, False)
        check_pchip(w)
        if axis == "freq":
            vis[:, s, :], weight[:, s, :] = x, w
        else:
            vis[:, s, :], weight[:, s, :] = x.T, w.T
    data = FakeStream(freq, ra, stack, prodstack, vis.copy(), weight.copy())
    res = task.process(data)
    assert res is not data and np.array_equal(data.vis[:], vis) and np.array_equal(data.weight[:], weight)
    rv, rw = np.array(res.vis[:]), np.array(res.weight[:])
    assert rv.dtype == np.complex64 and rw.dtype == np.float32
    ax = 0 if axis == "freq" else 2
    tv, tw = twin.task_columns(vis, weight, ax, modes, amap, EPS, cutoff, True, ld=True)
    fv, fw = twin.task_columns(vis, weight, ax, modes, amap, EPS, cutoff, True, ld=False)  # (rounded, as the truth)
    e_ref, e_f64 = errors(name, rv, rw, tv, tw, fv, fw)
    blob = dict(freq=freq, ra=ra, vis=vis, weight=weight, ref_vis=rv, ref_weight=rw, truth_vis=tv, truth_weight=tw, e_ref=e_ref, e_f64=e_f64,
                cuts=cuts, amap=np.asarray(amap), cutoff=np.array(cutoff), axis=np.array(axis))
    for i, A in enumerate(modes):
        blob[f"A{i}"] = A
    if stack is not None:
        blob["stack"] = stack
    if prodstack is not None:
        blob.update(prodstack=prodstack, feedmap=telescope.feedmap, baselines=telescope.baselines, freq_start=np.array(telescope.freq_start), latitude=np.array(telescope.latitude))
    for key, v in cfg.items():
        blob[f"cfg_{key}"] = np.asarray(v)
    if cls_name != "DPSSFilter":
        blob["baseline_cuts"] = np.asarray(task._get_baseline_cuts())
    for key, v in blob.items():
        out[f"{name}/{key}"] = v


def main():
    _refstub.load_reference()
    import importlib

    dpss = importlib.import_module("draco.util.dpss")
    interp = importlib.import_module("draco.analysis.interpolate")
    dpss.invert_no_zero = _refstub._invert_no_zero
    interp.constants = types.SimpleNamespace(c=scipy.constants.c)
    interp.mpitools = types.SimpleNamespace(allreduce=lambda x, op=None: x, MIN=None)
    out = {}

    freq = lambda n: 800.0 - DF * np.arange(n)  # noqa: E731
    radeg = lambda n: np.linspace(0.0, 360.0, n, endpoint=False)  # noqa: E731

    # ---- functions: (n, starting cut, step of the search, columns, special columns)
    function_case(dpss, out, "f70", 20261101, freq(70), 0.3, 0.001, 33, True)
    function_case(dpss, out, "f161", 20261102, freq(161), 0.2, 0.001, 5, False)
    function_case(dpss, out, "r140", 20261103, radeg(140), 0.04, 0.001, 9, True)
    # (near the cut the eigenvalues of these two orders are a factor 5.7 apart: a factor 3 on both sides does not exist)
    function_case(dpss, out, "f1024", 20261104, freq(1024), 0.25, 0.0005, 5, False, basis_file="dpss_basis_f1024.npz", need=2.3)
    function_case(dpss, out, "r1100", 20261105, radeg(1100), 0.27, 0.0005, 1, False, basis_file="dpss_basis_r1100.npz", need=2.3)

    # ---- DPSSFilter: one constant cut along frequency
    f = freq(70)
    hw, _ = search_cut(f, 0.3, 0.001, 3)
    task_case(interp, out, "t_plain", "DPSSFilter", 20261111, f, radeg(5), "freq", None, None, None, dict(halfwidths=[hw], centres=[0.0]), (70, 3, 5))

    # ---- DPSSFilterDelayStokesI: two distinct delay cuts along frequency (the stack axis holds the baselines)
    f = freq(161)
    h0, _ = search_cut(f, 0.2, 0.001, 3)
    h1, _ = search_cut(f, 0.3, 0.001, 3)
    stack = np.array([[0.0, 0.0], [22.0, 10.0], [0.0, (h1 - 0.0) * 1e-6 * scipy.constants.c], [22.0, 5.0]])
    task_case(interp, out, "t_delay", "DPSSFilterDelayStokesI", 20261112, f, radeg(3), "freq", stack, None, None, dict(halfwidths=[h0], centres=[0.0], za_cut=1.0, extra_cut=0.0), (161, 4, 3))
    assert np.array_equal(out["t_delay/cuts"], [h0, h1]), out["t_delay/cuts"]

    # ---- DPSSFilterMMode: two distinct m cuts along RA, baselines through the telescope's feedmap
    ra = radeg(140)
    m0, _ = search_cut(ra, 0.04, 0.01, 2)
    m1, _ = search_cut(ra, 0.10, 0.01, 2)
    lat, fstart = 49.3, 600.0
    bx = m1 * scipy.constants.c * np.cos(np.deg2rad(lat)) / ((np.pi / 180) * fstart * 1e6)
    prodstack = np.zeros(3, dtype=[("input_a", "<u2"), ("input_b", "<u2")])
    prodstack["input_a"], prodstack["input_b"] = [0, 0, 1], [1, 2, 2]
    feedmap = np.full((3, 3), -1, dtype=np.int64)
    feedmap[0, 1], feedmap[0, 2], feedmap[1, 2] = 2, 0, 1
    baselines = np.array([[bx, 3.0], [0.1, 7.0], [-bx, 0.0]])
    tel = types.SimpleNamespace(feedmap=feedmap, baselines=baselines, freq_start=fstart, latitude=lat)
    task_case(interp, out, "t_mmode", "DPSSFilterMMode", 20261113, 600.0 + np.arange(4.0), ra, "ra", None, prodstack, tel, dict(halfwidths=[m0], centres=[0.0]), (4, 3, 140))  # (the reference needs distinct axis lengths)
    assert np.array_equal(out["t_mmode/cuts"], [m0, m1]), out["t_mmode/cuts"]

    path = os.path.join(GOLDEN, "dpss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
