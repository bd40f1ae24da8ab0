"""GPU DAYENU filter of hybrid visibilities and `RADependentWeights` (`csrc/dayenu_hybrid.hip`,
`draco_amd/analysis/dayenu.py`, `draco_amd/analysis/ringmapmaker.py`) against a long-double truth and against vectors
produced by executing the reference (`tests/gen_golden_dayenu_hybrid.py` -> tests/golden/dayenu_hybrid.npz).

Error measure, as in `test_gpu_dayenu.py`: per dataset `e_gpu = max |gpu - truth| / max |truth|` with the truth
(`tests/dayenu_hybrid_twin.py`, long double) rounded to the dataset's dtype; required `e_gpu <= max(2 e_ref, floor)`,
`e_ref` the same measure of the reference's output (stored by the generator), and against the reference's vectors (at
the stored positions) `<= 3 e_ref + floor`.  The floor is `2**-22` for `vis` and `vis_weight` (float32 storage) and
`2**-51` for `filter`, `freq_cov` and the ring map's float64 datasets.  Each test prints `e_gpu` before it asserts.

Measured `e_gpu` / `e_ref` on an MI355X are in DESIGN section 7o.
"""

import os

import numpy as np
import pytest

import dayenu_hybrid_twin as twin
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FLOOR = {"vis": 2.0**-22, "weight": 2.0**-22, "filter": 2.0**-51, "freq_cov": 2.0**-51, "ring": 2.0**-51}
POLS = np.array(["XX", "YY"])


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "dayenu_hybrid.npz")) as z:
        return {k: z[k] for k in z.files}


_truth = {}


def truth_of(gold, name):
    """The truth of a case, computed once and left unchanged."""
    if name not in _truth:
        t = twin.truth_of(twin.case(gold, name))
        for a in t.values():
            if a is not None:
                a.setflags(write=False)
        _truth[name] = t
    return _truth[name]


def stream_of(c):
    from draco_amd.core import containers

    npol, nfreq, new, nel, nra = c["vis"].shape
    s = containers.HybridVisStream(pol=POLS[:npol], freq=c["freq"], ew=new, el=np.linspace(-0.5, 0.5, nel) if nel > 1 else np.zeros(1), ra=nra)
    s.vis[:] = c["vis"]
    s.weight[:] = c["weight"]
    return s


def run(c, **over):
    from draco_amd.analysis.dayenu import DayenuDelayFilterHybridVis

    s = stream_of(c)
    task = DayenuDelayFilterHybridVis(**{**c["cfg"], **over})
    task.setup()
    assert task.process(s) is s and s.vis.on_device and s.weight.on_device
    return s


_ran = {}


def ran(gold, name):
    """Host copies of the datasets of a case after the task, computed once."""
    if name not in _ran:
        s = run(twin.case(gold, name))
        _ran[name] = {"vis": np.array(s.vis[:]), "weight": np.array(s.weight[:])}
        for k in ("filter", "freq_cov"):
            if k in s:
                assert s.datasets[k].on_device
                _ran[name][k] = np.array(s.datasets[k][:])
        for a in _ran[name].values():
            a.setflags(write=False)
    return _ran[name]


def _check(label, ds, got, truth, got_at, ref, e_ref):
    floor = FLOOR[ds]
    e_gpu = twin.rel_err(got, truth)
    e_tri = float(np.abs(got_at - ref).max() / np.abs(ref).max())
    print(f"dayenu hybrid {label} {ds}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} (to the reference {e_tri:.3e})")
    assert np.isfinite(got.view(np.float32 if got.dtype.itemsize == 4 or got.dtype == np.complex64 else np.float64)).all()
    assert e_gpu <= max(2 * e_ref, floor), (label, ds, e_gpu, e_ref)
    assert e_tri <= 3 * e_ref + floor, (label, ds, e_tri, e_ref)


@pytest.mark.parametrize("name", twin.HYBRID_CASES)
def test_task(gold, name):
    g = gold
    c = twin.case(g, name)
    got, t = ran(g, name), truth_of(g, name)
    pos = c["pos"]
    assert got["vis"].dtype == np.complex64 and got["weight"].dtype == np.float32
    if name == "H6":  # the filter is saved and not applied: data and weights bit for bit
        assert np.array_equal(got["vis"].view(np.uint32), c["vis"].view(np.uint32)) and np.array_equal(got["weight"].view(np.uint32), c["weight"].view(np.uint32))
    else:
        sampled = g[f"{name}/ref_vis"].ndim == 4
        _check(name, "vis", got["vis"], t["vis"], twin.at_positions("vis", got["vis"], pos) if sampled else got["vis"], g[f"{name}/ref_vis"], float(g[f"{name}/e_ref_vis"]))
        _check(name, "weight", got["weight"], t["weight"], got["weight"], g[f"{name}/ref_weight"], float(g[f"{name}/e_ref_weight"]))
        assert np.array_equal(got["weight"] == 0, g[f"{name}/ref_weight"] == 0)
    for ds in ("filter", "freq_cov"):
        assert (ds in got) == (t[ds] is not None)
        if ds in got:
            assert got[ds].dtype == np.float64
            _check(name, ds, got[ds], t[ds], twin.at_positions(ds, got[ds], pos), g[f"{name}/ref_{ds}"], float(g[f"{name}/e_ref_{ds}"]))


def test_exact_properties(gold):
    c = twin.case(gold, "H33")
    got = ran(gold, "H33")
    flag = twin.sample_mask(c["weight"])  # [freq, ew, ra]
    skipped = ~flag.any(axis=0)  # [ew, ra]
    assert skipped.sum() == 1
    # skipped samples are untouched, bit for bit, and keep a zero filter and covariance
    v, vin = np.moveaxis(got["vis"], 3, -1), np.moveaxis(c["vis"], 3, -1)  # [pol, freq, ew, ra, el]
    assert np.array_equal(np.ascontiguousarray(v[:, :, skipped]).view(np.uint32), np.ascontiguousarray(vin[:, :, skipped]).view(np.uint32))
    assert np.array_equal(got["weight"][:, :, skipped].view(np.uint32), c["weight"][:, :, skipped].view(np.uint32))
    assert not got["filter"][..., skipped].any() and not got["freq_cov"][..., skipped].any()
    # one filter for all polarisations, zero on flagged rows and columns
    f = got["filter"]
    assert np.array_equal(f[0].view(np.uint64), f[1].view(np.uint64))
    rows = np.broadcast_to(flag[np.newaxis, :, np.newaxis], f.shape)
    cols = np.broadcast_to(flag[np.newaxis, np.newaxis, :], f.shape)
    assert not f[~rows].any() and not f[~cols].any() and f[rows & cols].any()
    single = flag.sum(axis=0) == 1
    assert single.sum() == 1 and np.count_nonzero(f[0][..., single]) == 1
    # the covariance is symmetric bit for bit
    cv = got["freq_cov"]
    assert np.array_equal(cv.view(np.uint64), np.ascontiguousarray(cv.transpose(0, 2, 1, 3, 4)).view(np.uint64))
    assert not cv[~rows].any() and not cv[~cols].any()
    # filtered data of a flagged channel is zero, as the reference's product with a zero row
    assert not v[:, ~flag & ~skipped[np.newaxis]].any()


def test_same_bits_twice_and_in_ragged_batches(gold):
    c = twin.case(gold, "H33")
    first = ran(gold, "H33")
    for over in ({}, {"workspace_mib": 0}):  # (0 MiB: one filter per batch)
        s = run(c, **over)
        for k, name in (("vis", "vis"), ("weight", "vis_weight"), ("filter", "filter"), ("freq_cov", "freq_cov")):
            a = np.array(s.datasets[name][:])
            assert np.array_equal(a.view(np.uint32), first[k].view(np.uint32)), (over, k)
    c = twin.case(gold, "H70")  # the attenuation mask across batches
    s = run(c, workspace_mib=0)
    assert np.array_equal(np.array(s.weight[:]).view(np.uint32), ran(gold, "H70")["weight"].view(np.uint32))
    assert np.array_equal(np.array(s.vis[:]).view(np.uint32), ran(gold, "H70")["vis"].view(np.uint32))


def test_errors(gold):
    from draco_amd.analysis.dayenu import MAX_ORDER, DayenuDelayFilterHybridVis
    from draco_amd.analysis.ringmapmaker import RADependentWeights
    from draco_amd.core import containers

    c = twin.case(gold, "H20")
    with pytest.raises(RuntimeError, match="At least one of"):
        DayenuDelayFilterHybridVis(apply_filter=False, save_filter=False).setup()
    with pytest.raises(NotImplementedError):
        DayenuDelayFilterHybridVis(tauc=[0.0, 0.1], tauw=[0.2, 0.6]).process(stream_of(c))
    with pytest.raises(ValueError, match="lambda_max"):
        DayenuDelayFilterHybridVis(epsilon=1e-17).process(stream_of(c))
    big = containers.HybridVisStream(pol=1, freq=600.0 + 0.01 * np.arange(MAX_ORDER + 1), ew=1, el=1, ra=2)
    big.weight[:] = 1.0
    with pytest.raises(ValueError, match="frequencies, the kernels take"):
        DayenuDelayFilterHybridVis(epsilon=1e-3).process(big)
    s = run(c)
    assert "freq_cov" in s and "filter" not in s
    with pytest.raises(NotImplementedError):
        s.complex_freq_cov
    npol, nfreq, new, nel, nra = c["vis"].shape
    rm = containers.RingMap(beam=1, pol=POLS[:npol], freq=c["freq"], ra=nra, el=np.linspace(-0.5, 0.5, nel))
    rm.weight[:] = 1.0
    with pytest.raises(RuntimeError, match="must save `weight_ew` and `exclude_cyl`"):
        RADependentWeights().process(s, rm)
    rm.attrs["weight_ew"], rm.attrs["exclude_cyl"] = "natural", []
    bad = containers.RingMap(beam=1, pol=POLS[:npol], freq=c["freq"], ra=nra + 1, el=np.linspace(-0.5, 0.5, nel), attrs_from=rm)
    bad.weight[:] = 1.0
    with pytest.raises(ValueError, match="does not match"):
        RADependentWeights().process(s, bad)
    out = RADependentWeights().process(s, rm)
    assert out is rm and "freq_cov" in rm and "filter" not in rm and rm.freq_cov.on_device and rm.weight.on_device
    with pytest.raises(NotImplementedError):
        rm.add_dataset("complex_filter")


# ---- RADependentWeights on H33's output


def ring_of(gold, scheme, excl, nel=5):
    from draco_amd.core import containers

    c = twin.case(gold, "H33")
    npol, nfreq, new, _, nra = c["vis"].shape
    rm = containers.RingMap(beam=1, pol=POLS[:npol], freq=c["freq"], ra=nra, el=np.linspace(-0.5, 0.5, nel))
    rm.weight[:] = gold["R/ring_weight"].astype(np.float64)
    rm.attrs["weight_ew"], rm.attrs["exclude_cyl"] = scheme, list(excl)
    return rm


@pytest.mark.parametrize("name", twin.R_CASES)
def test_ra_dependent_weights(gold, name):
    from draco_amd.analysis.ringmapmaker import RADependentWeights

    g = gold
    scheme, excl = twin.r_case(name)
    t33 = truth_of(g, "H33")
    rw = g["R/ring_weight"].astype(np.float64)
    rpos, fpos = g["R/rpos"], g["R/fpos"]
    hv = run(twin.case(g, "H33"))
    rm = ring_of(g, scheme, excl)
    assert RADependentWeights().process(hv, rm) is rm
    truth = dict(zip(("weight", "filter", "freq_cov"), twin.ra_dependent_weights(t33["weight"], rw, scheme, excl, t33["filter"], t33["freq_cov"], truth=True)))
    assert ("freq_cov" in rm) == (scheme != "inverse_variance") and "filter" in rm
    for ds in ("weight", "filter", "freq_cov"):
        if ds not in rm:
            continue
        assert rm.datasets[ds].on_device and rm.datasets[ds].dtype == np.float64
        got = np.array(rm.datasets[ds][:])
        e_ref = float(g[f"{name}/e_ref_{ds}"])
        e_gpu = twin.rel_err(got, truth[ds].astype(np.float64))
        at = got[:, :, rpos, :] if ds == "weight" else got[..., fpos]
        ref = g[f"{name}/ref_{ds}"]
        e_tri = float(np.abs(at - ref).max() / np.abs(ref).max())
        print(f"RADependentWeights {name} {ds}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} (to the reference {e_tri:.3e})")
        assert np.isfinite(got).all()
        assert e_gpu <= max(2 * e_ref, FLOOR["ring"]), (name, ds, e_gpu, e_ref)
        assert e_tri <= 3 * e_ref + FLOOR["ring"], (name, ds, e_tri, e_ref)
    assert np.array_equal(np.array(rm.weight[:]) == 0, truth["weight"] == 0)


# ---- the kernels, with exactly representable operands


def _exact_operands(rng, npol, n, new, nra, nmat):
    """NF small integers over 64, variances powers of two between 1/4 and 4 (or 0): every product and partial sum of
    the covariance is a multiple of 2**-14 below 2**20, exact in float64."""
    nfi = rng.integers(-3, 4, size=(nmat, n, n)).astype(np.int64)
    e = rng.integers(-2, 3, size=(npol, n, new, nra))
    weight = (2.0**e).astype(np.float32)
    weight[rng.uniform(size=weight.shape) < 0.1] = 0.0
    var4 = np.where(weight == 0, 0, np.rint(4.0 / np.where(weight == 0, 1, weight))).astype(np.int64)
    imat = rng.integers(0, nmat, size=(new, nra)).astype(np.int32)
    return nfi, weight, var4, imat


def _exact_case(rng, npol=2, n=33, new=2, nra=37, nmat=3):
    nfi, weight, var4, imat = _exact_operands(rng, npol, n, new, nra, nmat)
    imat[0, :32] = np.array([0] * 11 + [1] * 10 + [2] * 11)  # a stripe (and a wave) whose lanes hold three filters
    imat[1, :] = 1  # waves and stripes with one filter: the broadcast path
    imat[1, 5], imat[1, 6], imat[1, 36], imat[0, 33] = -1, -2, -2, nmat  # no filter: zero output
    return npol, n, new, nra, nmat, nfi, weight, var4, imat


def test_save_kernel_exact():
    import torch

    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    npol, n, new, nra, nmat, nfi, weight, var4, imat = _exact_case(np.random.default_rng(901))
    nf = nfi / 64.0
    want = np.zeros((npol, n, n, new, nra))
    ok = (imat >= 0) & (imat < nmat)
    want[:, :, :, ok] = np.moveaxis(nf[imat[ok]], 0, -1)[np.newaxis]
    nf_d, imat_d = ctx.to_device(nf), ctx.to_device(imat)
    out = torch.full((npol, n, n, new, nra), float("nan"), dtype=torch.float64, device=nf_d.device)
    _lib.check(_lib.lib.dmm_dayenu_hybrid_save(ctx.handle, npol, n, new, nra, ptr(nf_d), nmat, ptr(imat_d), 0, ptr(out)))
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # skip_negative: the samples without a filter are left as they are
    out = torch.full((npol, n, n, new, nra), 7.0, dtype=torch.float64, device=nf_d.device)
    _lib.check(_lib.lib.dmm_dayenu_hybrid_save(ctx.handle, npol, n, new, nra, ptr(nf_d), nmat, ptr(imat_d), 1, ptr(out)))
    want[:, :, :, ~ok] = 7.0
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("npol,n", [(2, 33), (1, 70)])  # (both orders cross a K-chunk: whole 32-byte runs and the clamped fetch of the last chunk)
def test_cov_kernel_exact(npol, n):
    import torch

    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    npol, n, new, nra, nmat, nfi, weight, var4, imat = _exact_case(np.random.default_rng(902), npol=npol, n=n)
    ok = (imat >= 0) & (imat < nmat)
    want = np.zeros((npol, n, n, new, nra))
    for x in range(new):
        for t in range(nra):
            if ok[x, t]:
                a = nfi[imat[x, t]].astype(np.float64)  # (integers below 2**53: every product and sum is exact in any order)
                for p in range(npol):
                    want[p, :, :, x, t] = ((a * var4[p, :, x, t][np.newaxis, :]) @ a.T) / (64.0 * 64.0 * 4.0)
    nf_d, imat_d, w_d = ctx.to_device(nfi / 64.0), ctx.to_device(imat), ctx.to_device(weight)
    out = torch.full((npol, n, n, new, nra), float("nan"), dtype=torch.float64, device=nf_d.device)
    _lib.check(_lib.lib.dmm_dayenu_hybrid_cov(ctx.handle, npol, n, new, nra, ptr(nf_d), nmat, ptr(imat_d), ptr(w_d), 0, ptr(out)))
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    out = torch.full((npol, n, n, new, nra), 7.0, dtype=torch.float64, device=nf_d.device)
    _lib.check(_lib.lib.dmm_dayenu_hybrid_cov(ctx.handle, npol, n, new, nra, ptr(nf_d), nmat, ptr(imat_d), ptr(w_d), 1, ptr(out)))
    want[:, :, :, ~ok] = 7.0
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want.view(np.uint64))


def test_mask_kernel():
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    rng = np.random.default_rng(903)
    npol, n, new, nra = 2, 7, 3, 300
    w = rng.uniform(0.5, 1.5, size=(npol, n, new, nra)).astype(np.float32)
    w[rng.uniform(size=w.shape) < 0.2] = 0.0
    w[0, 3, 1, 17] = -1.0  # a negative weight is not valid either
    w_d = ctx.to_device(w)
    flag = ctx.empty((n, new, nra), np.uint8)
    _lib.check(_lib.lib.dmm_dayenu_hybrid_mask(ctx.handle, npol, n, new, nra, ptr(w_d), ptr(flag)))
    assert np.array_equal(flag.cpu().numpy().astype(bool), np.all(w > 0, axis=0))
    assert np.array_equal(w_d.cpu().numpy().view(np.uint32), w.view(np.uint32))


@pytest.mark.parametrize("new,kind", [(4, "uniform"), (3, "natural")])
def test_ew_average_kernel(new, kind):
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    rng = np.random.default_rng(904 + new)
    nrow, per, nra = 3 * 5 * 5, 5, 300  # (pol, freq, freq_sum) rows with a coefficient row per (pol, freq)
    x = rng.standard_normal((nrow, new, nra))
    w = np.ones(new) if kind == "uniform" else (new - np.arange(new)).astype(np.float64)
    coef = np.tile(w / w.sum(), (nrow // per, 1))
    coef[1] = coef[1][::-1]  # (a row of its own: the index rows / rows_per_coef)
    out = ctx.empty((nrow, nra), np.float64)
    x_d, c_d = ctx.to_device(x), ctx.to_device(coef)
    _lib.check(_lib.lib.dmm_ew_average(ctx.handle, nrow, per, new, nra, ptr(c_d), ptr(x_d), ptr(out)))
    got = out.cpu().numpy()
    cr = np.repeat(coef, per, axis=0)[:, :, np.newaxis]
    if kind == "uniform":  # products with 1/4 are exact: the sum in ew order, bit for bit
        want = np.zeros((nrow, nra))
        for e in range(new):
            want = want + cr[:, e] * x[:, e]
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    else:  # one rounding for the coefficient, one per product, new - 1 for the sum
        LD = np.longdouble
        wl = w.astype(LD) / w.astype(LD).sum()
        cl = np.tile(wl, (nrow // per, 1))
        cl[1] = cl[1][::-1]
        cl = np.repeat(cl, per, axis=0)[:, :, np.newaxis]
        truth = (cl * x.astype(LD)).sum(axis=1)
        bound = (new + 2) * 2.0**-53 * (np.abs(cl) * np.abs(x)).sum(axis=1)
        err = np.abs(got.astype(LD) - truth)
        print(f"ew average natural new={new}: max err / bound {float((err / bound).max()):.3f}")
        assert np.all(err <= bound)


def test_ew_coef_and_scale_kernels():
    """The RA mean, the three schemes' coefficients and the scaling of the ring map's weights against long double."""
    from draco_amd import _lib
    from draco_amd.device import Context, ptr

    ctx = Context.get()
    rng = np.random.default_rng(905)
    LD = np.longdouble
    npol, nfreq, new, nra, nel = 2, 3, 4, 301, 3
    hw = rng.uniform(0.5, 1.5, size=(npol, nfreq, new, nra)).astype(np.float32)
    hw[rng.uniform(size=hw.shape) < 0.1] = 0.0
    hw[1, 2, 3, :] = 0.0  # an ew without any weight
    rw = rng.uniform(0.5, 1.5, size=(npol, nfreq, nra, nel))
    hw_d = ctx.to_device(hw)
    for scheme, table in ((_lib.DMM_EW_TABLE, np.array([4.0, 0.0, 2.0, 1.0])), (_lib.DMM_EW_INVERSE_VARIANCE, np.array([1.0, 0.0, 1.0, 1.0]))):
        var = twin.inz(hw).astype(LD)
        mean = var.mean(axis=-1, keepdims=True)
        w = (twin.inz(mean) if scheme == _lib.DMM_EW_INVERSE_VARIANCE else 1) * table.astype(LD)[None, None, :, None]
        w = np.broadcast_to(w, mean.shape)
        t_cf = (w * twin.inz(w.sum(axis=-2, keepdims=True)))[..., 0]
        t_cc = (w**2 * twin.inz(w.sum(axis=-2, keepdims=True) ** 2))[..., 0]
        t_rw = rw.astype(LD) * ((w**2 * mean).sum(axis=-2) * twin.inz((w**2 * var).sum(axis=-2)))[..., np.newaxis]
        cf, cc, w2 = (ctx.empty((npol, nfreq, new), np.float64) for _ in range(3))
        num = ctx.empty((npol, nfreq), np.float64)
        rw_d, table_d = ctx.to_device(rw), ctx.to_device(table)
        _lib.check(_lib.lib.dmm_ew_coef(ctx.handle, npol, nfreq, new, nra, scheme, ptr(table_d), ptr(hw_d), ptr(cf), ptr(cc), ptr(w2), ptr(num)))
        _lib.check(_lib.lib.dmm_ew_scale(ctx.handle, npol, nfreq, new, nra, nel, ptr(hw_d), ptr(w2), ptr(num), ptr(rw_d)))
        for label, got, truth in (("coef_filter", cf, t_cf), ("coef_cov", cc, t_cc), ("ring weight", rw_d, t_rw)):
            e = twin.rel_err(got.cpu().numpy(), truth.astype(np.float64))
            print(f"ew scheme {scheme} {label}: e_gpu {e:.3e}")
            # fewer than 64 roundings in sequence, all on non-negative terms: at most 11 in the mean (two terms per thread,
            # eight levels of the tree, the division), doubled by w^2, new - 1 per sum over ew, one per product and inverse
            assert e <= 64 * 2.0**-53, (scheme, label, e)


# ---- the chain


def test_chain_stays_on_device_and_matches_host_copies(gold):
    """H33 -> MModeTransform -> TikhonovRingMapMaker -> RADependentWeights -> Construct / ApplyWienerDelayTransform:
    bit-equal to the same chain fed with host copies of the ring map's datasets."""
    from draco_amd.analysis import powerspec as ps
    from draco_amd.analysis.ringmapmaker import RADependentWeights, TikhonovRingMapMaker
    from draco_amd.analysis.transform import MModeTransform
    from draco_amd.core import containers

    c = twin.case(gold, "H33")
    hv = run(c)
    mt = MModeTransform()
    mt.setup(None)
    hm = mt.process(hv)
    rng = np.random.default_rng(77)
    beam = containers.HybridVisMModes(mmax=hm.mmax, oddra=hm.oddra, pol=POLS, freq=c["freq"], ew=3, el=np.linspace(-0.5, 0.5, 5))
    beam.vis[:] = (1.0 + 0.1 * (rng.standard_normal(beam.vis[:].shape) + 1j * rng.standard_normal(beam.vis[:].shape))).astype(np.complex64)
    beam.weight[:] = 1.0
    maker = TikhonovRingMapMaker(weight_ew="natural", inv_SN=1e-2)
    maker.setup()
    rm = maker.process(hm, beam)
    assert rm.attrs["weight_ew"] == "natural" and list(rm.attrs["exclude_cyl"]) == []
    rm = RADependentWeights().process(hv, rm)
    for name in ("map", "weight", "dirty_beam_power", "filter", "freq_cov"):
        assert rm.datasets[name].on_device, name
    assert np.array_equal(rm.index_map["freq_sum"], rm.index_map["freq"])

    # the same ring map with every dataset on the host
    host = containers.RingMap(axes_from=rm, attrs_from=rm)
    for name in ("dirty_beam_power", "filter", "freq_cov"):
        host.add_dataset(name, allocate=True)
    for name in ("map", "weight", "dirty_beam_power", "filter", "freq_cov"):
        host.datasets[name][:] = np.array(rm.datasets[name][:])
        assert not host.datasets[name].on_device

    outs = []
    for r in (rm, host):
        op = ps.ConstructWienerDelayTransform().process(r)
        dt = ps.ApplyWienerDelayTransform().process(r, op)
        outs.append((np.array(op.filter[:]), np.array(dt.spectrum[:])))
    assert np.isfinite(outs[0][0].view(np.float32)).all() and outs[0][0].any() and outs[0][1].any()
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    assert np.array_equal(outs[0][1].view(np.uint64), outs[1][1].view(np.uint64))
