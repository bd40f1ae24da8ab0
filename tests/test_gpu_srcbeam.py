"""Source beamforming on the GPU: the tasks and the function on the cases of ``tests/golden/srcbeam.npz`` against the
long-double truth and the reference's vectors, kernel-edge shapes generated here from a seed against the long-double
twin, the catalogue order and repeated ``process`` calls.

Bounds.  Beam and weight alike: ``e_gpu <= max(32 e_f64, floor)`` against the truth -- ``e_f64`` is the float64 twin's
error, 32 the factor the DPSS tests allow another summation order, ``floor = 8 * 2^-53 * P_max`` the float64 rounding
of a phase of size ``P_max`` -- and ``<= 3 e_ref + floor`` against the reference's vectors.  The beam error is measured
against the size of what was summed, the weight error elementwise (``tests/srcbeam_twin.py``)."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import srcbeam_twin as twin  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(golden_dir):
    from draco_amd.core import containers

    z = dict(np.load(os.path.join(golden_dir, "srcbeam.npz")))
    tel, data, cat, grid = twin.golden_inputs(z)
    g = containers.GridBeam(freq=grid["freq"], pol=grid["pol"], input=np.arange(1), theta=grid["theta"], phi=grid["phi"])
    g.beam[:] = grid["beam"]
    g.weight[:] = grid["weight"]
    return {"z": z, "tel": tel, "cat": cat, "grid": g, "data": {k: twin.to_container(tel, d) for k, d in data.items()}}


def run_case(gold, name, cat=None, **extra):
    from draco_amd.analysis import beamform as bf

    dname, cls, cfg = twin.CASES[name]
    task = getattr(bf, cls)(timetrack=twin.TIMETRACK, **cfg, **extra)
    catalog = twin.to_catalog(gold["cat"] if cat is None else cat, tag="cat_a")
    args = ([gold["grid"]] if "External" in cls else []) + [gold["tel"]]
    if "Cat" in cls:
        task.setup(*args, gold["data"][dname])
        return task, task.process(catalog)
    task.setup(*args, catalog)
    return task, task.process(gold["data"][dname])


def check(label, got_beam, got_weight, truth_beam, truth_weight, norm, pmax, e_f64_beam, e_f64_weight, ref=None):
    fl = twin.floor(pmax)
    eb, ew = twin.beam_error(got_beam, truth_beam, norm), twin.weight_error(got_weight, truth_weight)
    print(f"{label}: beam e_gpu {eb:.2e} (e_f64 {e_f64_beam:.2e}) weight e_gpu {ew:.2e} (e_f64 {e_f64_weight:.2e}) floor {fl:.2e}")
    if ref is not None:
        ref_beam, ref_weight, e_ref_beam, e_ref_weight = ref
        rb, rw = twin.beam_error(got_beam, ref_beam, norm), twin.weight_error(got_weight, ref_weight)
        print(f"{label}: against the reference beam {rb:.2e} (e_ref {e_ref_beam:.2e}) weight {rw:.2e} (e_ref {e_ref_weight:.2e})")
    assert np.array_equal(got_beam == 0, truth_beam == 0), "zero patterns of the beam differ"
    assert eb <= max(32 * e_f64_beam, fl)
    assert ew <= max(32 * e_f64_weight, fl)
    if ref is not None:
        assert rb <= 3 * e_ref_beam + fl
        assert rw <= 3 * e_ref_weight + fl


@pytest.mark.parametrize("name", list(twin.CASES))
def test_task(gold, name):
    z = gold["z"]
    task, fb = run_case(gold, name)
    for ds in (fb.beam, fb.weight):
        assert ds.on_device and ds._dev.is_cuda and ds._dev.dtype == torch.float64
    beam, weight = fb.beam[:], fb.weight[:]
    g = lambda k: z[f"{name}/{k}"]  # noqa: E731
    assert beam.shape == g("ref_beam").shape
    check(name, beam, weight, g("truth_beam"), g("truth_weight"), float(g("norm")), float(g("pmax")), float(g("e_f64_beam")), float(g("e_f64_weight")),
          (g("ref_beam"), g("ref_weight"), float(g("e_ref_beam")), float(g("e_ref_weight"))))
    skipped = g("skipped")
    assert not beam[skipped].any() and not weight[skipped].any()
    if name.startswith("ts"):
        assert skipped.sum() == 3
    if not twin.full_config(twin.CASES[name][2])["collapse_ha"]:
        assert np.array_equal(fb.ha[:], g("ref_ha"))
        assert not fb.ha[:][skipped].any()
    assert fb.attrs["tag"] == ("lsd_4021" if name.startswith("ss") else "ts_a") + "_cat_a"
    assert np.array_equal(fb.position["ra"], gold["cat"]["ra"]) and np.array_equal(fb.position["dec"], gold["cat"]["dec"])
    assert np.array_equal(fb.redshift["z"], gold["cat"]["z"])
    assert list(fb.pol) == (["I"] if twin.CASES[name][2]["polarization"] == "I" else task.process_pol)


def test_zero_weight_window(gold):
    """The source at 200.2 degrees: every weight of its window is zero, so beam and weight are."""
    _, fb = run_case(gold, "ss_natural_full")
    src = int(np.flatnonzero(gold["cat"]["ra"] == 200.2)[0])
    assert not fb.beam[:][src].any() and not fb.weight[:][src].any()
    assert fb.weight[:][src - 1].any()


def test_function(gold):
    from draco_amd.util._fast_tools import beamform

    z = gold["z"]
    args = [z["func/" + k] for k in ("vis", "weight", "dec", "lat", "cosha", "sinha", "u", "v", "f_index", "ra_index")]
    out = beamform(*args)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (args[0].shape[0], len(args[9]))
    got = out.cpu().numpy()
    assert not got[1].any() and not got[3].any()  # frequencies not in f_index
    fl = twin.floor(float(z["func/pmax"]))
    e = twin.beam_error(got, z["func/truth"], float(z["func/norm"]))
    er = twin.beam_error(got, z["func/ref"], float(z["func/norm"]))
    print(f"function: e_gpu {e:.2e} (e_f64 {float(z['func/e_f64']):.2e}) against the reference {er:.2e} (e_ref {float(z['func/e_ref']):.2e}) floor {fl:.2e}")
    assert e <= max(32 * float(z["func/e_f64"]), fl)
    assert er <= 3 * float(z["func/e_ref"]) + fl


# stacks, window slots, sources sharing the window: one lane / under a wave / over a wave / over an LDS pass of stacks;
# one wave's share / every wave's share / many rounds of pairs on one sample
EDGES = [(1, 1, 1), (63, 2, 2), (65, 33, 130), (1030, 2, 130), (1030, 33, 1), (65, 1, 2), (63, 33, 2), (1, 2, 130)]


@pytest.mark.parametrize("ns,nha,nsrc", EDGES)
def test_kernel_edges(ns, nha, nsrc):
    from draco_amd.device import Context
    from draco_amd.util import _fast_tools

    rng = np.random.default_rng(1000 * ns + 10 * nha + nsrc)
    nf, nra = 2, 40
    vis = (rng.normal(size=(nf, nra, ns)) + 1j * rng.normal(size=(nf, nra, ns))).astype(np.complex64)
    w = rng.uniform(0.5, 2.0, size=(nf, nra, ns)).astype(np.float32)
    w[rng.uniform(size=w.shape) < 0.1] = 0.0
    u, v = rng.uniform(-80.0, 80.0, size=(nf, ns)), rng.uniform(-20.0, 20.0, size=(nf, ns))
    lat = np.deg2rad(49.3)
    start = 38  # the shared window wraps past the end of the axis
    ra_index = np.tile((start + np.arange(nha)) % nra, (nsrc, 1))
    dec = np.radians(rng.uniform(10.0, 70.0, size=nsrc))
    ha = np.radians(9.0 * (np.arange(nha) - nha // 2))[np.newaxis, :] + rng.uniform(-0.01, 0.01, size=(nsrc, 1))
    fmask = np.ones((nsrc, nf), dtype=bool)
    fmask[::2, 1] = False  # f_index a strict subset for every other source
    ut, vt = _fast_tools.phase_tables(dec[:, np.newaxis], lat, np.cos(ha), np.sin(ha))
    ctx = Context.get()
    F = _fast_tools.form(ctx, ctx.to_device(vis), ctx.to_device(w), ctx.to_device(u), ctx.to_device(v), ut, vt, ra_index, fmask)
    assert F.is_cuda and F.dtype == torch.float64 and tuple(F.shape) == (nsrc, nf, nha)
    got = F.cpu().numpy()
    truth, f64 = np.zeros(got.shape, dtype=np.longdouble), np.zeros(got.shape)
    pmax = 0.0
    for s in range(nsrc):
        f_index = np.flatnonzero(fmask[s])
        a = (vis, w, dec[s], lat, np.cos(ha[s]), np.sin(ha[s]), u, v, f_index, ra_index[s])
        truth[s], pm = twin.beamform(*a, dtype=np.longdouble, want_pmax=True)
        f64[s] = twin.beamform(*a, dtype=np.float64)
        pmax = max(pmax, pm)
    norm = float(np.sum(w * np.abs(vis), axis=-1)[:, ra_index[0]].max())
    e, e64, fl = twin.beam_error(got, truth, norm), twin.beam_error(f64, truth, norm), twin.floor(pmax)
    print(f"ns {ns} nha {nha} nsrc {nsrc}: e_gpu {e:.2e} e_f64 {e64:.2e} floor {fl:.2e}")
    assert not got[::2, 1].any()
    assert e <= max(32 * e64, fl)


def test_catalogue_order(gold):
    """A sorted catalogue in one chunk, a shuffled one in one chunk (the default workspace) and a shuffled one at one
    source per chunk give bit-identical rows."""
    cat = gold["cat"]
    order = np.argsort(cat["ra"])
    perm = np.random.default_rng(7).permutation(len(order))
    assert not np.array_equal(perm, order)
    pick = lambda idx: {k: v[idx] for k, v in cat.items()}  # noqa: E731
    for name in ("ss_natural_full", "ss_freqside1"):
        _, a = run_case(gold, name, cat=pick(order))
        _, b = run_case(gold, name, cat=pick(perm))
        _, c = run_case(gold, name, cat=pick(perm), workspace_mib=0)  # (one source per chunk)
        inv_a, inv_b = np.argsort(order), np.argsort(perm)
        for ds_a, ds_b, ds_c in ((a.beam, b.beam, c.beam), (a.weight, b.weight, c.weight)):
            assert np.array_equal(ds_a[:][inv_a], ds_b[:][inv_b])
            assert np.array_equal(ds_b[:], ds_c[:])
        assert a.beam[:].any()


@pytest.mark.parametrize("mode", ["inverse_variance", "natural", "uniform"])
def test_prepare_edges(mode):
    """``prepare`` on strict subsets of 65 and 1030 of 1100 stacks (more than one tile of stacks, ragged tails, an odd
    number of samples) against NumPy: the gathered values exactly, the float64 sums to rounding."""
    from draco_amd.device import Context
    from draco_amd.util import _fast_tools

    rng = np.random.default_rng(31)
    nf, nstack, nra = 2, 1100, 37
    vis = (rng.normal(size=(nf, nstack, nra)) + 1j * rng.normal(size=(nf, nstack, nra))).astype(np.complex64)
    w = rng.uniform(0.5, 2.0, size=(nf, nstack, nra)).astype(np.float32)
    w[rng.uniform(size=w.shape) < 0.1] = 0.0
    w[1, :, 5] = 0.0
    red = rng.integers(0, 4, size=(nstack, nra)).astype(np.float32)
    ctx = Context.get()
    vis_d, w_d = ctx.to_device(vis), ctx.to_device(w)
    for nsel in (65, 1030):
        sel = np.sort(rng.choice(nstack, size=nsel, replace=False))
        visT, ws, SW, SW2 = _fast_tools.prepare(ctx, vis_d, w_d, sel, mode, None if mode == "inverse_variance" else red)
        wv = np.moveaxis(w[:, sel, :], 1, 2).astype(np.float64)
        if mode == "inverse_variance":
            want = wv
        else:
            want = (wv > 0) * np.moveaxis(red[sel], 0, 1)[np.newaxis].astype(np.float64)
            if mode == "uniform":
                want = (want > 0).astype(np.float64)
        assert np.array_equal(visT.cpu().numpy(), np.moveaxis(vis[:, sel, :], 1, 2))
        assert ws.dtype == torch.float32 and np.array_equal(ws.cpu().numpy().astype(np.float64), want)
        sw, sw2 = want.sum(axis=-1), (want**2 * twin.inz(wv)).sum(axis=-1)
        assert np.allclose(SW.cpu().numpy(), sw, rtol=1e-13, atol=0) and np.allclose(SW2.cpu().numpy(), sw2, rtol=1e-13, atol=0)
        assert np.array_equal(SW.cpu().numpy() == 0, sw == 0)


def test_empty_catalogue_and_long_variable_window(gold):
    from draco_amd.analysis import beamform as bf

    for collapse in (True, False):
        task = bf.BeamFormCat(timetrack=twin.TIMETRACK, collapse_ha=collapse)
        task.setup(gold["tel"], gold["data"]["ss"])
        fb = task.process(twin.to_catalog({k: v[:0] for k, v in gold["cat"].items()}))
        assert fb.beam.shape == ((0, 4, 4) if collapse else (0, 4, 4, task.nha))
    # 2 int(ha_side) + 1 = 29 fits the 64 samples; at declination 67.3 the secant makes it 77
    task = bf.BeamFormCat(timetrack=20000.0, variable_timetrack=True)
    task.setup(gold["tel"], gold["data"]["ss"])
    assert task.nha == 29
    with pytest.raises(ValueError, match="longer than the RA axis"):
        task.process(twin.to_catalog(gold["cat"]))


def test_process_twice(gold):
    from draco_amd.analysis import beamform as bf

    cat1 = twin.to_catalog(gold["cat"], tag="cat_a")
    cat2 = twin.to_catalog({k: v[::-1][:7] for k, v in gold["cat"].items()}, tag="cat_b")
    task = bf.BeamFormCat(timetrack=twin.TIMETRACK, polarization="I")
    task.setup(gold["tel"], gold["data"]["ss"])
    first, second = task.process(cat1), task.process(cat2)
    assert second.attrs["tag"] == "lsd_4021_cat_b" and second.beam.shape == (7, 1, 4)
    for cat, got in ((cat1, first), (cat2, second)):
        fresh = bf.BeamFormCat(timetrack=twin.TIMETRACK, polarization="I")
        fresh.setup(gold["tel"], gold["data"]["ss"])
        want = fresh.process(cat)
        assert torch.equal(got.beam._dev, want.beam._dev) and torch.equal(got.weight._dev, want.weight._dev)
    task.process_finish()
    assert not hasattr(task, "vis")
