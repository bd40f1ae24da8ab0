"""Source beamforming on the host (no GPU): the float64 twin against the reference's vectors of
``tests/golden/srcbeam.npz``, the three host helpers against the reference's outputs, the containers, and the error
branches of the tasks that are reached before any device call."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import srcbeam_twin as twin  # noqa: E402

from draco_amd.analysis import beamform as bf  # noqa: E402
from draco_amd.core import containers  # noqa: E402
from draco_amd.util import tools  # noqa: E402


@pytest.fixture(scope="module")
def gold(golden_dir):
    z = dict(np.load(os.path.join(golden_dir, "srcbeam.npz")))
    tel, data, cat, grid = twin.golden_inputs(z)
    return {"z": z, "tel": tel, "data": data, "cat": cat, "grid": grid}


def _grid_container(grid):
    g = containers.GridBeam(freq=grid["freq"], pol=grid["pol"], input=np.arange(1), theta=grid["theta"], phi=grid["phi"])
    g.beam[:] = grid["beam"]
    g.weight[:] = grid["weight"]
    return g


@pytest.mark.parametrize("name", list(twin.CASES))
def test_twin_against_reference(gold, name):
    z, tel, cat = gold["z"], gold["tel"], gold["cat"]
    dname, cls, cfg = twin.CASES[name]
    full = twin.full_config(cfg)
    beamfunc = None
    if "External" in cls:  # the spline of the package's own mixin, evaluated per source as the reference does
        t = bf.BeamFormExternalCat(**{k: v for k, v in cfg.items()})
        t.process_pol = ["XX", "YY"]
        t._initialize_grid_beam(_grid_container(gold["grid"]))
        beamfunc = lambda pol, dec, ha: t._grid_beam(pol, np.array([dec]), ha[np.newaxis, :])[0]  # noqa: E731
    got = twin.process(tel, gold["data"][dname], cat, full, z["polmap"], z["bvec_m"], z[dname + "_redundancy"], np.float64, beamfunc)
    fl = twin.floor(float(z[name + "/pmax"]))
    eb = twin.beam_error(got["beam"], z[name + "/ref_beam"], float(z[name + "/norm"]))
    ew = twin.weight_error(got["weight"], z[name + "/ref_weight"])
    print(f"{name}: beam {eb:.2e} (e_ref {float(z[name + '/e_ref_beam']):.2e}) weight {ew:.2e} (e_ref {float(z[name + '/e_ref_weight']):.2e}) floor {fl:.2e}")
    assert eb <= 3 * float(z[name + "/e_ref_beam"]) + fl
    assert ew <= 3 * float(z[name + "/e_ref_weight"]) + fl
    assert np.array_equal(got["skipped"], z[name + "/skipped"])
    if not full["collapse_ha"]:
        assert np.abs(got["ha"] - z[name + "/ref_ha"]).max() < 1e-14


def test_twin_function_against_reference(gold):
    z = gold["z"]
    args = [z["func/" + k] for k in ("vis", "weight", "dec", "lat", "cosha", "sinha", "u", "v", "f_index", "ra_index")]
    got = twin.beamform(*args)
    e = twin.beam_error(got, z["func/ref"], float(z["func/norm"]))
    assert e <= 3 * float(z["func/e_ref"]) + twin.floor(float(z["func/pmax"]))
    assert not got[1].any() and not got[3].any()


def test_host_helpers(gold):
    z, tel = gold["z"], gold["tel"]
    inputs, prod, stack, rev = twin.make_index_maps(tel)
    imap = {"input": inputs, "prod": prod, "stack": stack}
    polmap = tools.polarization_map(imap, tel)
    assert np.array_equal(polmap, z["polmap"])
    assert (polmap == -1).sum() == 2  # the two auto-correlation stacks
    assert np.array_equal(tools.polarization_map(imap, tel, exclude_autos=False) == -1, np.zeros(len(stack), dtype=bool))
    assert np.array_equal(tools.baseline_vector(imap, tel), z["bvec_m"])
    for name in ("ss", "ts"):
        red = tools.calculate_redundancy(z[name + "_input_flags"], prod, rev["stack"], len(stack))
        assert red.dtype == np.float32 and np.array_equal(red, z[name + "_redundancy"])
    zero = tools.calculate_redundancy(np.zeros_like(z["ss_input_flags"]), prod, rev["stack"], len(stack))
    assert np.array_equal(zero, z["redundancy_zero_flags"])
    assert np.array_equal(zero, tools.calculate_redundancy(np.ones_like(z["ss_input_flags"]), prod, rev["stack"], len(stack)))


def test_polarization_map_stack_type(gold):
    tel = twin.FakeTelescope(twin.FREQ)
    tel.stack_type = "unique"
    inputs, prod, stack, _ = twin.make_index_maps(tel)
    with pytest.raises(RuntimeError, match="redundant"):
        tools.polarization_map({"input": inputs, "prod": prod, "stack": stack}, tel)


def test_containers():
    cat = containers.SourceCatalog(object_id=np.arange(5))
    assert cat["position"].dtype.names == ("ra", "dec") and cat["position"].shape == (5,)
    assert "redshift" not in cat and len(cat.index_map["object_id"]) == 5
    sc = containers.SpectroscopicCatalog(object_id=np.arange(5))
    assert "redshift" in sc and sc["redshift"].dtype.names == ("z", "z_error") and "position" in sc
    sc.attrs["tag"] = "x"
    fb = containers.FormedBeam(freq=twin.FREQ, object_id=np.arange(5), pol=np.array(["XX", "YY"]))
    for n in ("beam", "weight"):
        assert fb[n].shape == (5, 2, 4) and fb[n].dtype == np.float64 and fb[n].attrs["axis"] == ["object_id", "pol", "freq"]
    assert "redshift" not in fb
    with pytest.raises(KeyError):
        fb.redshift
    fb.add_dataset("redshift")
    assert fb.redshift.shape == (5,) and list(fb.pol) == ["XX", "YY"] and len(fb.id) == 5 and fb.frequency["centre"][0] == 608.0
    fh = containers.FormedBeamHA(freq=twin.FREQ, object_id=np.arange(5), pol=np.array(["I"]), ha=np.arange(7))
    assert fh.beam.shape == (5, 1, 4, 7) and fh.weight.dtype == np.float64
    assert fh.ha is fh.datasets["object_ha"] and fh.ha.shape == (5, 7) and fh.ha.dtype == np.float64
    g = containers.GridBeam(freq=twin.FREQ, pol=np.array(["XX", "YY"]), input=np.arange(1), theta=np.arange(9.0), phi=np.arange(16.0))
    assert g.beam.shape == (4, 2, 1, 9, 16) and g.beam.dtype == np.complex64 and g.weight.dtype == np.float32
    assert g.attrs["coords"] == "celestial" and g.coords == "celestial"
    assert containers.GridBeam(coords="telescope", freq=twin.FREQ, pol=1, input=1, theta=2, phi=2).coords == "telescope"


def test_task_error_branches(gold):
    tel, data, cat = gold["tel"], gold["data"], gold["cat"]
    with pytest.raises(RuntimeError, match="Stokes"):
        bf.BeamForm(polarization="stokes").setup(tel, None)
    with pytest.raises(NotImplementedError, match="collapse"):
        bf.BeamForm(variable_timetrack=True, collapse_ha=False).setup(tel, None)
    ss = twin.to_container(tel, data["ss"])
    del ss.attrs["lsd"]
    with pytest.raises(ValueError, match="LSD"):
        bf.BeamFormCat().setup(tel, ss)
    ss.attrs["lsd"] = 4021
    with pytest.raises(ValueError, match="longer than the RA axis"):
        bf.BeamFormCat(timetrack=50000.0).setup(tel, ss)
    del ss.datasets["input_flags"]  # the redundancy cannot be counted without them (the reference fails there too)
    for mode in ("natural", "uniform"):
        with pytest.raises(ValueError, match="input_flags"):
            bf.BeamFormCat(weight=mode, timetrack=twin.TIMETRACK).setup(tel, ss)
    with pytest.raises(NotImplementedError, match="ephemeris"):
        bf.icrs_to_cirs(np.zeros(2), np.zeros(2), 0.0)
    t = bf.BeamForm(freqside=1)
    t.setup(tel, None)
    t.epoch = 0.0
    with pytest.raises(NotImplementedError, match="CIRS"):
        t._process_catalog(twin.to_catalog(cat, coordinates="ICRS"))
    with pytest.raises(NotImplementedError, match="CIRS"):
        t._process_catalog(twin.to_catalog(cat, coordinates=None))
    with pytest.raises(ValueError, match="redshift"):
        t._process_catalog(twin.to_catalog({"ra": cat["ra"], "dec": cat["dec"], "z": None}))
    t._process_catalog(twin.to_catalog(cat, tag="cat_a"))
    assert t.nsource == 12 and t.tag_catalog == "cat_a"


def test_grid_beam_error_branches(gold):
    grid = gold["grid"]
    t = bf.BeamFormExternalCat(polarization="copol")
    t.process_pol = ["XX", "YY"]
    g = _grid_container(grid)
    g.attrs["coords"] = "telescope"
    with pytest.raises(RuntimeError, match="celestial"):
        t._initialize_grid_beam(g)
    g2 = containers.GridBeam(freq=grid["freq"], pol=grid["pol"], input=np.arange(2), theta=grid["theta"], phi=grid["phi"])
    with pytest.raises(NotImplementedError, match="input-dependent"):
        t._initialize_grid_beam(g2)
    with pytest.raises(ValueError, match="Do not recognize"):
        t._initialize_beam(containers.SourceCatalog(object_id=1))
    t._initialize_beam(_grid_container(grid))
    t.freq_local = grid["freq"] + 1.0
    with pytest.raises(RuntimeError, match="do not match"):
        t._initialize_beam_with_data()
    t.freq_local = grid["freq"]
    t._initialize_beam_with_data()
