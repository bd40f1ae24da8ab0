"""Host side of ``ComputeSystemSensitivity``: the float64 twin (``tests/sens_twin.py``) against the reference-executed
vectors of ``tests/golden/sens.npz`` (``tests/gen_golden_sens.py``), the two helpers ported from ``draco.util.tools``, the
optional ``TimeStream`` datasets and the search for distinct flag columns.  No GPU.

Bounds: ``weight`` is exact (integer terms below 2^24); ``measured`` and ``radiometer`` of the reference, float32 sums of
``n`` terms, lie within ``(n + 6) 2^-24`` relative of the float64 twin, ``n`` recorded per case.  In the case with negative
autocorrelations the bound is applied where ``|R|`` exceeds 1e-3 of the sum of the absolute values of R's terms, at most
1 % of the samples are left out, and NaN falls on the same samples.

Case (e) of the file is the co-polar part of the stacked stream: the reference's test for "already stacked over
cylinders" is "as many autocorrelation entries as polarisation products", which the full stack axis of this telescope (two
autocorrelation entries, three products) does not meet; that stream is case (f), where the reference returns a
radiometer estimate of zero."""

import os

import numpy as np
import pytest

import sens_twin as twin
from draco_amd.analysis.sensitivity import ComputeSystemSensitivity
from draco_amd.core import containers
from draco_amd.core.products import TransitTelescope
from draco_amd.util import tools

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sens.npz")
EPS = 2.0**-24
CASES = ("a", "b", "c", "d", "f")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def telescope(gold, name, **kw):
    """The telescope of a case: the stacked ones have one input masked in ``feedmask``."""
    tel = TransitTelescope(np.linspace(600.0, 601.0, 3), lmax=4, **dict(dict(ncyl=2, nfeed_cyl=3, npol_feed=2), **kw))
    if name in ("a", "b", "e", "f"):
        m = int(gold["masked_input"])
        tel.feedmask = tel.feedmask.copy()
        tel.feedmask[m, :] = tel.feedmask[:, m] = False
    return tel


def arrays(gold, name):
    """The arrays of a case by their short names; (f) is the stream of (a), (e) its co-polar stack entries."""
    src = "a" if name in ("e", "f") else name
    case = {k.split("/", 1)[1]: v for k, v in gold.items() if k.startswith(src + "/") and k.count("/") == 1}
    if name == "e":
        sel = gold["e/sel"]
        case.update(stack=case["stack"][sel], vis=case["vis"][:, sel], weight=case["weight"][:, sel], reverse_stack=gold["e/reverse_stack"])
    return case


def stream(case):
    ts = containers.TimeStream(freq=case["freq"], time=case["time"], input=case["input"], prod=case["prod"], stack=case["stack"], reverse_map_stack=case["reverse_stack"])
    ts.vis[:], ts.weight[:] = case["vis"], case["weight"]
    ts.attrs["tag"] = "sens"
    ts.add_dataset("input_flags")
    ts.input_flags[:] = case["input_flags"]
    if "gain" in case:
        ts.add_dataset("gain")
        ts.gain[:] = case["gain"]
        ts.add_dataset("flags/frac_lost")
        ts["flags"]["frac_lost"][:] = case["frac_lost"]
    return ts


def task_for(gold, name):
    intracyl = name in ("c", "e", "f")
    task = ComputeSystemSensitivity(exclude_intracyl=intracyl)
    task.setup(telescope(gold, name))
    return task


def twin_of(gold, name, terms=None):
    case = arrays(gold, name)
    tb = task_for(gold, name).tables(stream(case))
    return tb, twin.sensitivity(case["vis"], case["weight"], tb, case.get("frac_lost"), terms=terms)


def relative(got, want):
    """|got - want| / |want| where ``want`` is a number other than zero; |got| where it is zero."""
    got, want = got.astype(np.float64), want.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want))


@pytest.mark.parametrize("name", CASES)
def test_twin_against_reference(gold, name):
    terms = {}
    tb, (meas, radm, wgt, lost) = twin_of(gold, name, terms)
    assert list(tb["pol"]) == list(gold[f"{name}/pol"])
    assert terms["n"] == int(gold[f"{name}/n"])
    bound = (terms["n"] + 6) * EPS
    ref = {k: gold[f"{name}/ref/{k}"] for k in ("measured", "radiometer", "weight", "frac_lost")}
    assert np.array_equal(wgt, ref["weight"])
    assert np.array_equal(np.broadcast_to(lost, ref["frac_lost"].shape), ref["frac_lost"])
    for key, t in (("measured", meas), ("radiometer", radm)):
        assert np.array_equal(t, gold[f"{name}/twin/{key}"], equal_nan=True)
        assert np.array_equal(np.isnan(t), np.isnan(ref[key]))
        sel = ~np.isnan(t)
        if key == "radiometer" and name == "d":
            sel &= terms["cancel"] > 1e-3
            assert 1.0 - sel.mean() <= 0.01
        err = relative(ref[key], t)[sel].max()
        print(f"{name} {key}: {err:.3e} against {bound:.3e}")
        assert err <= bound
    if name == "d":
        assert np.isnan(radm).sum() >= 1 and np.isnan(radm[1, list(tb["pol"]).index("XY"), 33])
    if name == "f":
        assert not radm.any() and meas.any()  # no pair of autocorrelations is left; the measured estimate is there


def test_already_stacked_raises(gold):
    assert bool(gold["e/raised"])
    with pytest.raises(ValueError, match="already been stacked"):
        task_for(gold, "e").tables(stream(arrays(gold, "e")))


def test_needs_a_time_axis():
    ss = containers.SiderealStream(freq=np.array([600.0, 601.0]), ra=8, stack=3)
    with pytest.raises(TypeError, match="time"):
        ComputeSystemSensitivity().process(ss)


def test_warns_about_masked_baselines(gold, caplog):
    with caplog.at_level("WARNING"):
        task_for(gold, "a").tables(stream(arrays(gold, "a")))
    assert "There are 2 stacked baselines that are masked in the telescope instance." in caplog.text


@pytest.mark.parametrize("name", ("a", "c"))
def test_tools_against_reference(gold, name):
    case, tel = arrays(gold, name), telescope(gold, name)
    new, flag = tools.redefine_stack_index_map(tel, case["input"], case["prod"], case["stack"], case["reverse_stack"])
    assert new.dtype == case["stack"].dtype and np.array_equal(new, gold[f"redefine/{name}/stack"])
    assert flag.dtype == bool and np.array_equal(flag, gold[f"redefine/{name}/flag"])
    found = tools.find_inputs(tel.input_index, case["input"], require_match=False)
    assert isinstance(found, list) and [-1 if i is None else i for i in found] == list(gold[f"find_inputs/{name}"])
    if name == "a":
        assert found[int(gold["missing_input"])] is None and (new["prod"] != case["stack"]["prod"]).any() and not flag.all()
        with pytest.raises(ValueError, match="Could not find all of the keys"):
            tools.find_inputs(tel.input_index, case["input"], require_match=True)


def test_find_inputs_errors(gold):
    inputs = arrays(gold, "a")["input"]
    with pytest.raises(ValueError) as e:
        tools.find_inputs(np.zeros(3, dtype=[("other", "<u2")]), inputs)
    assert str(e.value) == str(gold["find_inputs/error"]) != ""
    with pytest.raises(ValueError, match="does not have a `correlator_input` field"):
        tools.find_inputs(inputs, np.zeros(3, dtype=[("chan_id", "<u2")]))
    from draco_amd.analysis import transform

    assert transform._find_inputs is tools.find_inputs


def test_cylinder_width():
    tel = TransitTelescope(np.array([600.0]), lmax=4, ncyl=2, nfeed_cyl=3)
    assert tel.cylinder_width == tel.cyl_sep == tel.cylinder_spacing


def test_timestream_optional_fields(gold, tmp_path):
    case = arrays(gold, "b")
    bare = containers.TimeStream(freq=case["freq"], time=case["time"], input=case["input"], prod=case["prod"], stack=case["stack"], reverse_map_stack=case["reverse_stack"])
    assert sorted(bare.datasets) == ["vis", "vis_weight"]
    assert "flags" not in bare and "gain" not in bare and "input_flags" not in bare
    with pytest.raises(KeyError):
        bare.input_flags
    assert "flags/frac_lost" not in containers.TimeStream._dataset_spec  # adding to one container does not leak
    ts = stream(case)
    assert "flags" in ts and "frac_lost" in ts["flags"] and "other" not in ts["flags"] and "gain" in ts
    assert ts.input_flags.shape == (12, 70) and ts.input_flags.dtype == np.float32
    assert ts.gain.shape == (3, 12, 70) and ts.gain.dtype == np.complex64
    assert ts["flags"]["frac_lost"].shape == (3, 70) and ts["flags"]["frac_lost"].dtype == np.float32
    assert list(ts.gain.attrs["axis"]) == ["freq", "input", "time"]
    path = str(tmp_path / "ts.npz")
    ts.save(path)
    back = containers.TimeStream.load(path)
    assert "flags" in back and sorted(back.datasets) == sorted(ts.datasets)
    for k in ts.datasets:
        assert np.array_equal(back.datasets[k][:], ts.datasets[k][:]) and back.datasets[k].dtype == ts.datasets[k].dtype
    assert list(back["flags"]["frac_lost"].attrs["axis"]) == ["freq", "time"]
    assert np.array_equal(back["flags"]["frac_lost"][:], case["frac_lost"])
    assert "flags/frac_lost" not in containers.TimeStream._dataset_spec


def test_unique_columns():
    rng = np.random.default_rng(5)
    base = rng.uniform(size=(12, 9)) < 0.5
    base[:, 3] = False  # an all-bad and an all-good column among them
    base[:, 4] = True
    flags = base[:, rng.integers(0, 9, 210)]
    cols, inverse = tools.unique_columns(flags)
    want, want_inverse = np.unique(flags, return_inverse=True, axis=1)
    assert cols.dtype == bool and cols.shape == want.shape and inverse.shape == (210,)
    assert np.array_equal(cols[:, inverse], flags)
    # the same set of columns, in whatever order
    assert sorted(map(tuple, cols.T)) == sorted(map(tuple, want.T))
    assert np.array_equal(want[:, np.asarray(want_inverse).reshape(-1)], cols[:, inverse])
    one, inv = tools.unique_columns(np.ones((12, 5), dtype=bool))
    assert one.shape == (12, 1) and not inv.any()


def test_tables_follow_the_gain(gold):
    tb_a = task_for(gold, "a").tables(stream(arrays(gold, "a")))
    tb_b = task_for(gold, "b").tables(stream(arrays(gold, "b")))
    assert tb_a["niff"] == 1 and tb_a["col"].shape == (1, 70) and tb_a["cnt"].shape[1] == 4  # four distinct flag columns
    assert tb_b["niff"] == 3 and tb_b["col"].shape == (3, 70) and tb_b["cnt"].shape[1] > 4
    case = arrays(gold, "b")
    good = (case["input_flags"].astype(bool)[None] & (case["gain"] != 1.0 + 0.0j))  # [freq, input, time]
    want = tools.calculate_redundancy(good[1].astype(np.float32), case["prod"], case["reverse_stack"]["stack"], len(case["stack"]))
    assert np.array_equal(tb_b["cnt"][:, tb_b["col"][1]], want)
    tb_c = task_for(gold, "c").tables(stream(arrays(gold, "c")))
    assert len(tb_c["auto_rows"]) == 12 and len(tb_c["grp_ptr"]) == 5
