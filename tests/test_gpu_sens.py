"""``ComputeSystemSensitivity`` and ``NegativeAutosMask`` on the GPU against the float64 twin (``tests/sens_twin.py``) and
the reference-executed vectors of ``tests/golden/sens.npz``.

Bounds.  ``weight`` is a sum of integers below 2^24: exact, bit-equal to the twin.  ``measured`` and ``radiometer`` are
accumulated in float64 as the twin's are and rounded to float32 once; the two differ by the order of the float64 sums
and by that rounding, one to three float32 roundings in all: 2^-22 relative.  Zeros and NaN fall on the same samples.
Against the reference vectors the reference's own float32 error, ``(n + 6) 2^-24`` (``test_sens_host.py``), is added.
"""

import numpy as np
import pytest

import sens_twin as twin
from test_sens_host import CASES, EPS, arrays, gold, relative, stream, task_for, telescope  # noqa: F401  (gold: fixture)

from draco_amd.analysis.sensitivity import ComputeSystemSensitivity
from draco_amd.core import containers
from draco_amd.core.products import TransitTelescope

pytestmark = pytest.mark.gpu

TWIN_BOUND = 2.0**-22
KEYS = ("measured", "radiometer", "weight", "frac_lost")


def device_arrays(out):
    """The four datasets as NumPy arrays, taken from the device tensors; none may have a host copy."""
    got = {}
    for k in KEYS:
        ds = out.datasets[k]
        assert ds.on_device and ds._host is None, f"{k} is not device resident"
        got[k] = ds._dev.cpu().numpy()
    return got


def against_twin(got, tw):
    meas, radm, wgt, lost = tw
    assert got["weight"].dtype == np.float32 and np.array_equal(got["weight"], wgt)
    assert np.array_equal(got["frac_lost"], np.broadcast_to(lost, got["frac_lost"].shape))
    for key, t in (("measured", meas), ("radiometer", radm)):
        g = got[key]
        assert g.dtype == np.float32 and g.shape == t.shape
        assert np.array_equal(np.isnan(g), np.isnan(t)), f"{key}: NaN on other samples"
        assert np.array_equal(g == 0, t == 0), f"{key}: zeros on other samples"
        err = relative(g, t)[~np.isnan(t)]
        worst = err.max() if err.size else 0.0
        print(f"{key}: {worst:.3e} against {TWIN_BOUND:.3e}")
        assert worst <= TWIN_BOUND


@pytest.mark.parametrize("name", CASES)
def test_process(gold, name):  # noqa: F811
    case = arrays(gold, name)
    task = task_for(gold, name)
    ts = stream(case)
    out = task.process(ts)
    assert isinstance(out, containers.SystemSensitivity)
    assert list(out.pol) == list(gold[f"{name}/pol"])
    assert np.array_equal(out.time, case["time"]) and np.array_equal(out.index_map["freq"], case["freq"]) and out.attrs["tag"] == "sens"
    got = device_arrays(out)
    terms = {}
    tw = twin.sensitivity(case["vis"], case["weight"], task.tables(ts), case.get("frac_lost"), terms=terms)
    against_twin(got, tw)
    # the reference vectors: its float32 error on top
    bound = (int(gold[f"{name}/n"]) + 6) * EPS + TWIN_BOUND
    assert np.array_equal(got["weight"], gold[f"{name}/ref/weight"])
    assert np.array_equal(got["frac_lost"], gold[f"{name}/ref/frac_lost"])
    for key in ("measured", "radiometer"):
        ref = gold[f"{name}/ref/{key}"]
        assert np.array_equal(np.isnan(got[key]), np.isnan(ref))
        sel = ~np.isnan(ref)
        if key == "radiometer" and name == "d":
            sel &= terms["cancel"] > 1e-3
        err = relative(got[key], ref)[sel].max()
        print(f"{name} {key} against the reference: {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    if name == "d":
        assert np.isnan(got["radiometer"]).sum() == 1


def test_already_stacked_raises(gold):  # noqa: F811
    with pytest.raises(ValueError, match="already been stacked"):
        task_for(gold, "e").process(stream(arrays(gold, "e")))


def random_stream(seed, tel, stacked, nfreq, ntime, gain=False):
    """A stream of free-form numbers on a telescope's products: about 10 % zero weights, a row and a time without
    weight, a row of negative weights, positive autocorrelations, three distinct columns of input flags."""
    rng = np.random.default_rng(seed)
    prod = tel.index_map_prod
    kw = dict(stack=tel.index_map_stack, reverse_map_stack=tel.reverse_map_stack) if stacked else {}
    freq = np.zeros(nfreq, dtype=[("centre", np.float64), ("width", np.float64)])
    freq["centre"], freq["width"] = 600.0 - 0.390625 * np.arange(nfreq), 0.390625
    ts = containers.TimeStream(freq=freq, time=1.6e9 + 9.5 * np.arange(ntime), input=tel.input_index, prod=prod, **kw)
    nstack = ts.vis.shape[1]
    vis = (rng.normal(size=(nfreq, nstack, ntime)) + 1j * rng.normal(size=(nfreq, nstack, ntime))).astype(np.complex64)
    ps = ts.prodstack
    autos = np.flatnonzero(ps["input_a"] == ps["input_b"])
    vis[:, autos] = rng.uniform(50.0, 150.0, (nfreq, len(autos), ntime)).astype(np.complex64)
    w = rng.uniform(0.5, 2.0, (nfreq, nstack, ntime)).astype(np.float32)
    w[rng.uniform(size=w.shape) < 0.1] = 0.0
    w[:, nstack // 2] = 0.0
    if ntime > 2:
        w[:, :, ntime // 2] = 0.0
    w[:, nstack // 3] = -np.abs(w[:, nstack // 3])
    ts.vis[:], ts.weight[:] = vis, w
    ts.add_dataset("input_flags")
    flags = np.ones((tel.nfeed, ntime), dtype=np.float32)
    flags[1, : ntime // 3] = 0.0
    flags[tel.nfeed - 2, ntime // 2 :] = 0.0
    ts.input_flags[:] = flags
    if gain:
        ts.add_dataset("gain")
        g = (rng.normal(size=(nfreq, tel.nfeed, ntime)) + 1j).astype(np.complex64)
        g[rng.uniform(size=g.shape) < 0.05] = 1.0
        ts.gain[:] = g
        ts.add_dataset("flags/frac_lost")
        ts["flags"]["frac_lost"][:] = rng.uniform(0.0, 0.3, (nfreq, ntime)).astype(np.float32)
    return ts


def run_against_twin(ts, tel, **cfg):
    task = ComputeSystemSensitivity(**cfg)
    task.setup(tel)
    out = task.process(ts)
    got = device_arrays(out)
    lost = ts["flags"]["frac_lost"][:] if "flags" in ts else None
    against_twin(got, twin.sensitivity(ts.vis[:], ts.weight[:], task.tables(ts), lost))
    return task, got


@pytest.mark.parametrize("layout", ["stacked_2x12", "unstacked_1x40"])
def test_stack_split(layout):
    """Row lists longer than one pass of a block (4 waves, 8 rows in flight each): every wave of the stack split, the
    unrolled loop, its tail and the combine in LDS all take part; 130 times are two full tiles and a tail of two.  The
    stacked 2 x 12 telescope has 35 to 69 rows per product; the unstacked single cylinder of 40 feeds 820 to 1600, and
    its two groups of 40 autocorrelations take the radiometer kernel through its unrolled loop as well."""
    if layout == "stacked_2x12":
        tel, stacked = TransitTelescope(np.array([600.0, 601.0]), lmax=4, ncyl=2, nfeed_cyl=12), True
    else:
        tel, stacked = TransitTelescope(np.array([600.0, 601.0]), lmax=4, ncyl=1, nfeed_cyl=40), False
    ts = random_stream(7, tel, stacked, nfreq=2, ntime=130, gain=not stacked)
    task, first = run_against_twin(ts, tel)
    tb = task.tables(ts)
    assert np.diff(tb["pol_ptr"]).min() > 32 and (stacked or np.diff(tb["grp_ptr"]).min() > 32)
    second = device_arrays(task.process(ts))
    for k in KEYS:
        assert first[k].tobytes() == second[k].tobytes(), f"{k}: two runs differ"


@pytest.mark.parametrize("shape", ["one_time", "one_freq", "no_rows"])
def test_degenerate_shapes(shape):
    if shape == "no_rows":
        # one cylinder, unstacked, intracylinder baselines excluded: every row list and every pair list is empty
        tel = TransitTelescope(np.array([600.0, 601.0]), lmax=4, ncyl=1, nfeed_cyl=3)
        _, got = run_against_twin(random_stream(11, tel, False, nfreq=2, ntime=70), tel, exclude_intracyl=True)
        assert not got["measured"].any() and not got["radiometer"].any() and not got["weight"].any()
        return
    tel = TransitTelescope(np.array([600.0, 601.0]), lmax=4, ncyl=2, nfeed_cyl=3)
    nfreq, ntime = (2, 1) if shape == "one_time" else (1, 70)
    _, got = run_against_twin(random_stream(12, tel, True, nfreq=nfreq, ntime=ntime), tel)
    assert got["measured"].shape == (nfreq, 3, ntime) and got["measured"].any()
    if shape == "one_time":  # no integration time can be read off one sample: NaN, as the reference's median of nothing
        assert np.isnan(got["radiometer"]).all()


def test_chain_into_rfi_mask(gold):  # noqa: F811
    """The device-resident output goes straight into ``RFISensitivityMask``; the mask equals the one from a copy of the
    container whose datasets went through the host."""
    from draco_amd.analysis.flagging import RFISensitivityMask

    out = task_for(gold, "a").process(stream(arrays(gold, "a")))
    cfg = dict(mask_type="combine", niter=2, base_size=(3, 7), mad_size=(3, 9), win_f_1d=3, max_m=8)
    direct = RFISensitivityMask(**cfg).process(out)
    for k in KEYS[:3]:
        assert out.datasets[k].on_device and out.datasets[k]._host is None, f"{k} came to the host on the way"
    copy = containers.SystemSensitivity(pol=out.pol, axes_from=out, attrs_from=out)
    for k in KEYS:
        copy.datasets[k][:] = out.datasets[k]._dev.cpu().numpy()
        assert not copy.datasets[k].on_device
    via_host = RFISensitivityMask(**cfg).process(copy)
    assert direct.mask[:].dtype == bool and np.array_equal(direct.mask[:], via_host.mask[:])
    assert direct.mask[:, 41].all()  # the time without weight


def test_negative_autos(gold):  # noqa: F811
    from draco_amd.analysis.flagging import NegativeAutosMask

    out = NegativeAutosMask().process(stream(arrays(gold, "d")))
    assert isinstance(out, containers.RFIMask) and out.mask.on_device and out.mask._host is None
    assert out.mask.dtype == np.bool_ and out.attrs["tag"] == "sens"
    assert np.array_equal(out.mask[:], gold["negauto/d/mask"]) and gold["negauto/d/mask"].sum() >= 2
    none = NegativeAutosMask().process(stream(arrays(gold, "c")))
    assert none.mask[:].shape == (3, 70) and not none.mask[:].any()
    # a list long enough for every wave of the block, and a time tail
    tel = TransitTelescope(np.array([600.0, 601.0]), lmax=4, ncyl=1, nfeed_cyl=40)
    ts = random_stream(13, tel, False, nfreq=2, ntime=130)
    vis = ts.vis[:].copy()
    ps = ts.prodstack
    autos = np.flatnonzero(ps["input_a"] == ps["input_b"])
    want = np.zeros((2, 130), dtype=bool)
    for k, (f, a, t) in enumerate([(0, 0, 0), (1, 79, 129), (0, 41, 64), (1, 6, 63), (0, 3, 128)]):
        vis[f, autos[a], t] = -1.0 - k
        want[f, t] = True
    vis[:, autos[0] + 1, 5] = -3.0  # a negative cross-correlation is no concern
    ts.vis[:] = vis
    assert np.array_equal(NegativeAutosMask().process(ts).mask[:], want)
