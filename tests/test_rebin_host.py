"""Host half of the rebinner and the direct interpolators (no GPU): ``util.regrid.rebin_matrix`` / ``grad_1d`` against
arrays the reference produced (tests/golden/rebin.npz, ``tests/gen_golden_rebin.py``), the CSR plan, the container
additions, the tasks' configuration and refusals, and the argument checks of the three new ABI entries."""

import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "rebin.npz")) as z:
        return {k: z[k] for k in z.files}


def test_rebin_matrix_is_the_references(gold):
    import rebin_twin as twin
    from draco_amd.util import regrid

    for name in gold["matrix/names"]:
        tra, ra, wt = gold[f"matrix/{name}/tra"], gold[f"matrix/{name}/ra"], float(gold[f"matrix/{name}/width_t"])
        R = regrid.rebin_matrix(tra, ra, width_t=wt)
        assert R.dtype == np.float64 and np.array_equal(R, gold[f"matrix/{name}/R"]), name
        assert np.array_equal(R, twin.rebin_matrix(tra, ra, wt)), name
        assert (np.count_nonzero(R, axis=0) <= 2).all(), "a sample touches at most two bins"
    R = regrid.rebin_matrix(gold["matrix/m40_nearest/tra"], gold["matrix/m40_nearest/ra"])  # width_t = 0: nearest bin
    assert set(np.unique(R)) <= {0.0, 1.0} and (R.sum(axis=0) <= 1).all()


def test_grad_1d_is_the_references(gold):
    from draco_amd.util import regrid

    x, si, mask = gold["grad/x"], gold["grad/si"], gold["grad/mask"]
    for key, per in (("periodic", 360.0), ("open", None)):
        keep = mask.copy()
        g, mk = regrid.grad_1d(x, si, mask, period=per)
        assert np.array_equal(mask, keep), "the caller's mask is not modified"
        ref, refm = gold[f"grad/{key}/grad"], gold[f"grad/{key}/mask"]
        assert np.array_equal(mk, refm) and mk[6] and mk[7], "two equal adjacent positions are flagged"
        assert not g[mk].any()
        ulp = np.spacing(np.maximum(np.abs(ref.real), np.abs(ref.imag)))
        assert np.all(np.abs(g.real - ref.real) <= 4 * ulp) and np.all(np.abs(g.imag - ref.imag) <= 4 * ulp), key


def test_rebin_plan_is_the_matrix_in_csr_form(gold):
    from draco_amd.util import regrid

    for name in gold["rebin/names"]:
        lsd, nra = gold[f"rebin/{name}/lsd"], int(gold[f"rebin/{name}/samples"])
        target = np.linspace(312, 313, nra, endpoint=False)
        wt = np.median(np.abs(np.diff(lsd)))
        plan = regrid.RebinPlan(None, lsd, target, wt, 312, np.linspace(0, 360, nra, endpoint=False))
        R = regrid.rebin_matrix(lsd, target, wt)
        g, t = np.nonzero(R)  # row-major: by bin, samples ascending
        assert np.array_equal(plan.sample_index, t) and np.array_equal(plan.value, R[g, t])
        assert np.array_equal(plan.row_ptr, np.searchsorted(g, np.arange(nra + 1))) and plan.row_ptr[-1] == len(t)
        assert plan.tile_span.shape == (-(-nra // 64), 2)
        for k, (a, b) in enumerate(plan.tile_span):
            cols = np.flatnonzero(R[64 * k : 64 * k + 64].any(axis=0))
            assert (a, b) == ((cols[0], cols[-1] + 1) if len(cols) else (0, 0))
            for gg in range(64 * k, min(64 * k + 64, nra)):  # a bin's samples are one contiguous span
                s = plan.sample_index[plan.row_ptr[gg] : plan.row_ptr[gg + 1]]
                assert len(s) == 0 or np.array_equal(s, np.arange(s[0], s[-1] + 1))
    lsd = gold["rebin/c37/lsd"].copy()
    lsd[[5, 6]] = lsd[[6, 5]]
    with pytest.raises(NotImplementedError, match="non-decreasing"):
        regrid.RebinPlan(None, lsd, np.linspace(312, 313, 16, endpoint=False), 0.02, 312, np.linspace(0, 360, 16, endpoint=False))


def test_container_additions(tmp_path):
    from draco_amd.core import containers

    ss = containers.SiderealStream(freq=np.array([600.0, 601.0]), ra=8, stack=3)
    for name in ("effective_ra", "nsample"):
        with pytest.raises(KeyError, match=f"Dataset '{name}' not initialised."):
            getattr(ss, name)
    ss.add_dataset("effective_ra")
    ss.add_dataset("nsample")
    assert ss.effective_ra.shape == (2, 3, 8) and ss.effective_ra.dtype == np.float32 and ss.nsample.dtype == np.uint16
    ss.effective_ra[:] = np.arange(48, dtype=np.float32).reshape(2, 3, 8)
    path = str(tmp_path / "s.npz")
    ss.save(path)
    back = containers.SiderealStream.load(path)
    assert np.array_equal(back.effective_ra[:], ss.effective_ra[:]) and back.effective_ra.attrs["axis"] == ["freq", "stack", "ra"]
    del ss["effective_ra"]
    assert "effective_ra" not in ss and "nsample" in ss
    with pytest.raises(KeyError):
        ss.effective_ra
    with pytest.raises(KeyError):
        del ss["effective_ra"]

    hv = containers.HybridVisStream(pol=2, freq=np.array([600.0, 601.0]), ew=3, el=5, ra=8)
    for name in ("effective_ra", "nsample"):
        with pytest.raises(KeyError, match=f"Dataset '{name}' not initialised."):
            getattr(hv, name)
        hv.add_dataset(name, allocate=True)
        assert getattr(hv, name).shape == (2, 2, 3, 8) and getattr(hv, name).dtype == np.float32
    hv.nsample[:] = 1.5
    path = str(tmp_path / "h.npz")
    hv.save(path)
    back = containers.HybridVisStream.load(path)
    assert np.array_equal(back.nsample[:], hv.nsample[:]) and back.effective_ra.attrs["axis"] == ["pol", "freq", "ew", "ra"]
    del hv["nsample"]
    assert "nsample" not in hv


def test_task_configuration_and_refusals():
    from draco_amd.analysis import sidereal
    from draco_amd.core import containers

    for cls in (sidereal.SiderealRegridderNearest, sidereal.SiderealRegridderLinear, sidereal.SiderealRegridderCubic, sidereal.SiderealRebinner):
        assert issubclass(cls, sidereal.SiderealRegridder)
        t = cls(samples=32, down_mix=True)
        assert t.samples == 32 and t.down_mix is True
    assert sidereal.SiderealRebinner().weight == "inverse_variance" and sidereal.SiderealRebinner(weight="uniform").weight == "uniform"
    with pytest.raises(ValueError, match="weight must be 'uniform' or 'inverse_variance'"):
        sidereal.SiderealRebinner(weight="natural")
    x = np.array([0.0, 1.0, 2.0, 4.0])
    assert list(sidereal._search_nearest(x, np.array([-1.0, 0.4, 0.5, 2.9, 3.1, 9.0]))) == [0, 0, 1, 2, 3, 3]

    mm = containers.MModes(mmax=3, freq=np.array([600.0, 601.0]), stack=4)
    mm.attrs["lsd"] = 312
    with pytest.raises(TypeError, match=r"No valid container mapping.\nGot <class 'draco_amd.core.containers.MModes'>.\nMappings exist for \["):
        sidereal.SiderealRebinner(samples=16).process(mm)
    hv = containers.HybridVisStream(pol=2, freq=np.array([600.0, 601.0]), ew=3, el=5, ra=8)
    hv.attrs["lsd"] = 312
    hv.add_dataset("dirty_beam", allocate=True)
    with pytest.raises(NotImplementedError, match="dirty_beam"):
        sidereal.SiderealRebinner(samples=16).process(hv)

    # a stream without effective_ra passes through the correction untouched
    ss = containers.SiderealStream(freq=np.array([600.0, 601.0]), ra=8, stack=3)
    ss.vis[:] = 1.0
    t = sidereal.RebinGradientCorrection()
    t.setup(ss)
    assert t.process(ss) is ss and (ss.vis[:] == 1.0).all() and ss.vis._dev_t is None


FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)

CALLS = {
    "dmm_rebin": (
        [FAKE, 1, 0, BUF, BUF, 6, 1, 37, 16, BUF, BUF, BUF, 40, BUF, BUF, 312.0, BUF, BUF, BUF, BUF, BUF],
        {1: [(2, "bad mode 2"), (-1, "bad mode -1")], 5: [(-1, "bad nrow -1")], 6: [(0, "fold 0 does not divide"), (4, "fold 4 does not divide")], 7: [(0, "bad sizes nt=0")],
         8: [(0, "bad sizes nt=37 nra=0"), (-3, "nra=-3")], 12: [(-1, "nnz=-1")], 3: [(C.c_void_p(0x2004), "16-byte aligned")]},
    ),
    "dmm_rebin_gradient": (
        [FAKE, BUF, BUF, BUF, BUF, BUF, BUF, BUF, None, 6, 48],
        {9: [(-1, "bad nrow -1")], 10: [(0, "bad nra 0"), (-5, "bad nra -5")], 8: [(BUF, "one of the two")]},
    ),
    "dmm_regrid_interp": (
        [FAKE, 2, BUF, BUF, 6, 37, 16, BUF, BUF, BUF, None, None, None, None, BUF, BUF],
        {1: [(3, "bad mode: 3 taps"), (0, "bad mode: 0 taps")], 4: [(-1, "bad nrow -1")], 5: [(0, "bad sizes nt=0")], 6: [(0, "nout=0")], 10: [(BUF, "all four or not at all")]},
    ),
}


def _arg_error(rc, match):
    from draco_amd import _lib

    assert rc == _lib.DMM_E_ARG, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg
    with pytest.raises(ValueError):
        _lib.check(rc)


@pytest.mark.parametrize("name", list(CALLS))
def test_abi_arguments(name):
    from draco_amd import _lib

    assert name in _lib.EXPORTED and (_lib.DMM_REBIN_UNIFORM, _lib.DMM_REBIN_INVERSE_VARIANCE) == (0, 1)
    fn = getattr(_lib.lib, name)
    ok, bad = CALLS[name]

    def call(i, v):
        a = list(ok)
        a[i] = v
        return fn(*a)

    _arg_error(call(0, None), "ctx is NULL")
    for i, cases in bad.items():
        for v, msg in cases:
            _arg_error(call(i, v), msg)
    for i, v in enumerate(ok):
        if i and v is BUF:
            _arg_error(call(i, None), "NULL argument" if not (name == "dmm_rebin_gradient" and i == 7) else "one of the two")
    a = list(ok)
    a[{"dmm_rebin": 5, "dmm_rebin_gradient": 9, "dmm_regrid_interp": 4}[name]] = 0
    assert fn(*a) == 0  # no rows: nothing to do
    if name == "dmm_rebin_gradient":
        rc = call(10, _lib.DMM_MAX_NRA + 1)
        assert rc == _lib.DMM_E_UNSUPPORTED and "fits the LDS" in _lib.lib.dmm_last_error().decode()
