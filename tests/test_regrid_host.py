"""Host-side checks of the regridding / stacking feature (no GPU): the new entry points are declared, exported and
bound, their argument checks answer before anything touches a device, and the host half (Lanczos matrix, compact
tables, containers, the telescope's time map) does what the reference's does."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

NEW = ("dmm_regrid_plan_create", "dmm_regrid_plan_destroy", "dmm_regrid_band_wiener", "dmm_sidereal_stack_add", "dmm_sidereal_stack_finish")


def test_new_symbols_declared_exported_bound():
    from draco_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "draco_amd.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(rf"\b{n}\s*\(", text), f"{n} is not declared in draco_amd.h"
        assert n in _lib.EXPORTED and hasattr(_lib.lib, n)
    assert _lib.lib.dmm_version() == 100


def test_tasks_importable_with_reference_config():
    from draco_amd.analysis.sidereal import SiderealRegridder, SiderealStacker
    from draco_amd.analysis.transform import LanczosRegridder, Regridder

    assert Regridder is LanczosRegridder and issubclass(SiderealRegridder, LanczosRegridder)
    r = SiderealRegridder()
    assert (r.samples, r.kernel_width, r.epsilon, r.mask_zero_weight, r.down_mix, r.start, r.end) == (1024, 5, 1e-3, False, False, None, None)
    s = SiderealStacker()
    assert (s.tag, s.weight, s.with_sample_variance) == ("stack", "inverse_variance", False)
    with pytest.raises(ValueError):
        SiderealStacker(weight="median")


def test_argument_errors():
    from draco_amd import _lib

    lib = _lib.lib
    h = C.c_void_p(1)  # a non-NULL ctx is not dereferenced before the argument checks
    out = C.c_void_p()
    with pytest.raises(ValueError, match="ctx is NULL"):
        _lib.check(lib.dmm_regrid_plan_create(None, 4, 4, 5, None, None, None, C.byref(out)))
    with pytest.raises(ValueError, match="NULL argument"):
        _lib.check(lib.dmm_regrid_plan_create(h, 4, 4, 5, None, None, None, C.byref(out)))
    a = np.zeros(4, np.int32)
    v = np.zeros(4)
    p = lambda x: C.c_void_p(x.ctypes.data)  # noqa: E731
    with pytest.raises(ValueError, match="kernel_width 9 outside 1 ... 6"):
        _lib.check(lib.dmm_regrid_plan_create(h, 4, 4, 9, p(a), p(a), p(v), C.byref(out)))
    bad = np.array([0, 0, 0, 7], np.int32)
    with pytest.raises(ValueError, match="span of grid point 3"):
        _lib.check(lib.dmm_regrid_plan_create(h, 4, 4, 5, p(a), p(bad), p(v), C.byref(out)))
    with pytest.raises(ValueError, match="plan is NULL"):
        _lib.check(lib.dmm_regrid_band_wiener(h, None, None, None, 1, 1e-3, 0, 1, 0, None, None, None, None, None, None))
    with pytest.raises(ValueError, match="ctx is NULL"):
        _lib.check(lib.dmm_sidereal_stack_add(None, 0, 0, None, None, None, None, None, None, None, None, 1))
    with pytest.raises(ValueError, match="NULL argument"):
        _lib.check(lib.dmm_sidereal_stack_add(h, 0, 0, None, None, None, None, None, None, None, None, 1))
    with pytest.raises(ValueError, match="bad mode 5"):
        _lib.check(lib.dmm_sidereal_stack_add(h, 5, 0, None, None, None, None, None, None, None, None, 1))
    with pytest.raises(ValueError, match="NULL argument"):
        _lib.check(lib.dmm_sidereal_stack_finish(h, 1, 0, None, None, None, None, 1))
    assert lib.dmm_sidereal_stack_add(h, 0, 0, None, None, None, None, None, None, None, None, 0) == 0
    assert lib.dmm_regrid_plan_destroy(None) == 0


def test_compact_rows_match_the_reference_spans():
    """`compact_rows` finds the spans `band_wiener` finds (regrid.py:64-66) and loses no non-zero of R."""
    import regrid_twin as twin
    from draco_amd.util import regrid

    rng = np.random.default_rng(5)
    times = np.sort(rng.uniform(-0.05, 1.05, 150))
    times = times[(times < 0.3) | (times > 0.45)]
    grid, pad = twin.padded_grid(64, 0.0, 1.0, 3)
    R = regrid.lanczos_forward_matrix(grid, times, 3).T.copy()
    assert np.array_equal(R, twin.forward_matrix(grid, times, 3))
    start, end, vals = regrid.compact_rows(R)
    s_ref = (R != 0).argmax(axis=-1)
    e_ref = np.where((R == 0).all(axis=-1), 0, R.shape[-1] - (R[..., ::-1] != 0).argmax(axis=-1))
    assert np.array_equal(end, e_ref) and np.array_equal(start[e_ref > 0], s_ref[e_ref > 0])
    assert (end == start).any(), "the gap leaves grid points without samples"
    back = np.zeros_like(R)
    o = 0
    for g in range(len(grid)):
        back[g, start[g] : end[g]] = vals[o : o + end[g] - start[g]]
        o += end[g] - start[g]
    assert np.array_equal(back, R)


def test_containers_and_time_map():
    from draco_amd.core import containers
    from draco_amd.core.products import TransitTelescope

    ts = containers.TimeStream(freq=np.array([600.0, 601.0]), time=1.6e9 + np.arange(7.0), stack=3)
    assert ts.vis.shape == (2, 3, 7) and ts.vis.dtype == np.complex64 and ts.weight.dtype == np.float32
    assert ts.vis.attrs["axis"][-1] == "time" and ts.time.dtype == np.float64
    ss = containers.SiderealStream(freq=np.array([600.0, 601.0]), ra=8, stack=3)
    ss.add_dataset("nsample")
    ss.add_dataset("sample_variance")
    assert ss.nsample.shape == (2, 3, 8) and ss.nsample.dtype == np.uint16
    assert ss.sample_variance.shape == (3, 2, 3, 8) and ss.sample_variance.dtype == np.float32
    tel = TransitTelescope(np.array([600.0]), lmax=4, ncyl=1, nfeed_cyl=2, longitude=-119.6, lsd_start=1.5e9)
    t = 1.5e9 + np.array([0.0, 86164.0905, 1000.0])
    lsd = tel.unix_to_lsd(t)
    assert np.allclose(lsd[1] - lsd[0], 1.0, rtol=0, atol=1e-10) and np.allclose(tel.lsd_to_unix(lsd), t, rtol=0, atol=1e-4)
    assert np.isclose(lsd[0], -119.6 / 360.0)


def test_fixtures_present_and_small():
    for n in ("regrid.npz", "sidereal_stack.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, n)) < 320 * 1024
    with np.load(os.path.join(GOLDEN, "regrid.npz")) as z:
        assert set(z["regrid/names"]) >= {"over_kw5", "under_kw5", "over_kw3", "under_kw3", "inside_kw5"}
        for n in z["regrid/names"]:
            assert 0 < float(z[f"regrid/{n}/e_ref"]) < 1e-3
