"""Argument validation of the four producers of the ring-map chain (``dmm_calc_redundancy``, ``dmm_vis_grid``,
``dmm_beamform_ns``, ``dmm_beamform_ew``), on the CPU, in the style of ``test_abi_srcbeam.py``: a made-up non-NULL handle
is enough to drive the host-side checks.  Every call below fails one of them, so none reaches a GPU call."""

import ctypes as C

import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)
SIZES = "bad sizes"

# name -> (an argument list that would pass, {argument index: [(bad value, message)]}, nullable indices)
CALLS = {
    # ctx, input_flags, ninput, nra, prod_a, prod_b, stack_index, nprod, nstack, all_good, redundancy
    "dmm_calc_redundancy": (
        [FAKE, BUF, 6, 63, BUF, BUF, BUF, 23, 7, 0, BUF],
        {2: [(0, SIZES), (-1, SIZES)], 3: [(0, SIZES)], 7: [(-1, SIZES)], 8: [(0, SIZES), (-7, SIZES)]},
        (),
    ),
    # ctx, vis, weight, redundancy, nfreq, nstack, nra, npol, ncell_pol, src, conj, grid_vis, grid_weight, grid_red
    "dmm_vis_grid": (
        [FAKE, BUF, BUF, BUF, 3, 7, 63, 4, 10, BUF, BUF, BUF, BUF, BUF],
        {4: [(0, SIZES)], 5: [(0, SIZES)], 6: [(-1, SIZES)], 7: [(0, SIZES)], 8: [(0, SIZES)], 3: [(None, "a redundancy grid needs the per-stack redundancy")]},
        (3, 13),
    ),
    # ctx, npol, nfreq, nx, ny, nra, npix, weight_mode, include_auto, grid_vis, grid_weight, grid_red, ns_window, nspos, el,
    # inv_wavelength, hv, hw, dirty_beam
    "dmm_beamform_ns": (
        [FAKE, 2, 2, 2, 15, 63, 63, 0, 0, BUF, BUF, BUF, BUF, BUF, BUF, BUF, BUF, BUF, BUF],
        {1: [(0, SIZES)], 2: [(0, SIZES)], 3: [(-2, SIZES)], 4: [(0, SIZES)], 5: [(0, SIZES)], 6: [(0, SIZES)],
         7: [(-1, "bad weight_mode -1"), (3, "bad weight_mode 3")]},
        (11, 12, 18),
    ),
    # ctx, npol_in, npol_out, nfreq, nx, nel, nra, single_beam, hv, hw, dirty_beam_in, pol_rotation, weight_ew, map, weight,
    # rms, dirty_beam_out
    "dmm_beamform_ew": (
        [FAKE, 4, 4, 1, 5, 33, 65, 0, BUF, BUF, BUF, BUF, BUF, BUF, BUF, BUF, BUF],
        {1: [(0, SIZES), (5, "4 input polarisations (5) are not supported")], 2: [(0, SIZES)], 3: [(0, SIZES)],
         4: [(0, SIZES), (9, "more than 8 EW baselines (9)")], 5: [(0, SIZES)], 6: [(-3, SIZES)],
         10: [(None, "dirty beam in and out go together")], 16: [(None, "dirty beam in and out go together")]},
        (10, 16),
    ),
}


def _arg_error(rc, match):
    assert rc == _lib.DMM_E_ARG, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg
    with pytest.raises(ValueError):
        _lib.check(rc)


def test_exported():
    for name in CALLS:
        assert name in _lib.EXPORTED
        assert len(getattr(_lib.lib, name).argtypes) == len(CALLS[name][0])


@pytest.mark.parametrize("name", list(CALLS))
def test_arguments(name):
    fn = getattr(_lib.lib, name)
    ok, bad, nullable = CALLS[name]

    def call(i, v):
        a = list(ok)
        a[i] = v
        return fn(*a)

    _arg_error(call(0, None), f"{name}: NULL argument")
    for i, cases in bad.items():
        for v, msg in cases:
            _arg_error(call(i, v), f"{name}: ")
            _arg_error(call(i, v), msg)
    for i, v in enumerate(ok):
        if i and v is BUF and i not in nullable:
            _arg_error(call(i, None), f"{name}: NULL argument")


def test_ns_weight_tables():
    """Natural weights need the redundancy grid, window weights their table; the inverse-variance mode needs neither
    (so dropping either there is no argument error: not called, it would run)."""
    a = list(CALLS["dmm_beamform_ns"][0])
    a[7], a[11] = 1, None
    _arg_error(_lib.lib.dmm_beamform_ns(*a), "natural weights need the redundancy grid")
    a = list(CALLS["dmm_beamform_ns"][0])
    a[7], a[12] = 2, None
    _arg_error(_lib.lib.dmm_beamform_ns(*a), "window weights need the [nfreq, ns] table")
    # the size checks come before the mode's: a bad size with a missing table is reported as the size
    a[4] = 0
    _arg_error(_lib.lib.dmm_beamform_ns(*a), SIZES)


def test_ew_limits_name_both_figures():
    a = list(CALLS["dmm_beamform_ew"][0])
    a[4] = 9
    _arg_error(_lib.lib.dmm_beamform_ew(*a), "more than 8 EW baselines (9) or 4 input polarisations (4) are not supported")
    a[4], a[1] = 8, 5
    _arg_error(_lib.lib.dmm_beamform_ew(*a), "more than 8 EW baselines (8) or 4 input polarisations (5) are not supported")
