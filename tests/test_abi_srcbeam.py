"""Argument validation of the source-beamforming entry points, on the CPU (no GPU call is reached), in the style of
``test_abi_dpss.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

import ctypes as C

import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)

# name -> (a valid argument list, {argument index: (bad value, message)}, nullable indices)
CALLS = {
    "dmm_srcbeam_prepare": (
        [FAKE, 4, 50, 64, 12, BUF, 1, BUF, BUF, BUF, BUF, BUF, BUF, BUF],
        {1: [(0, "frequency count 0 outside"), (65536, "frequency count 65536 outside")], 2: [(0, "bad stack count 0")], 3: [(-1, "bad sample count -1")],
         4: [(-1, "bad selection count -1"), (51, "bad selection count 51")], 6: [(3, "unknown weight mode 3"), (-1, "unknown weight mode -1")]},
        (),
    ),
    "dmm_srcbeam_form": (
        [FAKE, 4, 64, 12, 0, BUF, BUF, BUF, BUF, 10, 5, BUF, BUF, None, 50, BUF, BUF, BUF],
        {1: [(0, "frequency count 0 outside")], 2: [(0, "bad sample count 0")], 3: [(-1, "bad stack count -1")], 4: [(2, "unknown weight type 2")], 9: [(-1, "bad source count -1")],
         10: [(0, "bad window length 0"), (65, "window of 65 samples is longer than the axis (64)")], 14: [(-1, "bad pair count -1"), (51, "bad pair count 51")]},
        (13,),
    ),
    "dmm_srcbeam_collapse": (
        [FAKE, 4, 64, 2, 10, 5, 1, 0, 0, BUF, None, BUF, BUF, BUF, None, BUF, 12, BUF, BUF],
        {1: [(65536, "frequency count 65536 outside")], 2: [(0, "bad sample count 0")], 3: [(0, "polarisation count 0 outside"), (5, "polarisation count 5 outside")],
         4: [(-1, "bad source count -1")], 5: [(0, "bad window length 0"), (65, "window of 65 samples is longer than the axis (64)")], 16: [(9, "9 output rows for 10 sources")]},
        (10, 14),
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
    assert (_lib.DMM_SRCBEAM_INVERSE_VARIANCE, _lib.DMM_SRCBEAM_NATURAL, _lib.DMM_SRCBEAM_UNIFORM) == (0, 1, 2)
    assert (_lib.DMM_SRCBEAM_W_F32, _lib.DMM_SRCBEAM_W_F64) == (0, 1)


@pytest.mark.parametrize("name", list(CALLS))
def test_arguments(name):
    fn = getattr(_lib.lib, name)
    ok, bad, nullable = CALLS[name]

    def call(i, v):
        a = list(ok)
        a[i] = v
        return fn(*a)

    _arg_error(call(0, None), "ctx is NULL")
    for i, cases in bad.items():
        for v, msg in cases:
            _arg_error(call(i, v), msg)
    for i, v in enumerate(ok):
        if i and v is BUF and i not in nullable:
            _arg_error(call(i, None), "NULL argument")


def test_redundancy_needed_unless_inverse_variance():
    a = list(CALLS["dmm_srcbeam_prepare"][0])
    a[9] = None
    _arg_error(_lib.lib.dmm_srcbeam_prepare(*a), "NULL argument")


@pytest.mark.parametrize("name", ["dmm_srcbeam_form", "dmm_srcbeam_collapse"])
def test_no_sources(name):
    a = list(CALLS[name][0])
    a[{"dmm_srcbeam_form": 9, "dmm_srcbeam_collapse": 4}[name]] = 0
    if name == "dmm_srcbeam_form":
        a[14] = 0
    assert getattr(_lib.lib, name)(*a) == 0  # nothing to do
