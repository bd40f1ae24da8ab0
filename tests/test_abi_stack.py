"""Argument validation of the source-stacking entry points, on the CPU (no GPU call is reached), in the style of
``test_abi_srcbeam.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

import ctypes as C

import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)

# name -> (a valid argument list, {argument index: (bad value, message)}, nullable indices)
CALLS = {
    "dmm_ringmap_extract": (
        [FAKE, 4, 12, 32, 24, BUF, BUF, 0, 40, BUF, BUF, BUF, BUF, BUF],
        {1: [(0, "polarisation count 0 outside"), (5, "polarisation count 5 outside")], 2: [(0, "frequency count 0 outside"), (65536, "frequency count 65536 outside")],
         3: [(0, "bad ra count 0")], 4: [(-1, "bad el count -1")], 7: [(2, "unknown weight source 2")], 8: [(-1, "bad source count -1"), (1 << 31, "too many sources")]},
        (11,),
    ),
    "dmm_source_stack": (
        [FAKE, 40, 4, 12, 5, BUF, BUF, BUF, 1, BUF, None, BUF, 0, 0, BUF, 1, BUF, BUF, BUF],
        {1: [(-1, "bad source count -1")], 2: [(0, "polarisation count 0 outside"), (5, "polarisation count 5 outside")],
         3: [(0, "frequency count 0 outside"), (_lib.DMM_STACK_MAX_FREQ + 1, f"frequency count {_lib.DMM_STACK_MAX_FREQ + 1} outside")],
         4: [(0, "stack length 0 outside"), (13, "stack length 13 outside 1 ... 12")], 15: [(0, "room for 0 chunks")]},
        (10,),
    ),
    "dmm_ringmap_stack3d": (
        [FAKE, 4, 12, 32, 24, BUF, BUF, 0, 0, None, 40, BUF, BUF, BUF, BUF, 1, 5, BUF, 2, 3, 1, BUF, 1, BUF, BUF, BUF],
        {1: [(0, "polarisation count 0 outside")], 2: [(0, "frequency count 0 outside")], 3: [(0, "bad ra count 0")], 4: [(0, "bad el count 0")], 7: [(-1, "unknown weight source -1")],
         8: [(3, "unknown weight mode 3"), (-1, "unknown weight mode -1")], 10: [(-1, "bad source count -1")], 16: [(0, "bin count 0 outside"), (20000, "bin count 20000 outside")],
         18: [(16, "a patch of 33 pixels is longer than the ra axis (32)"), (-1, "longer than the ra axis")], 19: [(12, "a patch of 25 pixels is longer than the el axis (24)")],
         22: [(0, "room for 0 chunks")]},
        (9,),
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
    assert (_lib.DMM_STACK3D_INPUT, _lib.DMM_STACK3D_DEC, _lib.DMM_STACK3D_PATCH) == (0, 1, 2)
    assert _lib.DMM_STACK_SRC_CHUNK == 256 and _lib.DMM_STACK_MAX_FREQ == 2048


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


def test_dec_mode_needs_the_strip_weights():
    a = list(CALLS["dmm_ringmap_stack3d"][0])
    a[8] = _lib.DMM_STACK3D_DEC
    _arg_error(_lib.lib.dmm_ringmap_stack3d(*a), "NULL argument")


def test_extract_no_sources():
    a = list(CALLS["dmm_ringmap_extract"][0])
    a[8] = 0
    assert _lib.lib.dmm_ringmap_extract(*a) == 0  # nothing to do, nothing launched
