"""Argument validation of the DAYENU entry points, on the CPU (no GPU call is reached), in the style of
``test_abi_args.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

import ctypes as C

import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)


def _arg_error(rc, match):
    assert rc == _lib.DMM_E_ARG, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg
    with pytest.raises(ValueError, match=match):
        _lib.check(rc)


def _side(ptr=0x2000, ncol=8, sf=64, sc=1, si=8, so=0):
    return _lib.dmm_dayenu_side(C.c_void_p(ptr), ncol, sf, sc, si, so)


def test_exported():
    for name in ("dmm_dayenu_build", "dmm_dayenu_mask", "dmm_dayenu_apply"):
        assert name in _lib.EXPORTED


def test_build_args():
    lib = _lib.lib
    _arg_error(lib.dmm_dayenu_build(None, 64, 1, 1, BUF, BUF, BUF, BUF, BUF), "ctx is NULL")
    _arg_error(lib.dmm_dayenu_build(FAKE, 0, 1, 1, BUF, BUF, BUF, BUF, BUF), "order 0 outside")
    _arg_error(lib.dmm_dayenu_build(FAKE, 1025, 1, 1, BUF, BUF, BUF, BUF, BUF), "order 1025 outside")
    _arg_error(lib.dmm_dayenu_build(FAKE, 64, -1, 1, BUF, BUF, BUF, BUF, BUF), "bad matrix count")
    _arg_error(lib.dmm_dayenu_build(FAKE, 64, 1, 0, BUF, BUF, BUF, BUF, BUF), "bad stop band count")
    _arg_error(lib.dmm_dayenu_build(FAKE, 64, 1, 1, None, BUF, BUF, BUF, BUF), "NULL argument")
    _arg_error(lib.dmm_dayenu_build(FAKE, 64, 1, 1, BUF, BUF, BUF, BUF, None), "NULL argument")
    assert lib.dmm_dayenu_build(FAKE, 64, 0, 1, None, None, None, None, None) == 0  # nothing to do


def test_mask_args():
    lib = _lib.lib
    w = _side()
    _arg_error(lib.dmm_dayenu_mask(None, 0, 0, 64, 2, 1, C.byref(w), BUF), "ctx is NULL")
    _arg_error(lib.dmm_dayenu_mask(FAKE, 3, 0, 64, 2, 1, C.byref(w), BUF), "bad dtype")
    _arg_error(lib.dmm_dayenu_mask(FAKE, 0, 2, 64, 2, 1, C.byref(w), BUF), "bad layout")
    _arg_error(lib.dmm_dayenu_mask(FAKE, 0, 0, 0, 2, 1, C.byref(w), BUF), "order 0 outside")
    _arg_error(lib.dmm_dayenu_mask(FAKE, 0, 0, 64, -2, 1, C.byref(w), BUF), "bad item counts")
    _arg_error(lib.dmm_dayenu_mask(FAKE, 0, 0, 64, 2, 1, None, BUF), "NULL argument")
    _arg_error(lib.dmm_dayenu_mask(FAKE, 0, 0, 64, 2, 1, C.byref(w), None), "NULL argument")
    bad = _side(ncol=-1)
    _arg_error(lib.dmm_dayenu_mask(FAKE, 0, 0, 64, 2, 1, C.byref(bad), BUF), "negative count or stride")


def test_apply_args():
    lib = _lib.lib
    d, w = _side(ncol=16, sf=128, si=16), _side()
    _arg_error(lib.dmm_dayenu_apply(None, 0, 0, 64, 2, 1, BUF, 1, BUF, None, None, 2, C.byref(d), C.byref(w)), "ctx is NULL")
    _arg_error(lib.dmm_dayenu_apply(FAKE, 2, 0, 64, 2, 1, BUF, 1, BUF, None, None, 2, C.byref(d), C.byref(w)), "bad dtype")
    _arg_error(lib.dmm_dayenu_apply(FAKE, 0, -1, 64, 2, 1, BUF, 1, BUF, None, None, 2, C.byref(d), C.byref(w)), "bad layout")
    _arg_error(lib.dmm_dayenu_apply(FAKE, 0, 0, 0, 2, 1, BUF, 1, BUF, None, None, 2, C.byref(d), C.byref(w)), "order 0 outside")
    _arg_error(lib.dmm_dayenu_apply(FAKE, 0, 0, 64, 2, 1, BUF, -1, BUF, None, None, 2, C.byref(d), C.byref(w)), "negative count")
    _arg_error(lib.dmm_dayenu_apply(FAKE, 0, 0, 64, 2, 1, BUF, 1, BUF, None, None, -2, C.byref(d), C.byref(w)), "negative count")
    _arg_error(lib.dmm_dayenu_apply(FAKE, 0, 0, 64, 2, 1, None, 1, BUF, None, None, 2, C.byref(d), C.byref(w)), "NULL argument")
    _arg_error(lib.dmm_dayenu_apply(FAKE, 0, 0, 64, 2, 1, BUF, 1, None, None, None, 2, C.byref(d), C.byref(w)), "NULL argument")
    _arg_error(lib.dmm_dayenu_apply(FAKE, 0, 0, 64, 2, 1, BUF, 1, BUF, None, None, 2, None, None), "neither data nor weight")
    bad = _side(sf=-4)
    _arg_error(lib.dmm_dayenu_apply(FAKE, 0, 0, 64, 2, 1, BUF, 1, BUF, None, None, 2, C.byref(bad), C.byref(w)), "negative count or stride")
    assert lib.dmm_dayenu_apply(FAKE, 0, 0, 64, 2, 1, BUF, 1, BUF, None, None, 0, C.byref(d), C.byref(w)) == 0  # no units
