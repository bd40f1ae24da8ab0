"""Argument validation of the hybrid-visibility DAYENU and east-west average entry points, on the CPU (no GPU call is
reached), in the style of ``test_abi_dayenu.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

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


def test_exported():
    for name in ("dmm_dayenu_hybrid_mask", "dmm_dayenu_hybrid_save", "dmm_dayenu_hybrid_cov", "dmm_ew_coef", "dmm_ew_scale", "dmm_ew_average"):
        assert name in _lib.EXPORTED
    assert (_lib.DMM_EW_TABLE, _lib.DMM_EW_INVERSE_VARIANCE) == (0, 1)


def test_mask_args():
    f = _lib.lib.dmm_dayenu_hybrid_mask
    _arg_error(f(None, 2, 64, 3, 40, BUF, BUF), "ctx is NULL")
    _arg_error(f(FAKE, 2, 0, 3, 40, BUF, BUF), "order 0 outside")
    _arg_error(f(FAKE, 2, 1025, 3, 40, BUF, BUF), "order 1025 outside")
    _arg_error(f(FAKE, 0, 64, 3, 40, BUF, BUF), "bad shape")
    _arg_error(f(FAKE, 2, 64, 0, 40, BUF, BUF), "bad shape")
    _arg_error(f(FAKE, 2, 64, 3, 0, BUF, BUF), "bad shape")
    _arg_error(f(FAKE, 2, 64, 3, 40, None, BUF), "NULL argument")
    _arg_error(f(FAKE, 2, 64, 3, 40, BUF, None), "NULL argument")


def test_save_args():
    f = _lib.lib.dmm_dayenu_hybrid_save
    _arg_error(f(None, 2, 64, 3, 40, BUF, 1, BUF, 0, BUF), "ctx is NULL")
    _arg_error(f(FAKE, 2, 0, 3, 40, BUF, 1, BUF, 0, BUF), "order 0 outside")
    _arg_error(f(FAKE, 2, 1025, 3, 40, BUF, 1, BUF, 0, BUF), "order 1025 outside")
    _arg_error(f(FAKE, 2, 64, 3, -1, BUF, 1, BUF, 0, BUF), "bad shape")
    _arg_error(f(FAKE, 65536, 64, 3, 40, BUF, 1, BUF, 0, BUF), "bad shape")
    _arg_error(f(FAKE, 2, 64, 3, 40, BUF, -1, BUF, 0, BUF), "bad matrix count")
    _arg_error(f(FAKE, 2, 64, 3, 40, None, 1, BUF, 0, BUF), "NULL argument")
    _arg_error(f(FAKE, 2, 64, 3, 40, BUF, 1, None, 0, BUF), "NULL argument")
    _arg_error(f(FAKE, 2, 64, 3, 40, BUF, 1, BUF, 0, None), "NULL argument")


def test_cov_args():
    f = _lib.lib.dmm_dayenu_hybrid_cov
    _arg_error(f(None, 2, 64, 3, 40, BUF, 1, BUF, BUF, 0, BUF), "ctx is NULL")
    _arg_error(f(FAKE, 2, 0, 3, 40, BUF, 1, BUF, BUF, 0, BUF), "order 0 outside")
    _arg_error(f(FAKE, 2, 1025, 3, 40, BUF, 1, BUF, BUF, 0, BUF), "order 1025 outside")
    _arg_error(f(FAKE, 2, 64, 0, 40, BUF, 1, BUF, BUF, 0, BUF), "bad shape")
    _arg_error(f(FAKE, 300, 64, 300, 40, BUF, 1, BUF, BUF, 0, BUF), "do not fit the grid")
    _arg_error(f(FAKE, 2, 64, 3, 40, BUF, -2, BUF, BUF, 0, BUF), "bad matrix count")
    _arg_error(f(FAKE, 2, 64, 3, 40, None, 1, BUF, BUF, 0, BUF), "NULL argument")
    _arg_error(f(FAKE, 2, 64, 3, 40, BUF, 1, None, BUF, 0, BUF), "NULL argument")
    _arg_error(f(FAKE, 2, 64, 3, 40, BUF, 1, BUF, None, 0, BUF), "NULL argument")
    _arg_error(f(FAKE, 2, 64, 3, 40, BUF, 1, BUF, BUF, 0, None), "NULL argument")


def test_ew_coef_args():
    f = _lib.lib.dmm_ew_coef
    _arg_error(f(None, 2, 64, 3, 40, 0, BUF, BUF, BUF, BUF, BUF, BUF), "ctx is NULL")
    _arg_error(f(FAKE, 0, 64, 3, 40, 0, BUF, BUF, BUF, BUF, BUF, BUF), "bad shape")
    _arg_error(f(FAKE, 2, 64, 3, 0, 0, BUF, BUF, BUF, BUF, BUF, BUF), "bad shape")
    _arg_error(f(FAKE, 2, 64, 0, 40, 0, BUF, BUF, BUF, BUF, BUF, BUF), "0 east-west baselines outside")
    _arg_error(f(FAKE, 2, 64, 65, 40, 0, BUF, BUF, BUF, BUF, BUF, BUF), "65 east-west baselines outside")
    _arg_error(f(FAKE, 2, 64, 3, 40, 2, BUF, BUF, BUF, BUF, BUF, BUF), "bad scheme")
    for k in range(6):
        bufs = [BUF] * 6
        bufs[k] = None
        _arg_error(f(FAKE, 2, 64, 3, 40, 1, *bufs), "NULL argument")


def test_ew_scale_args():
    f = _lib.lib.dmm_ew_scale
    _arg_error(f(None, 2, 64, 3, 40, 5, BUF, BUF, BUF, BUF), "ctx is NULL")
    _arg_error(f(FAKE, 2, 64, 3, 40, 0, BUF, BUF, BUF, BUF), "bad shape")
    _arg_error(f(FAKE, 2, 64, 0, 40, 5, BUF, BUF, BUF, BUF), "bad shape")
    _arg_error(f(FAKE, 64, 1024, 3, 40, 5, BUF, BUF, BUF, BUF), "bad shape")
    for k in range(4):
        bufs = [BUF] * 4
        bufs[k] = None
        _arg_error(f(FAKE, 2, 64, 3, 40, 5, *bufs), "NULL argument")


def test_ew_average_args():
    f = _lib.lib.dmm_ew_average
    _arg_error(f(None, 100, 10, 3, 40, BUF, BUF, BUF), "ctx is NULL")
    _arg_error(f(FAKE, -1, 10, 3, 40, BUF, BUF, BUF), "bad shape")
    _arg_error(f(FAKE, 100, 0, 3, 40, BUF, BUF, BUF), "bad shape")
    _arg_error(f(FAKE, 100, 10, 0, 40, BUF, BUF, BUF), "bad shape")
    _arg_error(f(FAKE, 100, 10, 3, 0, BUF, BUF, BUF), "bad shape")
    _arg_error(f(FAKE, 65535 * 65536, 10, 3, 40, BUF, BUF, BUF), "do not fit the grid")
    _arg_error(f(FAKE, 100, 10, 3, 40, None, BUF, BUF), "NULL argument")
    _arg_error(f(FAKE, 100, 10, 3, 40, BUF, None, BUF), "NULL argument")
    _arg_error(f(FAKE, 100, 10, 3, 40, BUF, BUF, None), "NULL argument")
    assert f(FAKE, 0, 10, 3, 40, None, None, None) == 0  # nothing to do
