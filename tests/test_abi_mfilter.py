"""Argument validation of the DAYENU m-mode filter entry points, on the CPU (no GPU call is reached), in the style of
``test_abi_dayenu.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

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
    for name in ("dmm_mfilter_mask", "dmm_mfilter_cov", "dmm_mfilter_pack", "dmm_mfilter_unpack", "dmm_mfilter_solve", "dmm_mfilter_eye"):
        assert name in _lib.EXPORTED


def test_mask_args():
    lib = _lib.lib
    _arg_error(lib.dmm_mfilter_mask(None, 2, 3, 64, BUF, BUF, BUF), "ctx is NULL")
    _arg_error(lib.dmm_mfilter_mask(FAKE, 2, 3, 0, BUF, BUF, BUF), "order 0 outside")
    _arg_error(lib.dmm_mfilter_mask(FAKE, 2, 3, 4097, BUF, BUF, BUF), "order 4097 outside")
    _arg_error(lib.dmm_mfilter_mask(FAKE, -1, 3, 64, BUF, BUF, BUF), "bad frequency or stack count")
    _arg_error(lib.dmm_mfilter_mask(FAKE, 2, 0, 64, BUF, BUF, BUF), "bad frequency or stack count")
    _arg_error(lib.dmm_mfilter_mask(FAKE, 2, 3, 64, None, BUF, BUF), "NULL argument")
    _arg_error(lib.dmm_mfilter_mask(FAKE, 2, 3, 64, BUF, BUF, None), "NULL argument")
    assert lib.dmm_mfilter_mask(FAKE, 0, 3, 64, None, None, None) == 0  # nothing to do


def test_cov_args():
    lib = _lib.lib
    _arg_error(lib.dmm_mfilter_cov(None, 64, 1, BUF, BUF, BUF, BUF, BUF), "ctx is NULL")
    _arg_error(lib.dmm_mfilter_cov(FAKE, 0, 1, BUF, BUF, BUF, BUF, BUF), "order 0 outside")
    _arg_error(lib.dmm_mfilter_cov(FAKE, 4097, 1, BUF, BUF, BUF, BUF, BUF), "order 4097 outside")
    _arg_error(lib.dmm_mfilter_cov(FAKE, 64, -1, BUF, BUF, BUF, BUF, BUF), "bad matrix count")
    _arg_error(lib.dmm_mfilter_cov(FAKE, 64, 65536, BUF, BUF, BUF, BUF, BUF), "bad matrix count")
    _arg_error(lib.dmm_mfilter_cov(FAKE, 64, 1, None, BUF, BUF, BUF, BUF), "NULL argument")
    _arg_error(lib.dmm_mfilter_cov(FAKE, 64, 1, BUF, BUF, BUF, BUF, None), "NULL argument")
    assert lib.dmm_mfilter_cov(FAKE, 64, 0, None, None, None, None, None) == 0


@pytest.mark.parametrize("name", ["dmm_mfilter_pack", "dmm_mfilter_unpack"])
def test_pack_unpack_args(name):
    fn = getattr(_lib.lib, name)
    ok = [FAKE, 64, 3, 1, 2, BUF, BUF, None, BUF, BUF, BUF, BUF, BUF]  # (mix may be NULL: no mixer)

    def call(**over):
        a = list(ok)
        for k, v in over.items():
            a[int(k[1:])] = v
        return fn(*a)

    _arg_error(call(p0=None), "ctx is NULL")
    _arg_error(call(p1=0), "order 0 outside")
    _arg_error(call(p1=4097), "order 4097 outside")
    _arg_error(call(p2=0), "bad stack size")
    _arg_error(call(p3=-1), "bad matrix or entry count")
    _arg_error(call(p4=-2), "bad matrix or entry count")
    for k in (5, 6, 8, 9, 10, 11, 12):
        _arg_error(call(**{f"p{k}": None}), "NULL argument")
    assert call(p3=0) == 0 and call(p4=0) == 0  # nothing to do


def test_solve_args():
    lib = _lib.lib
    _arg_error(lib.dmm_mfilter_solve(None, 64, 4, 1, BUF, BUF, BUF), "ctx is NULL")
    _arg_error(lib.dmm_mfilter_solve(FAKE, 0, 4, 1, BUF, BUF, BUF), "order 0 outside")
    _arg_error(lib.dmm_mfilter_solve(FAKE, 4097, 4, 1, BUF, BUF, BUF), "order 4097 outside")
    _arg_error(lib.dmm_mfilter_solve(FAKE, 64, -1, 1, BUF, BUF, BUF), "bad row count")
    _arg_error(lib.dmm_mfilter_solve(FAKE, 64, 4, -1, BUF, BUF, BUF), "bad matrix count")
    _arg_error(lib.dmm_mfilter_solve(FAKE, 64, 4, 1, None, BUF, BUF), "NULL argument")
    _arg_error(lib.dmm_mfilter_solve(FAKE, 64, 4, 1, BUF, None, BUF), "NULL argument")
    _arg_error(lib.dmm_mfilter_solve(FAKE, 64, 4, 1, BUF, BUF, None), "NULL argument")
    assert lib.dmm_mfilter_solve(FAKE, 64, 4, 0, None, None, None) == 0


def test_eye_args():
    lib = _lib.lib
    _arg_error(lib.dmm_mfilter_eye(None, 64, 1, 0, BUF, BUF, BUF), "ctx is NULL")
    _arg_error(lib.dmm_mfilter_eye(FAKE, 0, 1, 0, BUF, BUF, BUF), "order 0 outside")
    _arg_error(lib.dmm_mfilter_eye(FAKE, 4097, 1, 0, BUF, BUF, BUF), "order 4097 outside")
    _arg_error(lib.dmm_mfilter_eye(FAKE, 64, -1, 0, BUF, BUF, BUF), "bad matrix count")
    _arg_error(lib.dmm_mfilter_eye(FAKE, 64, 1, 2, BUF, BUF, BUF), "bad stage")
    _arg_error(lib.dmm_mfilter_eye(FAKE, 64, 1, 1, None, BUF, BUF), "NULL argument")
    _arg_error(lib.dmm_mfilter_eye(FAKE, 64, 1, 1, BUF, BUF, None), "NULL argument")
    assert lib.dmm_mfilter_eye(FAKE, 64, 0, 0, None, None, None) == 0
