"""Argument validation of the delay-spectrum entry points, on the CPU (no GPU call is reached), in the style of
``test_abi_dayenu.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

import ctypes as C

import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)
NAMES = ("dmm_delay_fourier", "dmm_delay_prepare", "dmm_delay_project", "dmm_delay_solve", "dmm_delay_store")


def _arg_error(rc, match):
    assert rc == _lib.DMM_E_ARG, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg
    with pytest.raises(ValueError, match=match):
        _lib.check(rc)


def _view(ptr=0x2000, dtype=_lib.DMM_DELAY_C64, ss=1, sf=64, fold=(8, 0, 0, 0)):
    return _lib.dmm_delay_view(C.c_void_p(ptr), dtype, ss, sf, (C.c_int64 * 4)(*fold))


def test_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)


def test_fourier_args():
    lib = _lib.lib
    _arg_error(lib.dmm_delay_fourier(None, 32, 17, 0, BUF, BUF), "ctx is NULL")
    _arg_error(lib.dmm_delay_fourier(FAKE, 0, 17, 0, BUF, BUF), "bad sizes")
    _arg_error(lib.dmm_delay_fourier(FAKE, 32, -1, 0, BUF, BUF), "bad sizes")
    _arg_error(lib.dmm_delay_fourier(FAKE, 32, 17, 0, None, BUF), "NULL argument")
    _arg_error(lib.dmm_delay_fourier(FAKE, 32, 17, 0, BUF, None), "NULL argument")


def _prepare(ctx=FAKE, ndelay=32, nchan=17, nsample=5, nbase=3, base0=0, nfold=1, fold=(3,), data=None, weight=None, coef=BUF, chan=BUF, X=BUF, nzt=BUF, status=BUF):
    d = _view() if data is None else data
    w = _view(dtype=_lib.DMM_DELAY_F32) if weight is None else weight
    fold_n = (C.c_int64 * 4)(*(list(fold) + [0] * (4 - len(fold)))) if fold is not None else None
    return _lib.lib.dmm_delay_prepare(ctx, ndelay, nchan, nsample, nbase, base0, nfold, fold_n, C.byref(d) if d else None, C.byref(w) if w else None, 0, 1, 1, 0.0, 0.0, 1.0, coef, chan, X, nzt, status)


def test_prepare_args():
    _arg_error(_prepare(ctx=None), "ctx is NULL")
    _arg_error(_prepare(nchan=0), "bad sizes")
    _arg_error(_prepare(nsample=-5), "bad sizes")
    _arg_error(_prepare(nbase=-1), "bad baseline count")
    _arg_error(_prepare(nbase=65536), "bad baseline count")
    _arg_error(_prepare(nfold=5), "folded axes")
    _arg_error(_prepare(coef=None), "NULL argument")
    _arg_error(_prepare(status=None), "NULL argument")
    _arg_error(_prepare(data=_view(ptr=0)), "NULL argument")
    _arg_error(_prepare(data=_view(sf=-1)), "negative stride")
    _arg_error(_prepare(data=_view(dtype=7)), "bad data dtype")
    _arg_error(_prepare(weight=_view(dtype=_lib.DMM_DELAY_C64)), "bad weight dtype")
    _arg_error(_prepare(fold=(0,)), "bad length of folded axis")
    assert _prepare(nbase=0, coef=None, chan=None, X=None, nzt=None, status=None) == 0  # nothing to do


def test_project_args():
    lib = _lib.lib
    _arg_error(lib.dmm_delay_project(None, 32, 17, 6, 3, BUF, BUF, BUF, BUF), "ctx is NULL")
    _arg_error(lib.dmm_delay_project(FAKE, 0, 17, 6, 3, BUF, BUF, BUF, BUF), "bad sizes")
    _arg_error(lib.dmm_delay_project(FAKE, 32, 17, -6, 3, BUF, BUF, BUF, BUF), "bad sizes")
    _arg_error(lib.dmm_delay_project(FAKE, 32, 17, 6, -3, BUF, BUF, BUF, BUF), "bad baseline count")
    _arg_error(lib.dmm_delay_project(FAKE, 32, 17, 6, 3, None, BUF, BUF, BUF), "NULL argument")
    _arg_error(lib.dmm_delay_project(FAKE, 32, 17, 6, 3, BUF, BUF, BUF, None), "NULL argument")
    assert lib.dmm_delay_project(FAKE, 32, 17, 6, 0, None, None, None, None) == 0


def test_solve_args():
    lib = _lib.lib
    _arg_error(lib.dmm_delay_solve(None, 32, 0, 5, 3, BUF, BUF, BUF, BUF), "ctx is NULL")
    _arg_error(lib.dmm_delay_solve(FAKE, 0, 0, 5, 3, BUF, BUF, BUF, BUF), "order 0 outside")
    _arg_error(lib.dmm_delay_solve(FAKE, 2049, 0, 5, 3, BUF, BUF, BUF, BUF), "order 2049 outside")
    _arg_error(lib.dmm_delay_solve(FAKE, 47, 1, 5, 3, BUF, BUF, BUF, BUF), "odd order")
    _arg_error(lib.dmm_delay_solve(FAKE, 32, 0, 0, 3, BUF, BUF, BUF, BUF), "bad sample count")
    _arg_error(lib.dmm_delay_solve(FAKE, 32, 0, 5, -3, BUF, BUF, BUF, BUF), "bad baseline count")
    _arg_error(lib.dmm_delay_solve(FAKE, 32, 0, 5, 3, BUF, None, BUF, BUF), "NULL argument")
    _arg_error(lib.dmm_delay_solve(FAKE, 32, 0, 5, 3, BUF, BUF, None, BUF), "NULL argument")
    assert lib.dmm_delay_solve(FAKE, 2048, 0, 5, 0, None, None, None, None) == 0


def test_store_args():
    lib = _lib.lib
    _arg_error(lib.dmm_delay_store(None, 32, 0, 5, 6, 3, BUF, BUF, BUF, BUF, None), "ctx is NULL")
    _arg_error(lib.dmm_delay_store(FAKE, 0, 0, 5, 6, 3, BUF, BUF, BUF, BUF, None), "bad sizes")
    _arg_error(lib.dmm_delay_store(FAKE, 32, 0, 5, 4, 3, BUF, BUF, BUF, BUF, None), "bad sizes")
    _arg_error(lib.dmm_delay_store(FAKE, 32, 0, 5, 6, -3, BUF, BUF, BUF, BUF, None), "bad baseline count")
    _arg_error(lib.dmm_delay_store(FAKE, 32, 0, 5, 6, 3, BUF, BUF, BUF, None, None), "NULL argument")
    assert lib.dmm_delay_store(FAKE, 32, 0, 5, 6, 0, None, None, None, None, None) == 0
