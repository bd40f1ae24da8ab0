"""Argument validation of the null-filter entry points, on the CPU (no GPU call is reached), in the style of
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


def _side(ptr=0x2000, ncol=8, sf=64, sc=1, si=8, so=0):
    return _lib.dmm_dayenu_side(C.c_void_p(ptr), ncol, sf, sc, si, so)


def _build(ctx=FAKE, n=64, nmat=1, k=20, low=0, tol=1e-8, samples=BUF, modes=BUF, mask=BUF, window=None, nf=BUF, sig=BUF, nkeep=BUF, status=BUF, sweeps=None):
    return _lib.lib.dmm_nullfilter_build(ctx, n, nmat, k, None, low, tol, samples, modes, mask, window, nf, sig, nkeep, status, sweeps)


def test_exported():
    for name in ("dmm_nullfilter_build", "dmm_nullfilter_mask"):
        assert name in _lib.EXPORTED


def test_build_args():
    _arg_error(_build(ctx=None), "ctx is NULL")
    _arg_error(_build(n=0), "order 0 outside")
    _arg_error(_build(n=1025), "order 1025 outside")
    _arg_error(_build(k=1), "num_modes 1 outside")
    _arg_error(_build(k=1025), "num_modes 1025 outside")
    _arg_error(_build(nmat=-1), "bad matrix count")
    _arg_error(_build(low=2), "bad filter type")
    _arg_error(_build(tol=-1.0), "tol")
    for name in ("samples", "modes", "mask", "nf", "sig", "nkeep", "status"):
        _arg_error(_build(**{name: None}), "NULL argument")
    assert _build(nmat=0, samples=None, modes=None, mask=None, nf=None, sig=None, nkeep=None, status=None) == 0  # nothing to do


def test_mask_args():
    lib = _lib.lib
    w = _side()
    _arg_error(lib.dmm_nullfilter_mask(None, 0, 0, 64, 2, 1, 0, C.byref(w), BUF), "ctx is NULL")
    _arg_error(lib.dmm_nullfilter_mask(FAKE, 3, 0, 64, 2, 1, 0, C.byref(w), BUF), "bad dtype")
    _arg_error(lib.dmm_nullfilter_mask(FAKE, 0, 2, 64, 2, 1, 0, C.byref(w), BUF), "bad layout")
    _arg_error(lib.dmm_nullfilter_mask(FAKE, 0, 0, 0, 2, 1, 0, C.byref(w), BUF), "order 0 outside")
    _arg_error(lib.dmm_nullfilter_mask(FAKE, 0, 0, 1025, 2, 1, 0, C.byref(w), BUF), "order 1025 outside")
    _arg_error(lib.dmm_nullfilter_mask(FAKE, 0, 0, 64, -2, 1, 0, C.byref(w), BUF), "bad item counts")
    _arg_error(lib.dmm_nullfilter_mask(FAKE, 0, 0, 64, 2, 1, 2, C.byref(w), BUF), "bad join_outer")
    _arg_error(lib.dmm_nullfilter_mask(FAKE, 0, 0, 64, 2, 1, 0, None, BUF), "NULL argument")
    _arg_error(lib.dmm_nullfilter_mask(FAKE, 0, 0, 64, 2, 1, 0, C.byref(w), None), "NULL argument")
    bad = _side(ncol=-1)
    _arg_error(lib.dmm_nullfilter_mask(FAKE, 0, 0, 64, 2, 1, 0, C.byref(bad), BUF), "negative count or stride")
    assert lib.dmm_nullfilter_mask(FAKE, 0, 0, 64, 0, 1, 0, C.byref(w), BUF) == 0  # no items
