"""Argument validation of the Wiener delay transform's entry points, on the CPU (no GPU call is reached), in the style
of ``test_abi_powerspec.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

import ctypes as C

import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)
NAMES = ("dmm_wienerdelay_build", "dmm_wienerdelay_apply")


def _arg_error(rc, match):
    assert rc == _lib.DMM_E_ARG, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg
    with pytest.raises(ValueError, match=match):
        _lib.check(rc)


def test_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)
    assert _lib.DMM_WD_MAX_FREQ == 1024


def _build(ctx=FAKE, npol=2, nfreq=8, nra=3, nel=5, ndelay=4, bufs=None, dtype=_lib.DMM_C64, ws=0, bad=True):
    bufs = [BUF] * 9 if bufs is None else bufs
    first = C.c_int64(7)
    rc = _lib.lib.dmm_wienerdelay_build(ctx, npol, nfreq, nra, nel, ndelay, *bufs, dtype, ws, C.byref(first) if bad else None)
    return rc, first.value


def test_build_args():
    _arg_error(_build(ctx=None)[0], "ctx is NULL")
    _arg_error(_build(nfreq=0)[0], "nfreq 0 outside")
    _arg_error(_build(nfreq=1025, ndelay=8)[0], "nfreq 1025 outside")
    _arg_error(_build(ndelay=0)[0], "ndelay 0 outside")
    _arg_error(_build(ndelay=9)[0], "ndelay 9 outside")
    for kw in ({"npol": -1}, {"nra": -3}, {"nel": -5}):
        _arg_error(_build(**kw)[0], "negative count")
    _arg_error(_build(dtype=2)[0], "bad output dtype 2")
    _arg_error(_build(dtype=-1)[0], "bad output dtype -1")
    _arg_error(_build(ws=-1)[0], "negative workspace")
    _arg_error(_build(bad=False)[0], "first_bad is NULL")
    for i in range(9):
        bufs = [BUF] * 9
        bufs[i] = None
        _arg_error(_build(bufs=bufs)[0], "NULL argument")


def test_build_nothing_to_do():
    # no pixel: nothing is launched, not even with NULL arrays, and no pixel is reported
    for kw in ({"npol": 0}, {"nra": 0}, {"nel": 0}):
        rc, first = _build(bufs=[None] * 9, **kw)
        assert rc == 0 and first == -1


def _apply(ctx=FAKE, npol=2, nfreq=8, nra=3, nel=5, ndelay=4, bufs=None, dtype=_lib.DMM_C64):
    op, m, w, spec, sw = [BUF] * 5 if bufs is None else bufs
    return _lib.lib.dmm_wienerdelay_apply(ctx, npol, nfreq, nra, nel, ndelay, op, dtype, m, w, spec, sw)


def test_apply_args():
    _arg_error(_apply(ctx=None), "ctx is NULL")
    _arg_error(_apply(nfreq=0), "nfreq 0 outside")
    _arg_error(_apply(nfreq=1025), "nfreq 1025 outside")
    _arg_error(_apply(ndelay=0), "bad delay count")
    for kw in ({"npol": -1}, {"nra": -3}, {"nel": -5}, {"npol": 65536}, {"nra": 65536}):
        _arg_error(_apply(**kw), "bad count")
    _arg_error(_apply(dtype=3), "bad operator dtype 3")
    for i in range(5):
        bufs = [BUF] * 5
        bufs[i] = None
        _arg_error(_apply(bufs=bufs), "NULL argument")
    for kw in ({"npol": 0}, {"nra": 0}, {"nel": 0}):
        assert _apply(bufs=[None] * 5, **kw) == 0
