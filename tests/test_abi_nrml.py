"""Argument validation of the NRML entry points, on the CPU (no GPU call is reached), in the style of
``test_abi_delay.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

import ctypes as C

import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)
NAMES = ("dmm_nrml_start", "dmm_nrml_eval", "dmm_nrml_hessian", "dmm_nrml_direction")


def _arg_error(rc, match):
    assert rc == _lib.DMM_E_ARG, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg
    with pytest.raises(ValueError, match=match):
        _lib.check(rc)


def _ws(**over):
    fields = {k: 0x2000 for k, _ in _lib.dmm_nrml_ws._fields_}
    fields["PQ"] = None
    fields.update(over)
    return _lib.dmm_nrml_ws(*[fields[k] for k, _ in _lib.dmm_nrml_ws._fields_])


def test_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)
    assert (_lib.DMM_NRML_MAX_CHAN, _lib.DMM_NRML_MAX_DELAY) == (1024, 2048)


def _start(ctx=FAKE, ndelay=32, nchan=16, nsample=6, nbase=3, bufs=None):
    bufs = [BUF] * 15 if bufs is None else bufs
    return _lib.lib.dmm_nrml_start(ctx, ndelay, nchan, nsample, nbase, *bufs)


def test_start_args():
    _arg_error(_start(ctx=None), "ctx is NULL")
    _arg_error(_start(ndelay=0), "outside")
    _arg_error(_start(ndelay=2049), "outside")
    _arg_error(_start(nchan=1025), "outside")
    _arg_error(_start(nsample=0), "bad sample count")
    _arg_error(_start(nsample=65536), "bad sample count")
    _arg_error(_start(nbase=-1), "bad baseline count")
    _arg_error(_start(nbase=65536), "bad baseline count")
    for i in range(15):
        _arg_error(_start(bufs=[None if j == i else BUF for j in range(15)]), "NULL argument")
    assert _start(nbase=0, bufs=[None] * 15) == 0  # nothing to do


def _eval(ctx=FAKE, ndelay=32, nchan=16, nbase=3, ws="default", x=BUF, lo=-1.0, hi=1.0, status=BUF, value=BUF, grad=BUF):
    w = _ws() if ws == "default" else ws
    return _lib.lib.dmm_nrml_eval(ctx, ndelay, nchan, nbase, C.byref(w) if w is not None else None, x, lo, hi, status, value, grad)


def test_eval_args():
    _arg_error(_eval(ctx=None), "ctx is NULL")
    _arg_error(_eval(ndelay=2049), "outside")
    _arg_error(_eval(nchan=0), "outside")
    _arg_error(_eval(nbase=65536), "bad baseline count")
    _arg_error(_eval(ws=None), "NULL argument")
    _arg_error(_eval(ws=_ws(Ci=None)), "NULL argument")
    _arg_error(_eval(ws=_ws(Y=None)), "NULL argument")
    _arg_error(_eval(x=None), "NULL argument")
    _arg_error(_eval(grad=None), "NULL argument")
    _arg_error(_eval(lo=2.0), "bad bounds")
    assert _eval(nbase=0, ws=None, x=None, status=None, value=None, grad=None) == 0


def _hess(ctx=FAKE, ndelay=32, nchan=16, nbase=3, ws="default", exact=1, status=BUF, H=BUF):
    w = _ws(PQ=0x2000) if ws == "default" else ws
    return _lib.lib.dmm_nrml_hessian(ctx, ndelay, nchan, nbase, C.byref(w) if w is not None else None, exact, status, H)


def test_hessian_args():
    _arg_error(_hess(ctx=None), "ctx is NULL")
    _arg_error(_hess(ndelay=2049), "outside")
    _arg_error(_hess(nchan=1025), "outside")
    _arg_error(_hess(nbase=-1), "bad baseline count")
    _arg_error(_hess(ws=_ws(R=None)), "NULL argument")
    _arg_error(_hess(H=None), "NULL argument")
    _arg_error(_hess(ws=_ws()), "NULL argument")  # without the planes PQ
    assert _hess(nbase=0, ws=None, status=None, H=None) == 0


def test_direction_args():
    lib = _lib.lib
    _arg_error(lib.dmm_nrml_direction(None, 32, 3, BUF, BUF, BUF, BUF, BUF), "ctx is NULL")
    _arg_error(lib.dmm_nrml_direction(FAKE, 0, 3, BUF, BUF, BUF, BUF, BUF), "outside")
    _arg_error(lib.dmm_nrml_direction(FAKE, 2049, 3, BUF, BUF, BUF, BUF, BUF), "outside")
    _arg_error(lib.dmm_nrml_direction(FAKE, 32, 65536, BUF, BUF, BUF, BUF, BUF), "bad baseline count")
    for i in range(5):
        _arg_error(lib.dmm_nrml_direction(FAKE, 32, 3, *[None if j == i else BUF for j in range(5)]), "NULL argument")
    assert lib.dmm_nrml_direction(FAKE, 32, 0, None, None, None, None, None) == 0
