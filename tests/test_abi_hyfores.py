"""Argument validation of the stored-filter apply and HyFoReS entry points (`csrc/hyfores.hip`), on the CPU (no GPU call
is reached), in the style of ``test_abi_dayenu_hybrid.py``: a made-up non-NULL handle is enough to drive the host-side
checks."""

import ctypes as C

import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)
OUT = C.c_void_p(0x3000)


def _arg_error(rc, match):
    assert rc == _lib.DMM_E_ARG, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg
    with pytest.raises(ValueError, match=match):
        _lib.check(rc)


def test_exported():
    for name in ("dmm_hybrid_filter_apply", "dmm_hyfores_gain", "dmm_hyfores_window"):
        assert name in _lib.EXPORTED
    assert (_lib.DMM_HFA_OK, _lib.DMM_HFA_SKIPPED, _lib.DMM_HFA_ZERO_FILTER, _lib.DMM_HFA_MISSING_FREQ) == (0, 1, 2, 3)
    assert _lib.DMM_HYFORES_RUN == 64


def _apply(ctx=FAKE, shape=(2, 64, 3, 5, 40), filt=BUF, vis=BUF, weight=BUF, gain=None, atten=None, vis_out=OUT, weight_out=OUT, cov=None, bits=BUF, status=BUF):
    return _lib.lib.dmm_hybrid_filter_apply(ctx, *shape, filt, vis, weight, gain, atten, 0, 1, vis_out, weight_out, cov, bits, status)


def test_apply_args():
    _arg_error(_apply(ctx=None), "ctx is NULL")
    _arg_error(_apply(shape=(2, 0, 3, 5, 40)), "order 0 outside")
    _arg_error(_apply(shape=(2, 1025, 3, 5, 40)), "order 1025 outside")
    _arg_error(_apply(shape=(0, 64, 3, 5, 40)), "bad shape")
    _arg_error(_apply(shape=(2, 64, 0, 5, 40)), "bad shape")
    _arg_error(_apply(shape=(2, 64, 3, 0, 40)), "bad shape")
    _arg_error(_apply(shape=(2, 64, 3, 5, 0)), "bad shape")
    _arg_error(_apply(shape=(300, 64, 300, 5, 40)), "bad shape")
    _arg_error(_apply(shape=(2, 64, 3, 65536, 40)), "bad shape")
    _arg_error(_apply(shape=(2, 1024, 3, 65535, 40)), "do not fit the grid")
    for k in ("filt", "vis", "weight", "vis_out", "bits", "status"):
        _arg_error(_apply(**{k: None}), "NULL argument")
    _arg_error(_apply(vis_out=BUF), "out of place")
    _arg_error(_apply(weight_out=BUF), "out of place")


def test_gain_args():
    f = _lib.lib.dmm_hyfores_gain
    _arg_error(f(None, 2, 64, 3, 5, 40, BUF, BUF, BUF, BUF, None, OUT, OUT), "ctx is NULL")
    _arg_error(f(FAKE, 2, 0, 3, 5, 40, BUF, BUF, BUF, BUF, None, OUT, OUT), "order 0 outside")
    _arg_error(f(FAKE, 2, 1025, 3, 5, 40, BUF, BUF, BUF, BUF, None, OUT, OUT), "order 1025 outside")
    _arg_error(f(FAKE, 2, 64, 3, 0, 40, BUF, BUF, BUF, BUF, None, OUT, OUT), "bad shape")
    _arg_error(f(FAKE, 2, 64, 3, 5, -1, BUF, BUF, BUF, BUF, None, OUT, OUT), "bad shape")
    _arg_error(f(FAKE, 65536, 64, 1, 5, 40, BUF, BUF, BUF, BUF, None, OUT, OUT), "bad shape")
    for k in (0, 1, 2, 3, 5, 6):  # (the pixel mask, argument 4, may be NULL)
        bufs = [BUF, BUF, BUF, BUF, None, OUT, OUT]
        bufs[k] = None
        _arg_error(f(FAKE, 2, 64, 3, 5, 40, *bufs), "NULL argument")


def test_window_args():
    f = _lib.lib.dmm_hyfores_window
    _arg_error(f(None, 2, 64, 3, 5, 40, BUF, BUF, BUF, BUF, BUF, None, OUT, OUT), "ctx is NULL")
    _arg_error(f(FAKE, 2, 0, 3, 5, 40, BUF, BUF, BUF, BUF, BUF, None, OUT, OUT), "order 0 outside")
    _arg_error(f(FAKE, 2, 1025, 3, 5, 40, BUF, BUF, BUF, BUF, BUF, None, OUT, OUT), "order 1025 outside")
    _arg_error(f(FAKE, 0, 64, 3, 5, 40, BUF, BUF, BUF, BUF, BUF, None, OUT, OUT), "bad shape")
    _arg_error(f(FAKE, 2, 64, 3, 5, 0, BUF, BUF, BUF, BUF, BUF, None, OUT, OUT), "bad shape")
    for k in (0, 1, 2, 3, 4, 6, 7):
        bufs = [BUF, BUF, BUF, BUF, BUF, None, OUT, OUT]
        bufs[k] = None
        _arg_error(f(FAKE, 2, 64, 3, 5, 40, *bufs), "NULL argument")
