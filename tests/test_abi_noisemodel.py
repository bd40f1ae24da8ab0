"""Argument validation of the noise-model entry points (`csrc/noisemodel.hip`), on the CPU (no GPU call is reached), in
the style of ``test_abi_hyfores.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

import ctypes as C
import re

import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)
OUT = C.c_void_p(0x3000)
NAMES = ("dmm_noisemodel_pack", "dmm_noisemodel_factor", "dmm_noisemodel_store", "dmm_noisemodel_weight", "dmm_noise_colour", "dmm_noise_hermitian")


def _arg_error(rc, match):
    assert rc == _lib.DMM_E_ARG, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg
    with pytest.raises(ValueError, match=re.escape(match)):
        _lib.check(rc)


def test_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED
    assert (_lib.DMM_NOISE_OK, _lib.DMM_NOISE_NOT_POSDEF) == (0, 1)


def _pack(ctx=FAKE, shape=(2, 64, 3, 40), first=0, nsample=100, bufs=(BUF, BUF, BUF, OUT, OUT)):
    return _lib.lib.dmm_noisemodel_pack(ctx, *shape, first, nsample, *bufs)


def _store(ctx=FAKE, shape=(2, 64, 3, 40), first=0, nsample=100, bufs=(BUF, BUF, BUF, OUT)):
    return _lib.lib.dmm_noisemodel_store(ctx, *shape, first, nsample, *bufs)


@pytest.mark.parametrize("call,nbuf,who", [(_pack, 5, "dmm_noisemodel_pack"), (_store, 4, "dmm_noisemodel_store")])
def test_pack_and_store_args(call, nbuf, who):
    _arg_error(call(ctx=None), f"{who}: ctx is NULL")
    _arg_error(call(shape=(2, 0, 3, 40)), "order 0 outside")
    _arg_error(call(shape=(2, 1025, 3, 40)), "order 1025 outside")
    _arg_error(call(shape=(0, 64, 3, 40)), "bad shape")
    _arg_error(call(shape=(2, 64, 0, 40)), "bad shape")
    _arg_error(call(shape=(2, 64, 3, 0)), "bad shape")
    _arg_error(call(shape=(300, 64, 300, 40)), "bad shape")
    _arg_error(call(nsample=0), "bad sample range")
    _arg_error(call(nsample=65536, shape=(2, 64, 3, 20000)), "bad sample range")
    _arg_error(call(first=-1), "bad sample range")
    _arg_error(call(first=200, nsample=41), "bad sample range")  # 2 x 3 x 40 = 240 samples
    assert "200 + 41" in _lib.lib.dmm_last_error().decode()
    for k in range(nbuf):
        bufs = [BUF] * nbuf
        bufs[k] = None
        _arg_error(call(bufs=tuple(bufs)), "NULL argument")


def test_factor_args():
    f = _lib.lib.dmm_noisemodel_factor
    _arg_error(f(None, 64, 10, BUF, OUT), "ctx is NULL")
    _arg_error(f(FAKE, 0, 10, BUF, OUT), "order 0 outside")
    _arg_error(f(FAKE, 1025, 10, BUF, OUT), "order 1025 outside")
    _arg_error(f(FAKE, 64, 0, BUF, OUT), "bad matrix count 0")
    _arg_error(f(FAKE, 64, 65536, BUF, OUT), "bad matrix count 65536")
    _arg_error(f(FAKE, 64, 10, None, OUT), "NULL argument")
    _arg_error(f(FAKE, 64, 10, BUF, None), "NULL argument")


def test_weight_args():
    f = _lib.lib.dmm_noisemodel_weight
    good = [BUF, BUF, BUF, BUF, OUT]
    _arg_error(f(None, 2, 64, 3, 40, 30, *good), "ctx is NULL")
    _arg_error(f(FAKE, 0, 64, 3, 40, 30, *good), "bad shape")
    _arg_error(f(FAKE, 2, 0, 3, 40, 30, *good), "bad shape")
    _arg_error(f(FAKE, 2, 65536, 3, 40, 30, *good), "bad shape")
    _arg_error(f(FAKE, 2, 64, 0, 40, 30, *good), "bad shape")
    _arg_error(f(FAKE, 2, 64, 3, 0, 30, *good), "bad shape")
    _arg_error(f(FAKE, 2, 64, 3, 40, 0, *good), "bad stack count 0")
    _arg_error(f(FAKE, 2, 64, 3, 40, 65536, *good), "bad stack count 65536")
    for k in range(5):
        bufs = list(good)
        bufs[k] = None
        _arg_error(f(FAKE, 2, 64, 3, 40, 30, *bufs), "NULL argument")


def test_colour_args():
    f = _lib.lib.dmm_noise_colour
    good = [BUF, BUF, BUF, BUF, BUF, OUT, OUT]
    _arg_error(f(None, 2, 64, 3, 5, 40, 0, 0, *good), "ctx is NULL")
    _arg_error(f(FAKE, 2, 0, 3, 5, 40, 0, 0, *good), "order 0 outside")
    _arg_error(f(FAKE, 2, 1025, 3, 5, 40, 0, 0, *good), "order 1025 outside")
    _arg_error(f(FAKE, 0, 64, 3, 5, 40, 0, 0, *good), "bad shape")
    _arg_error(f(FAKE, 2, 64, 3, 5, 0, 0, 0, *good), "bad shape")
    _arg_error(f(FAKE, 2, 64, 3, 0, 40, 0, 0, *good), "bad ns count 0")
    _arg_error(f(FAKE, 2, 64, 3, 32768, 40, 0, 0, *good), "bad ns count 32768")
    _arg_error(f(FAKE, 2, 64, 3, 5, 40, 2, 0, *good), "slab (2, 0) outside 2 x 3")
    _arg_error(f(FAKE, 2, 64, 3, 5, 40, 0, 3, *good), "slab (0, 3) outside 2 x 3")
    _arg_error(f(FAKE, 2, 64, 3, 5, 40, -1, 0, *good), "slab (-1, 0) outside 2 x 3")
    for k in range(7):
        bufs = list(good)
        bufs[k] = None
        _arg_error(f(FAKE, 2, 64, 3, 5, 40, 0, 0, *bufs), "NULL argument")


def test_hermitian_args():
    f = _lib.lib.dmm_noise_hermitian
    _arg_error(f(None, 2, 64, 3, 5, 40, BUF, OUT), "ctx is NULL")
    _arg_error(f(FAKE, 2, 0, 3, 5, 40, BUF, OUT), "order 0 outside")
    _arg_error(f(FAKE, 2, 1025, 3, 5, 40, BUF, OUT), "order 1025 outside")
    _arg_error(f(FAKE, 2, 64, 0, 5, 40, BUF, OUT), "bad shape")
    _arg_error(f(FAKE, 128, 1024, 1, 5, 40, BUF, OUT), "bad shape")  # npol * nfreq past the grid
    _arg_error(f(FAKE, 2, 64, 3, 4, 40, BUF, OUT), "odd length, got 4")
    _arg_error(f(FAKE, 2, 64, 3, 0, 40, BUF, OUT), "odd length, got 0")
    _arg_error(f(FAKE, 2, 64, 3, 5, 40, None, OUT), "NULL argument")
    _arg_error(f(FAKE, 2, 64, 3, 5, 40, BUF, None), "NULL argument")
