"""Argument validation of the power-spectrum entry points, on the CPU (no GPU call is reached), in the style of
``test_abi_delay.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

import ctypes as C

import numpy as np
import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)
NAMES = ("dmm_uv_fft2_supported", "dmm_uv_fft2", "dmm_ps3d_cross", "dmm_ps_cyl_bin")


def _error(rc, code, match):
    assert rc == code, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg


def _arg_error(rc, match):
    _error(rc, _lib.DMM_E_ARG, match)
    with pytest.raises(ValueError, match=match):
        _lib.check(rc)


def test_exported():
    for name in NAMES:
        assert name in _lib.EXPORTED and hasattr(_lib.lib, name)


def test_supported_lengths():
    ok = _lib.lib.dmm_uv_fft2_supported
    assert all(ok(n) for n in (1, 2, 3, 500, 2048, 2049, 4095, 4096, 8192))
    assert not any(ok(n) for n in (0, -4, 4097, 6000, 8191, 8193, 16384))


def test_uv_fft2_args():
    f = _lib.lib.dmm_uv_fft2
    _arg_error(f(None, BUF, 2, 8, 16, 5, BUF, BUF, BUF, 0), "ctx is NULL")
    _arg_error(f(FAKE, BUF, 0, 8, 16, 5, BUF, BUF, BUF, 0), "bad sizes")
    _arg_error(f(FAKE, BUF, 2, -8, 16, 5, BUF, BUF, BUF, 0), "bad sizes")
    _arg_error(f(FAKE, BUF, 2, 8, 0, 5, BUF, BUF, BUF, 0), "bad sizes")
    _arg_error(f(FAKE, BUF, 2, 8, 16, 0, BUF, BUF, BUF, 0), "bad sizes")
    _arg_error(f(FAKE, None, 2, 8, 16, 5, BUF, BUF, BUF, 0), "NULL argument")
    _arg_error(f(FAKE, BUF, 2, 8, 16, 5, BUF, BUF, None, 0), "NULL argument")
    _arg_error(f(FAKE, BUF, 2, 8, 16, 5, BUF, None, BUF, 0), "one taper without the other")
    _arg_error(f(FAKE, BUF, 2, 8, 16, 5, None, BUF, BUF, 0), "one taper without the other")
    _arg_error(f(FAKE, BUF, 2, 8, 16, 5, BUF, BUF, BUF, -1), "bad slab size")
    # an axis the in-LDS transform does not take: refused before anything is planned or launched
    _error(f(FAKE, BUF, 1, 2, 8193, 1, None, None, BUF, 0), _lib.DMM_E_UNSUPPORTED, "ra axis of length 8193")
    _error(f(FAKE, BUF, 1, 2, 4097, 1, None, None, BUF, 0), _lib.DMM_E_UNSUPPORTED, "ra axis of length 4097")
    _error(f(FAKE, BUF, 1, 4097, 4, 1, None, None, BUF, 0), _lib.DMM_E_UNSUPPORTED, "el axis of length 4097")
    with pytest.raises(_lib.DmmError):
        _lib.check(f(FAKE, BUF, 1, 8193, 4, 1, None, None, BUF, 0))


def test_cross_args():
    f = _lib.lib.dmm_ps3d_cross
    _arg_error(f(None, BUF, BUF, 2, 2, 100, 1.0, BUF), "ctx is NULL")
    _arg_error(f(FAKE, BUF, BUF, 0, 2, 100, 1.0, BUF), "bad sizes")
    _arg_error(f(FAKE, BUF, BUF, 2, -1, 100, 1.0, BUF), "bad sizes")
    _arg_error(f(FAKE, BUF, BUF, 2, 2, 0, 1.0, BUF), "bad sizes")
    _arg_error(f(FAKE, BUF, BUF, 300, 300, 100, 1.0, BUF), "bad sizes")
    _arg_error(f(FAKE, None, BUF, 2, 2, 100, 1.0, BUF), "NULL argument")
    _arg_error(f(FAKE, BUF, None, 2, 2, 100, 1.0, BUF), "NULL argument")
    _arg_error(f(FAKE, BUF, BUF, 2, 2, 100, 1.0, None), "NULL argument")
    _arg_error(f(FAKE, BUF, BUF, 1, 1, 1 << 40, 1.0, BUF), "too many cells")


def test_cyl_bin_args():
    f = _lib.lib.dmm_ps_cyl_bin
    bm = np.array([[0, 1, -1], [2, 2, 0]], dtype=np.int16)
    m = bm.ctypes.data
    _arg_error(f(None, BUF, None, m, 4, 2, 3, 3, BUF, BUF, BUF), "ctx is NULL")
    _arg_error(f(FAKE, BUF, None, m, 0, 2, 3, 3, BUF, BUF, BUF), "bad sizes")
    _arg_error(f(FAKE, BUF, None, m, 4, -2, 3, 3, BUF, BUF, BUF), "bad sizes")
    _arg_error(f(FAKE, BUF, None, m, 4, 2, 0, 3, BUF, BUF, BUF), "bad sizes")
    _arg_error(f(FAKE, BUF, None, m, 4, 65536, 65536, 3, BUF, BUF, BUF), "bad sizes")
    _arg_error(f(FAKE, BUF, None, m, 4, 2, 3, 0, BUF, BUF, BUF), "bad bin count")
    _arg_error(f(FAKE, BUF, None, m, 4, 2, 3, _lib.DMM_PS_MAX_BINS + 1, BUF, BUF, BUF), "too many bins")
    _arg_error(f(FAKE, BUF, None, m, 1 << 20, 2, 3, 4096, BUF, BUF, BUF), "too many")
    _arg_error(f(FAKE, None, None, m, 4, 2, 3, 3, BUF, BUF, BUF), "NULL argument")
    _arg_error(f(FAKE, BUF, None, None, 4, 2, 3, 3, BUF, BUF, BUF), "NULL argument")
    _arg_error(f(FAKE, BUF, None, m, 4, 2, 3, 3, None, BUF, BUF), "NULL argument")
    _arg_error(f(FAKE, BUF, None, m, 4, 2, 3, 3, BUF, None, BUF), "NULL argument")
    _arg_error(f(FAKE, BUF, None, m, 4, 2, 3, 3, BUF, BUF, None), "NULL argument")
    # a bin index outside -1 ... nbins - 1 anywhere in the map
    _arg_error(f(FAKE, BUF, None, m, 4, 2, 3, 2, BUF, BUF, BUF), "bin index 2 of cell 3")
    bad = bm.copy()
    bad[1, 2] = -2
    _arg_error(f(FAKE, BUF, None, bad.ctypes.data, 4, 2, 3, 3, BUF, BUF, BUF), "bin index -2 of cell 5")
