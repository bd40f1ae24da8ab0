"""Argument validation of the entry points of ``csrc/vismask.hip``, on the CPU (no GPU call is reached), in the style of
``test_abi_rfi.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

import ctypes as C

import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)
OUT = C.c_void_p(0x3000)
SWEEPS = C.c_int32(-1)

# name -> (a valid argument list, indices of the required buffers)
CALLS = {
    "dmm_stokes_i_sum": ([FAKE, BUF, BUF, 6, 43, 160, BUF, BUF, 11, 20, OUT, OUT], (1, 2, 6, 7, 10, 11)),
    "dmm_wconv_filter": ([FAKE, _lib.DMM_REDUCE_C64, BUF, BUF, 66, 160, BUF, 31, 1, OUT], (2, 3, 6, 9)),
    "dmm_beam_abs_fft": ([FAKE, BUF, 6, 11, 160, OUT], (1, 5)),
    "dmm_rfi_hysteresis": ([FAKE, BUF, 6, 11, 160, 2.0, 8.0, 1, BUF, BUF, OUT, C.byref(SWEEPS)], (1, 8, 9, 10)),
    "dmm_rfi_beam_count": ([FAKE, BUF, 6, 11, 160, OUT], (1, 5)),
}


def _error(rc, code, match):
    assert rc == code, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg


def _arg_error(rc, match):
    _error(rc, _lib.DMM_E_ARG, match)
    with pytest.raises(ValueError, match=match):
        _lib.check(rc)


def call(name, **over):
    a = list(CALLS[name][0])
    for k, v in over.items():
        a[int(k[1:])] = v
    return getattr(_lib.lib, name)(*a)


def test_exported():
    for name in list(CALLS) + ["dmm_beam_abs_fft_supported"]:
        assert name in _lib.EXPORTED
    assert (_lib.DMM_WCONV_MAX_TAPS, _lib.DMM_RFI_HYST_MAX_SWEEPS) == (1023, 4096)


@pytest.mark.parametrize("name", list(CALLS))
def test_null_arguments(name):
    _arg_error(call(name, p0=None), "ctx is NULL")
    for i in CALLS[name][1]:
        _arg_error(call(name, **{f"p{i}": None}), "NULL argument")


def test_sizes_below_one():
    for i in (3, 4, 5, 8):
        _arg_error(call("dmm_stokes_i_sum", **{f"p{i}": 0}), "bad sizes")
    _arg_error(call("dmm_stokes_i_sum", p9=-1), "bad sizes")
    _arg_error(call("dmm_stokes_i_sum", p8=65536), "does not fit the grid")
    assert SWEEPS.value == -1
    for i in (4, 5):
        _arg_error(call("dmm_wconv_filter", **{f"p{i}": 0}), "bad sizes")
    for name in ("dmm_beam_abs_fft", "dmm_rfi_hysteresis", "dmm_rfi_beam_count"):
        for i in (2, 3, 4):
            _arg_error(call(name, **{f"p{i}": 0}), "bad sizes")
            _arg_error(call(name, **{f"p{i}": -3}), "bad sizes")


def test_filter_taps_and_types():
    for ntap in (30, 2, 0, -1):
        _arg_error(call("dmm_wconv_filter", p7=ntap), "must be odd and positive")
    _arg_error(call("dmm_wconv_filter", p7=_lib.DMM_WCONV_MAX_TAPS + 2), "beyond the supported bound of 1023")
    _arg_error(call("dmm_wconv_filter", p1=_lib.DMM_REDUCE_F32), "bad data type")
    _arg_error(call("dmm_wconv_filter", p1=7), "bad data type")
    _arg_error(call("dmm_wconv_filter", p9=BUF), "may not be the input")


def test_transform_lengths():
    ok = [n for n in range(1, 8300) if _lib.lib.dmm_beam_abs_fft_supported(n)]
    assert ok == list(range(1, 4097)) + [8192]
    assert not _lib.lib.dmm_beam_abs_fft_supported(0) and not _lib.lib.dmm_beam_abs_fft_supported(16384)
    for n in (4097, 8191, 16384):
        _error(call("dmm_beam_abs_fft", p3=n), _lib.DMM_E_UNSUPPORTED, f"length {n} does not fit")
        with pytest.raises(_lib.DmmError, match="does not fit"):
            _lib.check(_lib.DMM_E_UNSUPPORTED)
    _arg_error(call("dmm_beam_abs_fft", p5=BUF), "may not be the input")


def test_hysteresis_thresholds():
    _arg_error(call("dmm_rfi_hysteresis", p5=float("nan")), "a threshold is NaN")
    _arg_error(call("dmm_rfi_hysteresis", p6=float("nan")), "a threshold is NaN")
    _arg_error(call("dmm_rfi_hysteresis", p2=65536), "bad sizes")
    _arg_error(call("dmm_rfi_hysteresis", p10=BUF), "may not be the output")
