"""Argument validation of the RFI entry points (``csrc/rfi.hip``), on the CPU (no GPU call is reached), in the style of
``test_abi_gp.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

import ctypes as C

import numpy as np
import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)


def _arr(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, C.c_void_p(a.ctypes.data)


WIN, WIN_P = _arr([1, 2, 2], np.int32)
AXIS, AXIS_P = _arr([1, 1, 0], np.int32)
THR, THR_P = _arr([3.0, 2.5, 2.5], np.float64)
DIMS, DIMS_P = _arr([4, 3], np.int64)
STR, STR_P = _arr([8, 0], np.int64)

# name -> (a valid argument list, indices of the required buffers)
CALLS = {
    "dmm_rfi_medfilt": ([FAKE, BUF, BUF, 1, 8, 9, 3, 5, BUF], (1, 2, 8)),
    "dmm_rfi_quantile": ([FAKE, BUF, BUF, 4, 9, 0.15, BUF, None], (1, 2, 6)),
    "dmm_rfi_sumthreshold": ([FAKE, BUF, None, BUF, BUF, 8, 9, 3, WIN_P, AXIS_P, THR_P, 1, 0], (1, 3, 4, 8, 9, 10)),
    "dmm_rfi_sir": ([FAKE, BUF, 8, 9, 1, 0.2, 0, BUF, C.c_void_p(0x3000)], (1, 7, 8)),
    "dmm_rfi_absdev": ([FAKE, BUF, BUF, None, None, 72, BUF, BUF], (1, 2, 7)),
    "dmm_rfi_nsigma": ([FAKE, BUF, BUF, 1.4826, 5.0, float("nan"), 0, 72, BUF, None, None], (1, 2, 8)),
    "dmm_rfi_tv_flag": ([FAKE, BUF, 8, 9, BUF, 2, BUF, BUF, 8, BUF, 0.5, None, BUF], (1, 4, 6, 7, 9, 12)),
    "dmm_rfi_mask_op": ([FAKE, _lib.DMM_RFI_SELECT, BUF, BUF, BUF, 72, BUF], (2, 3, 4, 6)),
    "dmm_rfi_radiometer": ([FAKE, BUF, BUF, BUF, 8, 2, 9, BUF, BUF], (1, 2, 3, 7, 8)),
    "dmm_rfi_apply_mask": ([FAKE, BUF, 2, DIMS_P, 9, BUF, STR_P, 1, 9, 9, BUF, BUF], (1, 3, 5, 6, 10, 11)),
}


def _arg_error(rc, match):
    assert rc == _lib.DMM_E_ARG, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg
    with pytest.raises(ValueError, match=match):
        _lib.check(rc)


def call(name, **over):
    a = list(CALLS[name][0])
    for k, v in over.items():
        a[int(k[1:])] = v
    return getattr(_lib.lib, name)(*a)


def test_exported():
    for name in list(CALLS) + ["dmm_rfi_rows"]:
        assert name in _lib.EXPORTED
    assert (_lib.DMM_RFI_OR, _lib.DMM_RFI_SELECT) == (0, 1)
    assert (_lib.DMM_RFI_MAX_WINDOW, _lib.DMM_RFI_MAX_STRIP, _lib.DMM_RFI_MAX_ROW) == (255, 8192, 16384)
    assert _lib.lib.dmm_version() == 100


@pytest.mark.parametrize("name", list(CALLS))
def test_null_arguments(name):
    _arg_error(call(name, p0=None), "ctx is NULL")
    for i in CALLS[name][1]:
        _arg_error(call(name, **{f"p{i}": None}), "NULL argument")


def test_medfilt_sizes():
    for sf, st in ((4, 5), (3, 2), (0, 3), (-3, 3)):
        _arg_error(call("dmm_rfi_medfilt", p6=sf, p7=st), "must be odd and positive")
    for sf, st in ((257, 3), (3, 257), (255, 33), (101, 83)):
        _arg_error(call("dmm_rfi_medfilt", p6=sf, p7=st), "beyond the supported bound")
    _arg_error(call("dmm_rfi_medfilt", p3=-1), "bad sizes")
    _arg_error(call("dmm_rfi_medfilt", p4=65536), "does not fit the grid")
    assert call("dmm_rfi_medfilt", p3=0) == 0 and call("dmm_rfi_medfilt", p5=0) == 0  # nothing to do


def test_quantile_sizes():
    _arg_error(call("dmm_rfi_quantile", p4=16385), "row length 16385 outside")
    _arg_error(call("dmm_rfi_quantile", p5=1.5), "quantile 1.5 outside")
    _arg_error(call("dmm_rfi_quantile", p5=float("nan")), "quantile nan outside")
    _arg_error(call("dmm_rfi_quantile", p3=-1), "bad nrow")
    assert call("dmm_rfi_quantile", p3=0) == 0


def test_sumthreshold_steps():
    _arg_error(call("dmm_rfi_sumthreshold", p7=-1), "bad step count")
    keep, p = _arr([1, 0, 2], np.int32)
    _arg_error(call("dmm_rfi_sumthreshold", p8=p), "window 0 of step 1")
    keep, p = _arr([1, 4097, 2], np.int32)
    _arg_error(call("dmm_rfi_sumthreshold", p8=p), "window 4097 of step 1")
    keep, p = _arr([1, 2, 0], np.int32)
    _arg_error(call("dmm_rfi_sumthreshold", p9=p), "bad axis 2 of step 1")
    _arg_error(call("dmm_rfi_sumthreshold", p5=-1), "bad sizes")
    assert call("dmm_rfi_sumthreshold", p5=0) == 0


def test_other_sizes():
    _arg_error(call("dmm_rfi_sir", p4=2), "bad axis 2")
    _arg_error(call("dmm_rfi_sir", p5=float("nan")), "eta is NaN")
    _arg_error(call("dmm_rfi_sir", p8=BUF), "may not be the input")
    _arg_error(call("dmm_rfi_absdev", p3=BUF), "both or not at all")
    _arg_error(call("dmm_rfi_absdev", p5=-1), "bad count")
    _arg_error(call("dmm_rfi_nsigma", p7=-1), "bad count")
    _arg_error(call("dmm_rfi_tv_flag", p5=-1), "bad channel table sizes")
    _arg_error(call("dmm_rfi_mask_op", p1=2), "bad operation 2")
    assert call("dmm_rfi_mask_op", p1=_lib.DMM_RFI_OR, p4=None, p5=0) == 0
    _arg_error(call("dmm_rfi_radiometer", p4=40000, p5=2), "bad sizes")
    _arg_error(call("dmm_rfi_apply_mask", p2=5), "5 leading axes")
    _arg_error(call("dmm_rfi_apply_mask", p8=0), "the mask has no samples")
    assert call("dmm_rfi_apply_mask", p9=0) == 0
    _arg_error(_lib.lib.dmm_rfi_rows(None, BUF, BUF, BUF, BUF, 8, 9), "ctx is NULL")
    _arg_error(_lib.lib.dmm_rfi_rows(FAKE, None, BUF, BUF, BUF, 8, 9), "NULL argument")
    _arg_error(_lib.lib.dmm_rfi_rows(FAKE, BUF, BUF, BUF, BUF, -1, 9), "bad sizes")
