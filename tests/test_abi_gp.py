"""Argument validation of the Gaussian-process entry points (``csrc/gp.hip``), on the CPU (no GPU call is reached), in
the style of ``test_abi_dpss.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

import ctypes as C

import numpy as np
import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)


def _arr(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, C.c_void_p(a.ctypes.data)


DIMS, DIMS_P = _arr([[40, 12, 70, 0], [35, 10, 0, 0]], np.int32)
TYPES, TYPES_P = _arr([_lib.DMM_GP_MATERN25, _lib.DMM_GP_RATIONAL], np.int32)
PARAMS, PARAMS_P = _arr([[0.1, 1.0, 0.0], [0.2, 1.0, 1.5]], np.float64)

# name -> (a valid argument list, index of ngroup, index of dims, indices of the device buffers)
CALLS = {
    "dmm_gp_fill": ([FAKE, 2, TYPES_P, PARAMS_P, 1e-3, 2, DIMS_P, BUF, 40, 12, 128, BUF, BUF, BUF, BUF], 5, 6, (2, 3, 7, 11, 12, 13, 14)),
    "dmm_gp_project": ([FAKE, 2, DIMS_P, BUF, 40, 12, 128, BUF, BUF, 1e-8, BUF, BUF, BUF], 1, 2, (3, 7, 8, 10, 11, 12)),
    "dmm_gp_compact": ([FAKE, 2, DIMS_P, BUF, 40, 128, 9, BUF, BUF, BUF, BUF], 1, 2, (3, 7, 8, 9, 10)),
    "dmm_gp_apply": ([FAKE, 3, 5, 50, 32, 10, 2, DIMS_P, BUF, 40, 128, 9] + [BUF] * 9 + [None] * 4 + [BUF, BUF], 6, 7, (8, 12, 13, 14, 15, 16, 17, 18, 19, 20, 25, 26)),
}


def _arg_error(rc, match):
    assert rc == _lib.DMM_E_ARG, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg
    with pytest.raises(ValueError, match=match):
        _lib.check(rc)


def test_exported():
    for name in list(CALLS) + ["dmm_gp_masks"]:
        assert name in _lib.EXPORTED
    assert (_lib.DMM_GP_GAUSSIAN, _lib.DMM_GP_RATIONAL, _lib.DMM_GP_MATERN15, _lib.DMM_GP_MATERN25) == (0, 1, 2, 3)
    assert (_lib.DMM_GP_OK, _lib.DMM_GP_NOT_POSDEF) == (0, 1)
    assert _lib.lib.dmm_version() == 100


@pytest.mark.parametrize("name", list(CALLS))
def test_arguments(name):
    fn = getattr(_lib.lib, name)
    ok, i_g, i_dims, bufs = CALLS[name]

    def call(**over):
        a = list(ok)
        for k, v in over.items():
            a[int(k[1:])] = v
        return fn(*a)

    _arg_error(call(p0=None), "ctx is NULL")
    _arg_error(call(**{f"p{i_g}": -1}), "bad group count -1")
    _arg_error(call(**{f"p{i_g}": 65536}), "bad group count 65536")
    assert call(**{f"p{i_g}": 0}) == 0  # nothing to do
    for i in bufs + (i_dims,):
        _arg_error(call(**{f"p{i}": None}), "NULL argument")
    for bad, match in (([[41, 12, 70, 0]], "bad sizes of group 0"), ([[40, 41, 70, 0]], "bad sizes of group 0"), ([[40, 12, 129, 0]], "bad sizes of group 0"),
                       ([[40, 12, 70, 0], [0, 1, 0, 0]], "bad sizes of group 1")):
        full = bad if len(bad) == 2 else bad + [[35, 10, 0, 0]]
        keep, p = _arr(full, np.int32)
        _arg_error(call(**{f"p{i_dims}": p}), match)
        del keep


def test_sizes():
    fill, proj, comp, app = (CALLS[n][0] for n in ("dmm_gp_fill", "dmm_gp_project", "dmm_gp_compact", "dmm_gp_apply"))

    def call(name, args, **over):
        a = list(args)
        for k, v in over.items():
            a[int(k[1:])] = v
        return getattr(_lib.lib, name)(*a)

    _arg_error(call("dmm_gp_fill", fill, p8=0), "order 0 outside")
    _arg_error(call("dmm_gp_fill", fill, p9=41), "band rows 41 outside")
    _arg_error(call("dmm_gp_fill", fill, p10=100), "bad row pitch 100")
    _arg_error(call("dmm_gp_fill", fill, p1=0), "kernel count 0 outside")
    _arg_error(call("dmm_gp_fill", fill, p1=5), "kernel count 5 outside")
    _arg_error(call("dmm_gp_fill", fill, p4=float("nan")), "epsilon is NaN")
    bad_t, p = _arr([7, 0], np.int32)
    _arg_error(call("dmm_gp_fill", fill, p2=p), "bad kernel type 7")
    bad_w, p = _arr([[0.0, 1.0, 0.0], [0.2, 1.0, 1.5]], np.float64)
    _arg_error(call("dmm_gp_fill", fill, p3=p), "must be positive")
    bad_a, p = _arr([[0.1, 1.0, 0.0], [0.2, 1.0, 0.0]], np.float64)
    _arg_error(call("dmm_gp_fill", fill, p3=p), "rational scale")
    _arg_error(call("dmm_gp_project", proj, p9=-1.0), "bad tolerance")
    _arg_error(call("dmm_gp_project", proj, p6=64 * 3 + 1), "bad row pitch")
    _arg_error(call("dmm_gp_compact", comp, p6=0), "span width 0 outside")
    _arg_error(call("dmm_gp_compact", comp, p6=41), "span width 41 outside")
    _arg_error(call("dmm_gp_apply", app, p11=0), "span width 0 outside")
    _arg_error(call("dmm_gp_apply", app, p3=0), "bad sizes")
    _arg_error(call("dmm_gp_apply", app, p5=-1), "bad sizes")
    _arg_error(call("dmm_gp_apply", app, p21=BUF), "all four or not at all")
    assert call("dmm_gp_apply", app, p1=0) == 0 and call("dmm_gp_apply", app, p2=0) == 0


def test_masks():
    ok = [FAKE, BUF, 3, 5, 50, BUF, BUF, BUF]
    _arg_error(_lib.lib.dmm_gp_masks(None, *ok[1:]), "ctx is NULL")
    for i in (1, 5, 6, 7):
        a = list(ok)
        a[i] = None
        _arg_error(_lib.lib.dmm_gp_masks(*a), "NULL argument")
    a = list(ok)
    a[2] = -1
    _arg_error(_lib.lib.dmm_gp_masks(*a), "bad sizes")
    a = list(ok)
    a[3] = 0
    assert _lib.lib.dmm_gp_masks(*a) == 0
