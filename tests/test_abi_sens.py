"""Argument validation of the sensitivity entry points (``csrc/sensitivity.hip``), on the CPU (no GPU call is reached),
in the style of ``test_abi_rfi.py``: a made-up non-NULL handle is enough to drive the host-side checks.  The index tables
are host pointers and are read by the checks, so they are real arrays here."""

import ctypes as C

import numpy as np
import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)

NF, NSTACK, NT, NCOL, NPOL, NGROUP = 3, 10, 5, 4, 2, 2


def _arr(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, C.c_void_p(a.ctypes.data)


COL, COL_P = _arr([0, 1, 2, 3, 0])  # niff = 1
COL3, COL3_P = _arr([[0, 1, 2, 3, 0]] * 3)  # niff = nf
POL_PTR, POL_PTR_P = _arr([0, 2, 3])
ROWS, ROWS_P = _arr([[0, 1], [4, 2], [9, 2]])
GRP_PTR, GRP_PTR_P = _arr([0, 1, 3])
AROWS, AROWS_P = _arr([0, 3, 9])
PAIR_PTR, PAIR_PTR_P = _arr([0, 1, 3])
PAIRS, PAIRS_P = _arr([[0, 0], [0, 1], [1, 0]])

# name -> (a valid argument list, indices of the required buffers)
CALLS = {
    "dmm_sens_measured": ([FAKE, BUF, NF, NSTACK, NT, BUF, NCOL, 1, COL_P, NPOL, POL_PTR_P, ROWS_P, BUF, BUF, BUF], (1, 5, 8, 10, 11, 12, 13, 14)),
    "dmm_sens_radiometer": ([FAKE, BUF, BUF, NF, NSTACK, NT, BUF, NCOL, 1, COL_P, NGROUP, GRP_PTR_P, AROWS_P, NPOL, PAIR_PTR_P, PAIRS_P, None, 3.9e6, BUF, BUF, BUF],
                            (1, 2, 6, 9, 11, 12, 14, 15, 18, 19, 20)),
    "dmm_sens_negative_autos": ([FAKE, BUF, NF, NSTACK, NT, 3, AROWS_P, BUF, BUF], (1, 6, 7, 8)),
}
SIZES = {"dmm_sens_measured": (2, 3, 4), "dmm_sens_radiometer": (3, 4, 5), "dmm_sens_negative_autos": (2, 3, 4)}  # nf, nstack, nt


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
    for name in CALLS:
        assert name in _lib.EXPORTED
    assert _lib.DMM_SENS_MAX_GROUP == 64


@pytest.mark.parametrize("name", list(CALLS))
def test_null_arguments(name):
    _arg_error(call(name, p0=None), "ctx is NULL")
    for i in CALLS[name][1]:
        _arg_error(call(name, **{f"p{i}": None}), "NULL argument")


@pytest.mark.parametrize("name", list(CALLS))
def test_sizes(name):
    for i in SIZES[name]:
        for bad in (0, -1):
            _arg_error(call(name, **{f"p{i}": bad}), "sizes must be positive")
    _arg_error(call(name, **{f"p{SIZES[name][0]}": 65536}), "does not fit the grid")


@pytest.mark.parametrize("name,ncol,niff,col", [("dmm_sens_measured", 6, 7, 8), ("dmm_sens_radiometer", 7, 8, 9)])
def test_columns(name, ncol, niff, col):
    _arg_error(call(name, **{f"p{ncol}": 0}), "ncol must be positive")
    _arg_error(call(name, **{f"p{niff}": 2}), "niff 2 is neither 1 nor nf = 3")
    _arg_error(call(name, **{f"p{niff}": 0}), "niff 0 is neither 1 nor nf = 3")
    _arg_error(call(name, **{f"p{ncol}": 3}), "column index 3 of sample 3 outside 0 ... 2")
    keep, p = _arr([0, 1, -1, 3, 0])
    _arg_error(call(name, **{f"p{col}": p}), "column index -1 of sample 2")
    # niff = nf reads all nf rows of the table: the bad entry sits in the last one
    bad = COL3.copy()
    bad[2, 4] = 4
    keep, p = _arr(bad)
    _arg_error(call(name, **{f"p{niff}": NF, f"p{col}": p}), "column index 4 of sample 14")


def test_measured_tables():
    _arg_error(call("dmm_sens_measured", p9=0), "npol 0 outside")
    keep, p = _arr([0, 3, 2])
    _arg_error(call("dmm_sens_measured", p10=p), "pol_ptr is not monotone at entry 2")
    keep, p = _arr([1, 2, 3])
    _arg_error(call("dmm_sens_measured", p10=p), "pol_ptr does not start at 0")
    _arg_error(call("dmm_sens_measured", p3=9), "row index 9 of entry 2 outside 0 ... 8")
    keep, p = _arr([[0, 1], [-1, 2], [9, 2]])
    _arg_error(call("dmm_sens_measured", p11=p), "row index -1 of entry 1")
    keep, p = _arr([[0, 1], [4, 3], [9, 2]])
    _arg_error(call("dmm_sens_measured", p11=p), "factor 3 of entry 1 is neither 1 nor 2")


def test_radiometer_tables():
    _arg_error(call("dmm_sens_radiometer", p13=0), "npol 0 outside")
    _arg_error(call("dmm_sens_radiometer", p10=-1), "ngroup -1 outside 0 ... 64")
    _arg_error(call("dmm_sens_radiometer", p10=65), "ngroup 65 outside 0 ... 64")
    keep, p = _arr([0, 3, 1])
    _arg_error(call("dmm_sens_radiometer", p11=p), "grp_ptr is not monotone at entry 2")
    keep, p = _arr([2, 2, 3])
    _arg_error(call("dmm_sens_radiometer", p11=p), "grp_ptr does not start at 0")
    keep, p = _arr([0, 2, 1])
    _arg_error(call("dmm_sens_radiometer", p14=p), "pair_ptr is not monotone at entry 2")
    _arg_error(call("dmm_sens_radiometer", p4=9), "row index 9 of entry 2 outside 0 ... 8")
    keep, p = _arr([[0, 0], [0, 2], [1, 0]])
    _arg_error(call("dmm_sens_radiometer", p15=p), "group 2 of pair 1 outside 0 ... 1")
    keep, p = _arr([[0, 0], [0, 1], [-1, 0]])
    _arg_error(call("dmm_sens_radiometer", p15=p), "group -1 of pair 2")


def test_negative_autos_tables():
    _arg_error(call("dmm_sens_negative_autos", p5=-1), "bad row count -1")
    _arg_error(call("dmm_sens_negative_autos", p3=9), "row index 9 of entry 2 outside 0 ... 8")
    keep, p = _arr([0, -2, 9])
    _arg_error(call("dmm_sens_negative_autos", p6=p), "row index -2 of entry 1")
