"""Argument validation of the DPSS entry points, on the CPU (no GPU call is reached), in the style of
``test_abi_mfilter.py``: a made-up non-NULL handle is enough to drive the host-side checks."""

import ctypes as C

import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first
BUF = C.c_void_p(0x2000)
LAY = (C.c_int64 * 4)(5, 0, 1, 5)
BAD_LAY = (C.c_int64 * 4)(0, 0, 1, 5)

# name -> (a valid argument list, index of n, index of k or None, index of nb, nb bounded by 65535, nullable indices)
CALLS = {
    "dmm_dpss_pack": ([FAKE, 64, 3, LAY, BUF, BUF, BUF, None, BUF, BUF, BUF, BUF, BUF], 1, None, 2, True, (7,)),
    "dmm_dpss_gram": ([FAKE, 64, 20, 3, BUF, BUF, 1e-3, BUF, BUF], 1, 2, 3, True, ()),
    "dmm_dpss_project": ([FAKE, 64, 20, 3, BUF, BUF, BUF, BUF, BUF], 1, 2, 3, True, ()),
    "dmm_dpss_solve": ([FAKE, 20, 3, BUF, BUF, BUF], 1, None, 2, True, ()),
    "dmm_dpss_variance": ([FAKE, 64, 20, 3, BUF, BUF, 1e-3, BUF, BUF, BUF], 1, 2, 3, True, ()),
    "dmm_dpss_synth": ([FAKE, 64, 20, 3, BUF, BUF, BUF], 1, 2, 3, True, ()),
    "dmm_dpss_gapflag": ([FAKE, 64, 3, BUF, 2.5, BUF], 1, None, 2, False, ()),
    "dmm_dpss_pchip": ([FAKE, 64, 3, BUF, BUF, BUF, BUF, BUF], 1, None, 2, False, ()),
    "dmm_dpss_store": ([FAKE, 64, 3, LAY, BUF, BUF, BUF, BUF, BUF, BUF, BUF, None, BUF, 1, BUF, BUF], 1, None, 2, True, (11,)),
}


def _arg_error(rc, match):
    assert rc == _lib.DMM_E_ARG, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg
    with pytest.raises(ValueError, match=match):
        _lib.check(rc)


def test_exported():
    for name in CALLS:
        assert name in _lib.EXPORTED
    assert (_lib.DMM_DPSS_OK, _lib.DMM_DPSS_SKIPPED, _lib.DMM_DPSS_NOT_POSDEF) == (0, 1, 2)


@pytest.mark.parametrize("name", list(CALLS))
def test_arguments(name):
    fn = getattr(_lib.lib, name)
    ok, i_n, i_k, i_nb, bounded, nullable = CALLS[name]

    def call(**over):
        a = list(ok)
        for k, v in over.items():
            a[int(k[1:])] = v
        return fn(*a)

    _arg_error(call(p0=None), "ctx is NULL")
    _arg_error(call(**{f"p{i_n}": 0}), "order 0 outside")
    _arg_error(call(**{f"p{i_n}": 4097}), "order 4097 outside")
    if i_k is not None:
        _arg_error(call(**{f"p{i_k}": 0}), "mode count 0 outside")
        _arg_error(call(**{f"p{i_k}": 65}), "mode count 65 outside")
    _arg_error(call(**{f"p{i_nb}": -1}), "bad column count -1")
    if bounded:
        _arg_error(call(**{f"p{i_nb}": 65536}), "bad column count 65536")
    for i, v in enumerate(ok):
        if i and (v is BUF or v is LAY) and i not in nullable:
            _arg_error(call(**{f"p{i}": None}), "NULL argument")
    assert call(**{f"p{i_nb}": 0}) == 0  # nothing to do


@pytest.mark.parametrize("name", ["dmm_dpss_pack", "dmm_dpss_store"])
def test_layout(name):
    a = list(CALLS[name][0])
    a[3] = BAD_LAY
    _arg_error(getattr(_lib.lib, name)(*a), "bad layout")


def test_gapflag_nan():
    _arg_error(_lib.lib.dmm_dpss_gapflag(FAKE, 64, 3, BUF, float("nan"), BUF), "cutoff is NaN")
