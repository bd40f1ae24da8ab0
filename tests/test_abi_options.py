"""Reading options back through ``dmm_ctx_get_counter("opt_<name>")``: the argument checks, on the CPU.

As in ``test_abi_args.py`` a made-up handle is enough: the name is looked up before the context is touched.
"""

import ctypes as C

import pytest

from draco_amd import _lib

FAKE = C.c_void_p(0x1000)  # never dereferenced: every call below must fail its checks first


def _arg_error(rc, match):
    assert rc == _lib.DMM_E_ARG, rc
    msg = _lib.lib.dmm_last_error().decode()
    assert match in msg, msg
    with pytest.raises(ValueError, match=match):
        _lib.check(rc)


def test_an_unknown_option_is_not_an_unknown_counter():
    lib = _lib.lib
    v = C.c_int64()
    _arg_error(lib.dmm_ctx_get_counter(FAKE, b"opt_no_such", C.byref(v)), "unknown option 'no_such'")
    _arg_error(lib.dmm_ctx_get_counter(FAKE, b"opt_", C.byref(v)), "unknown option ''")
    _arg_error(lib.dmm_ctx_get_counter(FAKE, b"no_such_counter", C.byref(v)), "unknown counter 'no_such_counter'")
    _arg_error(lib.dmm_ctx_get_counter(FAKE, b"prof_no_such_us", C.byref(v)), "unknown counter")
    _arg_error(lib.dmm_ctx_set_option(FAKE, b"opt_ml_eigen", 1), "unknown option 'opt_ml_eigen'")  # the prefix is the read path's alone


def test_null_arguments_of_the_read_path():
    lib = _lib.lib
    v = C.c_int64()
    _arg_error(lib.dmm_ctx_get_counter(None, b"opt_ml_eigen", C.byref(v)), "NULL argument")
    _arg_error(lib.dmm_ctx_get_counter(FAKE, None, C.byref(v)), "NULL argument")
    _arg_error(lib.dmm_ctx_get_counter(FAKE, b"opt_ml_eigen", None), "NULL argument")
    _arg_error(lib.dmm_ctx_set_option(FAKE, None, 1), "NULL argument")
