"""CPU: the burst bank's reassembly entry points exist, the ABI is still 1, and they refuse bad arguments in the order include/jaero_hip.h gives,
before any HIP call (the refusals that need a bank -- a P bank, fb = 8400, never enabled -- are tests/test_gpu_aerol_rt.py's)."""
import ctypes as C
import os
import re

from jaero_amd import acars, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbols_exist_and_the_abi_is_1():
    L = capi.lib()
    assert {"jaero_aerol_rt_enable", "jaero_aerol_rt_stats"} <= set(capi.EXPORTS)
    assert L.jaero_aerol_rt_enable and L.jaero_aerol_rt_stats
    assert L.jaero_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "jaero_hip.h")).read()
    assert re.search(r"int jaero_aerol_rt_enable\(jaero_aerol_ctx \*ctx, int msg_capacity\);", hdr)
    assert re.search(r"int jaero_aerol_rt_stats\(jaero_aerol_ctx \*ctx, long long \*stats /\* \[nchannels\]\[8\] \*/\);", hdr)
    assert "is\n * deliberately not here" not in hdr and "deliberately not in this change" not in hdr  # the R / T path is no longer missing
    assert (acars.MSG_RCHAN, acars.MSG_RSIGNAL) == (32, 64)


def test_null_arguments_are_refused_without_a_device():
    L = capi.lib()
    st = (C.c_longlong * 8)()
    assert L.jaero_aerol_rt_enable(None, 4) == capi.E_INVAL and b"jaero_aerol_rt_enable" in L.jaero_last_error() and b"null ctx" in L.jaero_last_error()
    assert L.jaero_aerol_rt_enable(None, -1) == capi.E_INVAL and b"null ctx" in L.jaero_last_error()  # the null handle comes first
    assert L.jaero_aerol_rt_enable(None, 0) == capi.E_INVAL
    assert L.jaero_aerol_rt_stats(None, st) == capi.E_INVAL and b"jaero_aerol_rt_stats" in L.jaero_last_error()
    assert L.jaero_aerol_rt_stats(None, None) == capi.E_INVAL
    # the message class of jaero_aerol_read_all still needs a bank that enabled a reassembly: the first check refuses it, and names both calls
    n, off, buf = C.c_int(7), (C.c_int * 2)(), (C.c_ubyte * 544)()
    assert L.jaero_aerol_read_all(None, capi.AEROL_MESSAGES, buf, 1, off, C.byref(n), None, None) == capi.E_INVAL
    assert b"what = 4" in L.jaero_last_error() and b"jaero_aerol_rt_enable" in L.jaero_last_error() and n.value == 7
