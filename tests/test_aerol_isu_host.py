"""CPU: the ISU reassembly's entry points refuse bad arguments in the order include/jaero_hip.h gives, before any HIP call (the refusals that need
a bank -- burst, fb = 8400, never enabled -- are tests/test_gpu_aerol_isu.py's), and the row's layout is the header's."""
import ctypes as C
import os
import re

import numpy as np

from jaero_amd import acars, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_arguments_are_refused_without_a_device():
    L = capi.lib()
    n = C.c_int(7)
    buf = (C.c_ubyte * 544)()
    st = (C.c_longlong * 4)()
    off = (C.c_int * 2)()
    assert L.jaero_aerol_isu_enable(None, 4) == capi.E_INVAL and b"jaero_aerol_isu_enable" in L.jaero_last_error()
    assert L.jaero_aerol_isu_enable(None, -1) == capi.E_INVAL  # the null handle comes first
    assert L.jaero_aerol_read_msgs(None, 0, buf, 1, C.byref(n)) == capi.E_INVAL and b"jaero_aerol_read_msgs" in L.jaero_last_error()
    assert n.value == 7
    assert L.jaero_aerol_isu_stats(None, st) == capi.E_INVAL and b"jaero_aerol_isu_stats" in L.jaero_last_error()
    # jaero_aerol_read_all: the message log is a class only of a bank that enabled it; without one, 4 is refused where it always was
    assert L.jaero_aerol_read_all(None, capi.AEROL_MESSAGES, buf, 1, off, C.byref(n), None, None) == capi.E_INVAL
    assert b"what = 4" in L.jaero_last_error() and b"jaero_aerol_isu_enable" in L.jaero_last_error()
    assert L.jaero_aerol_read_all(None, capi.AEROL_MESSAGES, buf, -1, None, None, None, None) == capi.E_INVAL and b"what = 4" in L.jaero_last_error()
    assert L.jaero_aerol_read_all(None, capi.AEROL_MESSAGES + 1, buf, 1, off, C.byref(n), None, None) == capi.E_INVAL
    assert b"MESSAGES" in L.jaero_last_error() and b"none of" in L.jaero_last_error()
    assert L.jaero_aerol_profile2_read(None, 5, None, None, 0) == capi.E_INVAL
    assert L.jaero_abi_version() == 1


def test_the_row_is_the_headers_struct():
    hdr = open(os.path.join(ROOT, "include", "jaero_hip.h")).read()
    body = re.search(r"typedef struct jaero_aerol_msg\s*\{(.*?)\}\s*jaero_aerol_msg;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[.*", "", v.strip()) for decl in body.split(";") if decl.strip() for v in decl.strip().split(" ", 1)[1].split(",")]
    assert names == list(acars.MSG_DTYPE.names) == [f[0] for f in capi.Msg._fields_]
    assert C.sizeof(capi.Msg) == acars.MSG_DTYPE.itemsize == 544 and 544 % 16 == 0
    for f in acars.MSG_DTYPE.names:
        assert getattr(capi.Msg, f).offset == acars.MSG_DTYPE.fields[f][1], f
    assert int(re.search(r"#define JAERO_AEROL_MESSAGES (\d+)", hdr).group(1)) == capi.AEROL_MESSAGES == 4
    assert (capi.MSG_AES0, capi.MSG_ACARS, capi.MSG_TEXT, capi.MSG_MORE, capi.MSG_PARITY) == (
        acars.MSG_AES0, acars.MSG_ACARS, acars.MSG_TEXT, acars.MSG_MORE, acars.MSG_PARITY) == (1, 2, 4, 8, 16)
