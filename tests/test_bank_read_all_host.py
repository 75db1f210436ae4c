"""CPU (no device): the demodulator bank's one-call reads (jaero_read_all, jaero_read_status_all, jaero_profile2_read and their two test hooks)
exist behind ABI 1, and every argument check that is decided before a device is looked for answers JAERO_EINVAL in the order
include/jaero_hip.h documents."""
import ctypes as C

import numpy as np
import pytest

from jaero_amd import capi

NEW = ("jaero_read_all", "jaero_read_status_all", "jaero_profile2_read", "jaero_debug_read_all_bytes", "jaero_debug_softbit_counts")


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def test_symbols_and_abi(L):
    for name in NEW:
        assert name in capi.EXPORTS and getattr(L, name)
    assert L.jaero_abi_version() == 1
    assert (capi.BANK_SOFTBITS, capi.BANK_STATUS_LOG, capi.BANK_EVENTS, capi.BANK_SYMBOLS) == (0, 1, 2, 3)


def read_all(L, ctx=None, what=0, rows=True, caprows=4, offsets=True, taken=True):
    buf = np.zeros((8, 6), np.float64)
    off = np.zeros(8, np.int32)
    n = C.c_int(-7)
    rc = L.jaero_read_all(ctx, what, buf.ctypes.data if rows else None, caprows, off.ctypes.data if offsets else None,
                          C.byref(n) if taken else None, None, None)
    assert n.value == -7  # nothing is written on a refusal
    return rc, L.jaero_last_error()


# the documented order: what, caprows, offsets / nchannels_taken, rows, ctx
FAULTS = [(dict(what=4), b"what"), (dict(caprows=-1), b"caprows < 0"), (dict(offsets=False), b"null offsets"), (dict(taken=False), b"null offsets"),
          (dict(rows=False), b"null rows"), (dict(), b"null ctx")]


@pytest.mark.parametrize("kw,word", FAULTS)
def test_read_all_einval_each(L, kw, word):
    rc, msg = read_all(L, **kw)
    assert rc == capi.E_INVAL and b"jaero_read_all" in msg and word in msg, msg


def test_read_all_null_rows_is_fine_for_the_sizing_call(L):
    rc, msg = read_all(L, rows=False, caprows=0)
    assert rc == capi.E_INVAL and b"jaero_read_all" in msg and b"null ctx" in msg  # the only fault left


def test_read_all_what_below_range(L):
    rc, msg = read_all(L, what=-1)
    assert rc == capi.E_INVAL and b"what" in msg


@pytest.mark.parametrize("i", range(len(FAULTS) - 1))
def test_read_all_two_faults_report_the_earlier(L, i):
    for j in range(i + 1, len(FAULTS)):
        kw = dict(FAULTS[j][0])
        kw.update(FAULTS[i][0])
        rc, msg = read_all(L, **kw)
        assert rc == capi.E_INVAL and b"jaero_read_all" in msg and FAULTS[i][1] in msg, (i, j, msg)


def test_status_all_null_arguments(L):
    st = (capi.Status * 2)()
    assert L.jaero_read_status_all(None, C.addressof(st)) == capi.E_INVAL
    assert b"jaero_read_status_all" in L.jaero_last_error()
    assert np.dtype(capi.Status).itemsize == C.sizeof(capi.Status) == 40


def test_profile2_null_ctx_and_range(L):
    ms, n = C.c_double(0), C.c_int(0)
    assert L.jaero_profile2_read(None, 5, C.byref(ms), C.byref(n), 0) == capi.E_INVAL
    assert b"jaero_profile2_read" in L.jaero_last_error()
    assert L.jaero_profile2_read(None, 6, C.byref(ms), C.byref(n), 0) == capi.E_INVAL
    # the older entry point keeps its own range
    assert L.jaero_profile_read(None, 5, C.byref(ms), C.byref(n), 0) == capi.E_INVAL
    assert b"jaero_profile_read" in L.jaero_last_error()


def test_debug_hooks_null_ctx(L):
    assert L.jaero_debug_read_all_bytes(None) == -1
    cnt = np.zeros(4, np.int32)
    assert L.jaero_debug_softbit_counts(None, cnt.ctypes.data, cnt.ctypes.data) == capi.E_INVAL
    assert b"jaero_debug_softbit_counts" in L.jaero_last_error()
