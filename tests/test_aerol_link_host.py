"""CPU (no device): the entry points of the Aero-L bank's dcd link and one-call reads exist behind ABI 1, and every argument check that is
decided before a device is looked for answers JAERO_EINVAL in the order include/jaero_hip.h documents."""
import ctypes as C

import numpy as np
import pytest

from jaero_amd import capi


@pytest.fixture(scope="module")
def L():
    return capi.lib()


def test_symbols_and_abi(L):
    for name in ("jaero_aerol_link_dcd", "jaero_aerol_read_all", "jaero_aerol_profile2_read", "jaero_aerol_debug_extra_bytes"):
        assert name in capi.EXPORTS and getattr(L, name)
    assert L.jaero_abi_version() == 1
    assert (capi.AEROL_SUS, capi.AEROL_PACKETS, capi.AEROL_EVENTS, capi.AEROL_VOICE) == (0, 1, 2, 3)


def read_all(L, ctx=None, what=0, rows=True, caprows=4, offsets=True, taken=True):
    buf = np.zeros((8, 16), np.int32)
    off = np.zeros(8, np.int32)
    n = C.c_int(-7)
    rc = L.jaero_aerol_read_all(ctx, what, buf.ctypes.data if rows else None, caprows, off.ctypes.data if offsets else None,
                                C.byref(n) if taken else None, None, None)
    return rc, L.jaero_last_error()


# the documented order: what, caprows, offsets / nchannels_taken, rows, ctx
FAULTS = [(dict(what=4), b"what"), (dict(caprows=-1), b"caprows < 0"), (dict(offsets=False), b"null offsets"), (dict(taken=False), b"null offsets"),
          (dict(rows=False), b"null rows"), (dict(), b"null ctx")]


@pytest.mark.parametrize("kw,word", FAULTS)
def test_read_all_einval_each(L, kw, word):
    rc, msg = read_all(L, **kw)
    assert rc == capi.E_INVAL and b"jaero_aerol_read_all" in msg and word in msg, msg


def test_read_all_null_rows_is_fine_for_the_sizing_call(L):
    rc, msg = read_all(L, rows=False, caprows=0)
    assert rc == capi.E_INVAL and b"null ctx" in msg  # the only fault left


def test_read_all_what_below_range(L):
    rc, msg = read_all(L, what=-1)
    assert rc == capi.E_INVAL and b"what" in msg


@pytest.mark.parametrize("i", range(len(FAULTS) - 1))
def test_read_all_two_faults_report_the_earlier(L, i):
    for j in range(i + 1, len(FAULTS)):
        kw = dict(FAULTS[j][0])
        kw.update(FAULTS[i][0])
        rc, msg = read_all(L, **kw)
        assert rc == capi.E_INVAL and FAULTS[i][1] in msg, (i, j, msg)


def test_link_null_ctx(L):
    assert L.jaero_aerol_link_dcd(None, None) == capi.E_INVAL and b"jaero_aerol_link_dcd: null ctx" in L.jaero_last_error()
    # null ctx comes first: a bank argument that could not be looked at without faulting is never looked at
    assert L.jaero_aerol_link_dcd(None, C.c_void_p(0)) == capi.E_INVAL and b"null ctx" in L.jaero_last_error()


def test_profile2_null_ctx_and_range(L):
    ms, n = C.c_double(0), C.c_int(0)
    assert L.jaero_aerol_profile2_read(None, 3, C.byref(ms), C.byref(n), 0) == capi.E_INVAL
    assert b"jaero_aerol_profile2_read" in L.jaero_last_error()
    # the older entry point keeps its own range
    assert L.jaero_aerol_profile_read(None, 3, C.byref(ms), C.byref(n), 0) == capi.E_INVAL
