"""CPU: the device code of the ISU reassembly (jaero_amd/csrc/k_aerol_isu.h) compiled for the host and run thread by thread behind the
emulated bit pipeline, in the rounds of jaero_aerol_write (tests/host_emul/aerol_isu_emul.cpp), against the definition as
tests/isu_oracle.py states it: message rows, counters and the untouched signal-unit and event rows, for every case of tests/isu_cases.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import isu_cases as IC
import isu_oracle as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def E(oracle_mod):
    oracle_mod.lib()
    td = tempfile.mkdtemp(prefix="aerol_isu_emul_")
    so = os.path.join(td, "libaerol_isu_emul.so")
    cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tests", "host_emul", "stub"), "-o", so,
           os.path.join(ROOT, "tests", "host_emul", "aerol_isu_emul.cpp"), "-L" + os.path.join(ROOT, "oracle"), "-l:liboracle.so",
           "-Wl,-rpath," + os.path.join(ROOT, "oracle")]
    subprocess.check_call(cmd)
    L = C.CDLL(so)
    L.emuli_create.restype = C.c_void_p
    L.emuli_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.emuli_destroy.argtypes = [C.c_void_p]
    L.emuli_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.emuli_read.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.emuli_overflow.argtypes = [C.c_void_p, C.c_int]
    L.emuli_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return L


def feed(E, h, streams, width, rng):
    nch = len(streams)
    pos = np.zeros(nch, dtype=np.int64)
    lens = np.array([len(s) for s in streams])
    while (pos < lens).any():
        cnt = np.minimum(rng.integers(1, width, size=nch), lens - pos).astype(np.int32)
        buf = np.zeros((nch, width), np.int16)
        for c in range(nch):
            buf[c, :cnt[c]] = streams[c][pos[c]:pos[c] + cnt[c]]
        assert E.emuli_write(h, buf.ctypes.data, cnt.ctypes.data, width, int(cnt.max())) == 0
        pos += cnt


@pytest.mark.parametrize("fb,nch,width", [(1200, 9, 6000), (1200, 8, 700), (600, 8, 2500), (10500, 8, 6000)])
def test_rows_and_counters_equal_the_definition(E, oracle_mod, fb, nch, width):
    """Every script, ragged per-channel counts in every write (width 700: less than a block per write)."""
    plan = IC.channel_plan(nch, fb)
    streams = [IC.stream(name, fb, inv, lead) for name, inv, lead in plan]
    h = E.emuli_create(nch, fb, 500, 16)
    feed(E, h, streams, width, np.random.default_rng(fb + width))
    total = 0
    for c, (name, inv, lead) in enumerate(plan):
        msgs, stats, missing, sus, ev = IC.expected(oracle_mod, name, fb, inv, lead)
        got = np.zeros(16, dtype=IO.MSG)
        n = E.emuli_read(h, c, 2, got.ctypes.data, 16)
        st = np.zeros(4, np.int64)
        E.emuli_stats(h, c, st.ctypes.data)
        assert E.emuli_overflow(h, c) == 0
        assert n == len(msgs) and got[:n].tobytes() == msgs.tobytes(), (c, name)
        assert np.array_equal(st, stats), (c, name, st, stats)
        gs = np.zeros((600, 16), np.int32)
        ns = E.emuli_read(h, c, 0, gs.ctypes.data, 600)
        ge = np.zeros((256, 3), np.int64)
        ne = E.emuli_read(h, c, 1, ge.ctypes.data, 256)
        assert np.array_equal(gs[:ns], sus) and np.array_equal(ge[:ne], ev), (c, name)
        total += n
    assert total >= 20
    E.emuli_destroy(h)


def test_a_full_log_drops_rows_and_keeps_counting(E, oracle_mod):
    """Capacity 3 where a channel completes 12: the first three rows, the messages' overflow bit (8), all twelve counted."""
    fb = 1200
    h = E.emuli_create(1, fb, 500, 3)
    feed(E, h, [IC.stream("sizes", fb)], 6000, np.random.default_rng(1))
    msgs, stats, _, _, _ = IC.expected(oracle_mod, "sizes", fb)
    got = np.zeros(8, dtype=IO.MSG)
    assert E.emuli_read(h, 0, 2, got.ctypes.data, 8) == 3 and got[:3].tobytes() == msgs[:3].tobytes()
    assert E.emuli_overflow(h, 0) == 8
    st = np.zeros(4, np.int64)
    E.emuli_stats(h, 0, st.ctypes.data)
    assert np.array_equal(st, stats) and st[3] == 12
    E.emuli_destroy(h)
