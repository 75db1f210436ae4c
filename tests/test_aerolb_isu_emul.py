"""CPU: the device code of the burst bank's R / T reassembly (jaero_amd/csrc/k_aerolb_isu.h) compiled for the host and run thread by thread
behind the emulated packet search, in the rounds of jaero_aerol_write (tests/host_emul/aerolb_isu_emul.cpp), against the definition as
tests/rt_isu_oracle.py states it: message rows, all eight counters and the untouched packet and event rows, for every case of
tests/rt_isu_cases.py at the three rates."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import rt_isu_cases as RC
import rt_isu_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def E(oracle_mod):
    oracle_mod.lib()
    td = tempfile.mkdtemp(prefix="aerolb_isu_emul_")
    so = os.path.join(td, "libaerolb_isu_emul.so")
    cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "tests", "host_emul", "stub"), "-o", so,
           os.path.join(ROOT, "tests", "host_emul", "aerolb_isu_emul.cpp"), "-L" + os.path.join(ROOT, "oracle"), "-l:liboracle.so",
           "-Wl,-rpath," + os.path.join(ROOT, "oracle")]
    subprocess.check_call(cmd)
    L = C.CDLL(so)
    L.emulr_create.restype = C.c_void_p
    L.emulr_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.emulr_destroy.argtypes = [C.c_void_p]
    L.emulr_write.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.emulr_read.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.emulr_overflow.argtypes = [C.c_void_p, C.c_int]
    L.emulr_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return L


def feed(E, h, streams, width, rng):
    """Ragged per-channel counts in every write, from rows whose base is 16-byte aligned."""
    nch = len(streams)
    pos = np.zeros(nch, dtype=np.int64)
    lens = np.array([len(s) for s in streams])
    raw = np.zeros(nch * width + 8, np.int16)
    off = (-raw.ctypes.data % 16) // 2
    buf = raw[off:off + nch * width].reshape(nch, width)
    while (pos < lens).any():
        cnt = np.minimum(rng.integers(1, width + 1, size=nch), lens - pos).astype(np.int32)
        buf[:] = 0
        for c in range(nch):
            buf[c, :cnt[c]] = streams[c][pos[c]:pos[c] + cnt[c]]
        assert E.emulr_write(h, buf.ctypes.data, cnt.ctypes.data, width, int(cnt.max())) == 0
        pos += cnt


@pytest.mark.parametrize("fb,width", [(10500, 3000), (10500, 2996), (1200, 2504), (600, 2500)])
def test_rows_and_counters_equal_the_definition(E, oracle_mod, fb, width):
    """Every case and a noise-only channel; width 2996: rows that are not 16-byte aligned (the bit walk's other path)."""
    plan = RC.channel_plan(len(RC.NAMES) + 1, fb, noise_every=len(RC.NAMES) + 1)
    streams = [RC.stream(name, fb, inv) for name, inv in plan]
    h = E.emulr_create(len(plan), fb, 700, 64)
    feed(E, h, streams, width, np.random.default_rng(fb + width))
    total = 0
    for c, (name, inv) in enumerate(plan):
        msgs, stats, missing, pk, ev, _ = RC.expected(oracle_mod, name, fb, inv)
        got = np.zeros(64, dtype=RO.MSG)
        n = E.emulr_read(h, c, 2, got.ctypes.data, 64)
        st = np.zeros(8, np.int64)
        E.emulr_stats(h, c, st.ctypes.data)
        assert E.emulr_overflow(h, c) == 0
        assert np.array_equal(st, stats), (c, name, st, stats)
        assert n == len(msgs) and got[:n].tobytes() == msgs.tobytes(), (c, name)
        gs = np.zeros((700, 16), np.int32)
        ns = E.emulr_read(h, c, 0, gs.ctypes.data, 700)
        ge = np.zeros((256, 3), np.int64)
        ne = E.emulr_read(h, c, 1, ge.ctypes.data, 256)
        assert np.array_equal(gs[:ns], pk) and np.array_equal(ge[:ne], ev), (c, name)
        total += n
    assert total >= 40
    E.emulr_destroy(h)


def test_a_full_log_drops_rows_and_keeps_counting(E, oracle_mod):
    """Capacity 3 where a channel completes more: the first three rows, the messages' overflow bit (8), all counted."""
    fb = 10500
    h = E.emulr_create(1, fb, 700, 3)
    feed(E, h, [RC.stream("r_sizes", fb)], 3000, np.random.default_rng(1))
    msgs, stats, _, _, _, _ = RC.expected(oracle_mod, "r_sizes", fb)
    assert len(msgs) > 3
    got = np.zeros(8, dtype=RO.MSG)
    assert E.emulr_read(h, 0, 2, got.ctypes.data, 8) == 3 and got[:3].tobytes() == msgs[:3].tobytes()
    assert E.emulr_overflow(h, 0) == 8
    st = np.zeros(8, np.int64)
    E.emulr_stats(h, 0, st.ctypes.data)
    assert np.array_equal(st, stats) and st[6] == len(msgs)
    E.emulr_destroy(h)


def test_a_packet_log_without_room_loses_no_message(E, oracle_mod):
    """su_capacity 2: the packet rows overflow (bit 1), every message still completes."""
    fb = 10500
    h = E.emulr_create(1, fb, 2, 64)
    feed(E, h, [RC.stream("mixed", fb)], 3000, np.random.default_rng(2))
    msgs, stats, _, _, _, _ = RC.expected(oracle_mod, "mixed", fb)
    got = np.zeros(64, dtype=RO.MSG)
    n = E.emulr_read(h, 0, 2, got.ctypes.data, 64)
    assert n == len(msgs) and got[:n].tobytes() == msgs.tobytes()
    assert E.emulr_overflow(h, 0) == 1
    E.emulr_destroy(h)
