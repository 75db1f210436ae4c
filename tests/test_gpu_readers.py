"""GPU (-m gpu): the eight per-channel readers of the C ABI share one drain and one argument rule.  For every reader on every bank kind that
has it: a drain in pieces of a few rows hands over, in order, exactly what one full drain of an identically fed twin bank hands over, and
caprows < 0 or a null row buffer is refused with JAERO_EINVAL before anything is copied (the rows stay readable).  Also: the kernel timings
of a bank survive a rate-changing jaero_set_settings, and the Aero-L timer counts launches in all three kernel classes."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from jaero_amd import aerol_frames as AF
from jaero_amd import signalgen as G

pytestmark = pytest.mark.gpu

CH = {"pieces": 0, "negcap": 1, "nullrows": 2}  # one channel of the twin banks per case: the cases do not drain each other's rows


def _make_golden():
    spec = importlib.util.spec_from_file_location("mk", os.path.join(os.path.dirname(__file__), "golden", "make_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


def _feed_demod(bank, pcm, chunk):
    for s in range(0, pcm.shape[1], chunk):
        bank.write(pcm[:, s:s + chunk])


def _feed_aerol(bank, soft, width):
    n = max(len(x) for x in soft)
    for s in range(0, n, width):
        buf = np.zeros((len(soft), width), np.int16)
        cnt = np.zeros(len(soft), np.int32)
        for c, x in enumerate(soft):
            part = x[s:s + width]
            buf[c, :len(part)] = part
            cnt[c] = len(part)
        bank.write(buf, counts=cnt)


def _cont():
    from jaero_amd import demodulator as D
    pcm = np.stack([G.oqpsk(40000, seed=G.SEED_BASE + 900 + c)[0] for c in range(3)])
    b = D.DemodulatorBank(D.OqpskSettings(), 3, status_log=True, capture_symbols=True, max_write_samples=8192, softbit_capacity=40000)
    _feed_demod(b, pcm, 8192)
    return b


def _burst():
    from jaero_amd import demodulator as D
    n = 48000 * 3
    pcm = np.stack([G.burst_msk(n, burst_starts=[30000 + 5000 * c], fc=1900.0, ebno_db=18.0, seed=G.SEED_BASE + 910 + c)[0] for c in range(3)])
    b = D.DemodulatorBank(D.BurstMskSettings(freq_center=1900.0, fb=1200.0, lockingbw=1800.0), 3, capture_symbols=True, trace=True,
                          max_write_samples=8192, softbit_capacity=30000)
    _feed_demod(b, pcm, 7000)
    return b


def _aerolp():
    from jaero_amd import demodulator as D
    soft = []
    for c in range(3):
        bits, _ = AF.p_channel_bits(AF.random_payloads(4, 10500, seed=920 + c), 10500)
        soft.append(AF.to_soft(bits, sigma=20.0, seed=c))
    b = D.AeroLBank(3, 10500, max_softbits_per_write=6000, su_capacity=400)
    _feed_aerol(b, soft, 6000)
    return b


def _aerolrt():
    from jaero_amd import demodulator as D
    mk = _make_golden()
    soft = [mk.rt_case(930 + c, 20.0)[1] for c in range(3)]
    b = D.AeroLBank(3, 10500, max_softbits_per_write=3000, su_capacity=700, burst=True)
    _feed_aerol(b, soft, 3000)
    return b


def _aerolc():
    from jaero_amd import demodulator as D
    soft = [AF.c_channel_case(940 + c, 4, 20.0, lead=100 + 30 * c)[1] for c in range(3)]
    b = D.AeroLBank(3, 8400, max_softbits_per_write=4096)
    _feed_aerol(b, soft, 4096)
    return b


BANKS = {"cont": _cont, "burst": _burst, "aerolp": _aerolp, "aerolrt": _aerolrt, "aerolc": _aerolc}
# reader id -> (bank kind, C function, row width, row dtype)
READERS = {
    "cont_softbits": ("cont", "jaero_read_softbits", 1, np.int16),
    "cont_status_log": ("cont", "jaero_read_status_log", 6, np.float64),
    "cont_symbols": ("cont", "jaero_read_symbols", 3, np.float64),
    "burst_softbits": ("burst", "jaero_read_softbits", 1, np.int16),
    "burst_symbols": ("burst", "jaero_read_symbols", 3, np.float64),
    "burst_events": ("burst", "jaero_read_events", 3, np.float64),
    "aerolp_sus": ("aerolp", "jaero_aerol_read_sus", 16, np.int32),
    "aerolp_events": ("aerolp", "jaero_aerol_read_events", 3, np.int64),
    "aerolrt_packets": ("aerolrt", "jaero_aerol_read_packets", 16, np.int32),
    "aerolrt_events": ("aerolrt", "jaero_aerol_read_events", 3, np.int64),
    "aerolc_sus": ("aerolc", "jaero_aerol_read_sus", 16, np.int32),
    "aerolc_events": ("aerolc", "jaero_aerol_read_events", 3, np.int64),
    "aerolc_voice": ("aerolc", "jaero_aerol_read_voice", 304, np.uint8),
}


@pytest.fixture(scope="module")
def twins():
    from jaero_amd import capi
    capi.lib()
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = (BANKS[kind](), BANKS[kind]())
        return made[kind]

    yield get
    for a, b in made.values():
        a.close()
        b.close()


def _read(bank, fn, ch, width, dtype, cap, null_rows=False):
    buf = np.empty((max(cap, 1), width), dtype)
    n = C.c_int(0)
    rc = getattr(bank.L, fn)(bank.h, ch, None if null_rows else buf.ctypes.data, cap, C.byref(n))
    return rc, buf[:n.value].copy()


def _full(bank, fn, ch, width, dtype):
    from jaero_amd import capi
    rc, rows = _read(bank, fn, ch, width, dtype, 1 << 16)
    assert rc == capi.E_OK, bank.L.jaero_last_error()
    rc, more = _read(bank, fn, ch, width, dtype, 1 << 16)
    assert rc == capi.E_OK and len(more) == 0
    return rows


@pytest.mark.parametrize("case", list(CH))
@pytest.mark.parametrize("reader", list(READERS))
def test_reader(twins, reader, case):
    from jaero_amd import capi
    kind, fn, width, dtype = READERS[reader]
    a, b = twins(kind)
    ch = CH[case]
    want = _full(b, fn, ch, width, dtype)
    assert len(want) > 0, reader
    if case == "pieces":
        parts, sizes = [], [1, 2, 3]
        step = max(3, len(want) // 6)
        while True:
            rc, rows = _read(a, fn, ch, width, dtype, sizes[len(parts)] if len(parts) < len(sizes) else step)
            assert rc == capi.E_OK, a.L.jaero_last_error()
            if len(rows) == 0:
                break
            parts.append(rows)
        got = np.concatenate(parts)
    else:
        rc, _ = _read(a, fn, ch, width, dtype, -1 if case == "negcap" else 16, null_rows=case == "nullrows")
        assert rc == capi.E_INVAL
        got = _full(a, fn, ch, width, dtype)
    assert got.shape == want.shape and np.array_equal(got, want), reader


def test_profile_totals_survive_a_rate_change():
    """jaero_profile_read: the launches a bank timed before a rate-changing jaero_set_settings (read or not yet read) stay in its totals, and
    the re-created bank keeps adding to them."""
    from jaero_amd import capi
    from jaero_amd import demodulator as D

    capi.lib()
    pcm = np.stack([G.msk(20000, fb=600.0, seed=G.SEED_BASE + 950 + c)[0] for c in range(2)])
    a = D.DemodulatorBank(D.MskSettings(), 2, max_write_samples=4096)
    b = D.DemodulatorBank(D.MskSettings(), 2, max_write_samples=4096)
    for bank in (a, b):
        bank.profile_enable(True)
        _feed_demod(bank, pcm[:, :10000], 4096)
    first = [a.profile_read(k) for k in range(3)]
    for bank in (a, b):
        _feed_demod(bank, pcm[:, 10000:], 4096)  # not read before the rate change
    a.set_settings(D.MskSettings(fb=1200.0, lockingbw=1800.0))
    after = [a.profile_read(k) for k in range(3)]
    twin = [b.profile_read(k) for k in range(3)]
    for k in range(3):
        assert after[k][1] == twin[k][1] > first[k][1] > 0, (k, first, after, twin)
        assert after[k][0] > first[k][0] > 0
    _feed_demod(a, pcm, 4096)
    grown = [a.profile_read(k) for k in range(3)]
    for k in range(3):
        assert grown[k][1] > after[k][1] and grown[k][0] > after[k][0]
    a.close()
    b.close()


@pytest.mark.parametrize("kind", ["aerolp", "aerolc"])
def test_aerol_profile_counts_every_class(kind):
    from jaero_amd import capi
    capi.lib()
    bank = BANKS[kind]()  # fed without profiling: nothing counted
    assert all(bank.profile_read(k) == (0.0, 0) for k in range(3))
    bank.profile_enable(True)
    soft = np.full((3, 4096), 128, np.int16)
    bank.write(soft)
    bank.write(soft)
    for k in range(3):
        ms, n = bank.profile_read(k)
        assert n >= 2 and ms > 0, (k, ms, n)
    bank.close()
