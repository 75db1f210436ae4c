"""GPU (-m gpu): jaero_read_all and jaero_read_status_all, every channel of a demodulator bank in one call, against a twin bank that is fed the
same writes and read channel by channel through jaero_read_softbits / _status_log / _events / _symbols / _status (the path every other test
checks against the oracle).  Rows, offsets and counts: exact equality.

Sizes follow the sweep kernels' workgroup of W = 256 channels: 1, 70 (part of one workgroup), 257 (a second workgroup holding one channel)
and 513 (three block sums).  The soft-bit gather (k_sweep_gather_i16) packs 2-byte rows into 16-byte words: the counts are made ragged
(channels drained to zero between others, odd counts, workgroup totals that are no multiple of 8) and the tests assert that they are."""
import ctypes as C

import numpy as np
import pytest

from jaero_amd import aerol_frames as AF
from jaero_amd import signalgen as G

pytestmark = pytest.mark.gpu

W = 256  # SWEEP_W of k_aerol_sweep.h


@pytest.fixture(scope="module")
def B():
    from jaero_amd import capi
    from jaero_amd import demodulator as D

    capi.lib()
    return D


@pytest.fixture(scope="module")
def K():
    from jaero_amd import capi

    return capi


def classes(K):
    return {K.BANK_SOFTBITS: ("jaero_read_softbits", np.int16, 1), K.BANK_STATUS_LOG: ("jaero_read_status_log", np.float64, 6),
            K.BANK_EVENTS: ("jaero_read_events", np.float64, 3), K.BANK_SYMBOLS: ("jaero_read_symbols", np.float64, 3)}


def read_channel(K, bank, what, ch, cap=1 << 16):
    """The existing path: (rc, rows) of one channel."""
    fn, dt, width = classes(K)[what]
    buf = np.empty((max(cap, 1), width), dt)
    n = C.c_int(0)
    rc = getattr(bank.L, fn)(bank.h, ch, buf.ctypes.data, cap, C.byref(n))
    assert rc in (K.E_OK, K.E_OVERFLOW), (rc, bank.L.jaero_last_error())
    rows = buf[: n.value].copy()
    return rc, rows.reshape(-1) if width == 1 else rows


def read_twin(K, twin, what):
    rows, ov = [], []
    for c in range(twin.nch):
        rc, r = read_channel(K, twin, what, c)
        rows.append(r)
        ov.append(rc == K.E_OVERFLOW)
    return rows, np.array(ov, dtype=bool)


def expect(rows, caprows):
    """The definition: (taken, offsets[nch + 1], packed rows, pending) for per-channel rows and a capacity."""
    cnt = np.array([len(r) for r in rows], dtype=np.int64)
    P = np.cumsum(cnt)
    taken = int((P <= caprows).sum())
    off = np.concatenate([[0], P])
    off[taken:] = off[taken]
    packed = np.concatenate(rows[:taken]) if taken else rows[0][:0]
    return taken, off.astype(np.int32), packed, int(P[-1])


def check_call(K, bank, what, caprows, rows, ov):
    rc, got, off, taken, pending, o = bank.read_all_raw(what, caprows)
    etaken, eoff, epacked, epending = expect(rows, caprows)
    assert taken == etaken and pending == epending, (taken, etaken, pending, epending)
    assert np.array_equal(off, eoff)
    assert got.shape == epacked.shape and got.dtype == epacked.dtype and got.tobytes() == epacked.tobytes()
    eo = ov.copy()
    eo[taken:] = False
    assert np.array_equal(o, eo)
    assert rc == (K.E_OVERFLOW if eo.any() else K.E_OK)
    return taken


def check_whole(K, bank, twin, what):
    """The sizing call, then everything in one call, against the twin read per channel; the bank is left with nothing to read."""
    rows, ov = read_twin(K, twin, what)
    total = sum(len(r) for r in rows)
    rc, _, _, taken, pending, _ = bank.read_all_raw(what, 0)
    assert pending == total and taken == expect(rows, 0)[0]
    assert check_call(K, bank, what, total, rows, ov) == bank.nch
    return rows, ov


def feed(banks, pcm, chunk):
    for s in range(0, pcm.shape[1], chunk):
        for b in banks:
            b.write(pcm[:, s:s + chunk])


def continuous(B, kind, nch, n, **kw):
    """Two identical banks and their PCM: four distinct signals tiled over the channels."""
    if kind == "oqpsk":
        sig = [G.oqpsk(n, fc=8000.0 + 9.0 * k, seed=G.SEED_BASE + 1200 + k)[0] for k in range(4)]
        st = B.OqpskSettings()
    else:
        sig = [G.msk(n, fb=1200.0, fc=1000.0 + 7.0 * k, seed=G.SEED_BASE + 1210 + k)[0] for k in range(4)]
        st = B.MskSettings(fb=1200.0, lockingbw=1800.0)
    pcm = np.stack([sig[c % 4] for c in range(nch)])
    kw.setdefault("softbit_capacity", 20000)
    return [B.DemodulatorBank(st, nch, max_write_samples=10000, **kw) for _ in range(2)], pcm


# ---- 1. continuous soft bits, ragged ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nch", [("oqpsk", 1), ("oqpsk", 70), ("oqpsk", W + 1), ("msk", 1), ("msk", 70), ("msk", W + 1), ("oqpsk", 2 * W + 1)])
def test_continuous_softbits_ragged(B, K, kind, nch):
    (bank, twin), pcm = continuous(B, kind, nch, 30000)
    feed([bank, twin], pcm[:, :20000], 10000)
    for b in (bank, twin):
        for c in range(1, nch - 1, 3):  # channels without rows between the others (not the last one: 257 keeps rows in its second workgroup)
            assert read_channel(K, b, K.BANK_SOFTBITS, c)[0] == K.E_OK
        for c in range(0, nch, 5):  # odd counts: offsets off every alignment
            rc, r = read_channel(K, b, K.BANK_SOFTBITS, c, cap=7)
            assert rc == K.E_OK and (len(r) == 7 or c % 3 == 1)
    cnt, pend = bank.softbit_counts()
    assert not pend.any() and cnt.sum() > 0
    print("counts", kind, nch, cnt[:12], "workgroup totals", [int(cnt[k:k + W].sum()) for k in range(0, nch, W)])
    assert (cnt & 1).any()
    if nch > 1:  # otherwise the test proves nothing about the gather's word boundaries
        assert (cnt == 0).any() and int(cnt[:W].sum()) % 8 != 0
    rows, _ = check_whole(K, bank, twin, K.BANK_SOFTBITS)
    assert np.array_equal(np.array([len(r) for r in rows]), cnt)
    assert not bank.softbit_counts()[0].any()
    # the state continues
    feed([bank, twin], pcm[:, 20000:], 10000)
    for c in range(nch):
        ra, rb = read_channel(K, bank, K.BANK_SOFTBITS, c), read_channel(K, twin, K.BANK_SOFTBITS, c)
        assert ra[0] == rb[0] == K.E_OK and len(ra[1]) > 0 and np.array_equal(ra[1], rb[1]), c
    bank.close(); twin.close()


# ---- 2. burst soft bits with a live tail -----------------------------------------------------------------------------------------------
# Bursts on the even channels, each a few samples later than the one before, so that a write that ends inside the bursts leaves channels at
# every stage: groups emitted and a tail pending, a tail only, nothing yet.  The odd channels see noise only.
BURST = {
    # kind: (samples per channel, first burst start, stagger per bursting channel, samples of the first write)
    "burstoqpsk": (72000, 40000, 61, 53000),
    "burstmsk": (112000, 40000, 131, 69500),
}


def burst_pcm(kind, nch):
    n, start, stagger, _ = BURST[kind]
    lead = stagger * nch
    if kind == "burstoqpsk":
        base = G.burst_oqpsk(n + lead, burst_starts=[start + lead], ndata_sym=700, fc=8010.0, ebno_db=16.0, seed=G.SEED_BASE + 1300)[0]
        quiet = G.burst_oqpsk(n, burst_starts=[], fc=8010.0, ebno_db=16.0, seed=G.SEED_BASE + 1301)[0]
    else:
        base = G.burst_msk(n + lead, burst_starts=[start + lead], fc=1900.0, ebno_db=18.0, seed=G.SEED_BASE + 1310)[0]
        quiet = G.burst_msk(n, burst_starts=[], fc=1900.0, ebno_db=18.0, seed=G.SEED_BASE + 1311)[0]
    pcm = np.empty((nch, n), np.int16)
    for c in range(nch):
        if c % 2:
            pcm[c] = np.roll(quiet, 997 * c)
        else:  # the burst of channel c starts at start + stagger * c / 2
            s0 = lead - stagger * (c // 2)
            pcm[c] = base[s0:s0 + n]
    return pcm


def burst_banks(B, kind, nch, count):
    st = B.BurstOqpskSettings(freq_center=8010.0) if kind == "burstoqpsk" else B.BurstMskSettings(freq_center=1900.0, fb=1200.0, lockingbw=1800.0)
    return [B.DemodulatorBank(st, nch, trace=True, max_write_samples=8192, softbit_capacity=30000) for _ in range(count)]


@pytest.fixture(scope="module")
def burst_signals():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = burst_pcm(kind, 70)
        return made[kind]

    return get


@pytest.mark.parametrize("kind", list(BURST))
def test_burst_softbits_keep_the_pending_tail(B, K, burst_signals, kind):
    nch, cut = 70, BURST[kind][3]
    pcm = burst_signals(kind)
    bank, twin, swept, plain = burst_banks(B, kind, nch, 4)
    feed([bank, twin, swept, plain], pcm[:, :cut], 8192)
    cnt, pend = bank.softbit_counts()
    emitted = cnt - pend
    print("burst counts", kind, "held", cnt[:20], "pending", pend[:20])
    assert ((pend > 0) & (emitted > 0)).any() and ((pend > 0) & (emitted == 0)).any() and (cnt == 0).any()
    rows, _ = check_whole(K, bank, twin, K.BANK_SOFTBITS)
    assert np.array_equal(np.array([len(r) for r in rows]), emitted)
    assert any((r == -1).any() for r in rows)  # start-of-burst markers came along
    cnt2, pend2 = bank.softbit_counts()
    assert np.array_equal(cnt2, pend) and np.array_equal(pend2, pend)  # the tail is what is left, at the front
    first = swept.read_all(K.BANK_SOFTBITS)
    # the rest of the signal: the tail survived and was not duplicated
    feed([bank, twin, swept, plain], pcm[:, cut:], 8192)
    more = 0
    for c in range(nch):
        ra, rb = read_channel(K, bank, K.BANK_SOFTBITS, c), read_channel(K, twin, K.BANK_SOFTBITS, c)
        assert ra[0] == rb[0] == K.E_OK and np.array_equal(ra[1], rb[1]), c
        more += len(ra[1])
    assert more > 0
    # write, sweep, write, sweep = write, write, read per channel
    second = swept.read_all(K.BANK_SOFTBITS)
    assert first[2] == second[2] == nch
    for c in range(nch):
        got = np.concatenate([r[off[c]:off[c + 1]] for r, off, _ in (first, second)])
        assert np.array_equal(got, read_channel(K, plain, K.BANK_SOFTBITS, c)[1]), c
    for b in (bank, twin, swept, plain):
        b.close()


# ---- 3. logs ---------------------------------------------------------------------------------------------------------------------------
def test_status_log_of_a_continuous_bank(B, K):
    (bank, twin), pcm = continuous(B, "oqpsk", 70, 30000, status_log=True)
    feed([bank, twin], pcm, 10000)
    rows, _ = check_whole(K, bank, twin, K.BANK_STATUS_LOG)
    assert min(len(r) for r in rows) > 0 and rows[0].shape[1] == 6
    assert bank.read_all_raw(K.BANK_STATUS_LOG, 0)[3:5] == (70, 0)
    bank.close(); twin.close()


@pytest.mark.parametrize("kind", list(BURST))
def test_events_of_a_burst_bank(B, K, burst_signals, kind):
    nch, cut = 70, BURST[kind][3]
    pcm = burst_signals(kind)
    bank, twin = burst_banks(B, kind, nch, 2)
    feed([bank, twin], pcm[:, :cut], 8192)
    rows, _ = check_whole(K, bank, twin, K.BANK_EVENTS)
    cnt = np.array([len(r) for r in rows])
    assert cnt.sum() > 4 * nch and len(set(cnt)) > 1 and rows[0].shape[1] == 3
    feed([bank, twin], pcm[:, cut:cut + 8192], 8192)
    check_whole(K, bank, twin, K.BANK_EVENTS)
    bank.close(); twin.close()


def test_symbols_of_a_five_channel_bank(B, K):
    (bank, twin), pcm = continuous(B, "oqpsk", 5, 20000, capture_symbols=True)
    feed([bank, twin], pcm, 10000)
    assert read_channel(K, bank, K.BANK_SYMBOLS, 2)[0] == read_channel(K, twin, K.BANK_SYMBOLS, 2)[0] == K.E_OK  # one channel without rows
    rows, _ = check_whole(K, bank, twin, K.BANK_SYMBOLS)
    assert sum(len(r) for r in rows) > 1000 and len(rows[2]) == 0
    bank.close(); twin.close()


# ---- 4. the capacity rule --------------------------------------------------------------------------------------------------------------
def test_capacity_rule_on_softbits(B, K):
    """caprows = v_0 - 1 (nothing is taken, nothing touched), 0 (the sizing call), a capacity in the middle of the channels (a prefix), total - 1
    (everything up to the last channel), then the channel not taken read per channel exactly as the twin's."""
    nch = 70
    (bank, twin), pcm = continuous(B, "oqpsk", nch, 10000)
    feed([bank, twin], pcm, 10000)
    rows, ov = read_twin(K, twin, K.BANK_SOFTBITS)
    cnt = np.array([len(r) for r in rows])
    assert cnt.min() > 1 and not ov.any()
    for caprows in (int(cnt[0]) - 1, 0):
        assert check_call(K, bank, K.BANK_SOFTBITS, caprows, rows, ov) == 0
    t = check_call(K, bank, K.BANK_SOFTBITS, int(cnt[:37].sum()) + 1, rows, ov)
    assert t == 37
    rest = [r[:0] if c < t else r for c, r in enumerate(rows)]
    assert check_call(K, bank, K.BANK_SOFTBITS, int(cnt[t:].sum()) - 1, rest, ov) == nch - 1
    for c in range(nch):
        rc, r = read_channel(K, bank, K.BANK_SOFTBITS, c)
        assert rc == K.E_OK
        assert np.array_equal(r, rows[c]) if c == nch - 1 else len(r) == 0, c
    bank.close(); twin.close()


# ---- 5. overflow -----------------------------------------------------------------------------------------------------------------------
def test_overflowed_channels_are_reported_where_the_twin_reports_them(B, K):
    nch = 70
    (bank, twin), pcm = continuous(B, "oqpsk", nch, 20000, softbit_capacity=1000)  # a write of 4000 samples makes at most 875 soft bits
    for s0 in range(0, 20000, 4000):
        feed([bank, twin], pcm[:, s0:s0 + 4000], 4000)
        if s0 < 16000:  # the even channels are read in time (and hold the last write's bits at the sweep), the odd ones never
            for b in (bank, twin):
                for c in range(0, nch, 2):
                    assert read_channel(K, b, K.BANK_SOFTBITS, c)[0] == K.E_OK
    rows, ov = read_twin(K, twin, K.BANK_SOFTBITS)
    assert ov.any() and not ov[::2].any() and len(set(len(r) for r in rows)) > 2  # (how many bits a channel makes depends on when it locks)
    total = sum(len(r) for r in rows)
    rc, got, off, taken, pending, o = bank.read_all_raw(K.BANK_SOFTBITS, total)
    assert rc == K.E_OVERFLOW and b"jaero_read_all" in bank.L.jaero_last_error()
    assert taken == nch and pending == total and np.array_equal(o, ov)
    assert np.array_equal(off, expect(rows, total)[1]) and np.array_equal(got, np.concatenate(rows))
    # the bits are cleared: neither reader reports them again
    assert bank.read_all_raw(K.BANK_SOFTBITS, 0)[0] == K.E_OK
    assert all(read_channel(K, bank, K.BANK_SOFTBITS, c)[0] == K.E_OK for c in range(nch))
    # and the Python surface: raised after the arrays are filled, or handed back
    feed([bank, twin], pcm, 4000)
    rows, ov = read_twin(K, twin, K.BANK_SOFTBITS)
    assert ov.any()
    with pytest.raises(K.JaeroError) as e:
        bank.read_all(K.BANK_SOFTBITS)
    assert e.value.code == K.E_OVERFLOW and np.array_equal(e.value.overflowed, ov)
    flat, off, taken = e.value.result
    assert taken == nch and np.array_equal(flat, np.concatenate(rows))
    feed([bank], pcm, 4000)
    assert bank.read_all(K.BANK_SOFTBITS, overflowed=True)[3].any()
    bank.close(); twin.close()


# ---- 6. refusals with a device ---------------------------------------------------------------------------------------------------------
def _refused(K, bank, what):
    off = np.full(bank.nch + 1, -3, np.int32)
    n = C.c_int(-7)
    rc = bank.L.jaero_read_all(bank.h, what, None, 0, off.ctypes.data, C.byref(n), None, None)
    assert n.value == -7 and (off == -3).all()
    return rc


def test_classes_a_bank_does_not_have(B, K, burst_signals):
    (cont, twin), pcm = continuous(B, "oqpsk", 5, 10000)
    feed([cont, twin], pcm, 10000)
    assert _refused(K, cont, K.BANK_EVENTS) == K.E_NOTSUP and b"jaero_read_all" in cont.L.jaero_last_error()
    assert _refused(K, cont, K.BANK_STATUS_LOG) == K.E_INVAL  # not enabled at create
    assert _refused(K, cont, K.BANK_SYMBOLS) == K.E_INVAL
    check_whole(K, cont, twin, K.BANK_SOFTBITS)  # every row still readable
    cont.close(); twin.close()
    kind = "burstoqpsk"
    burst, btwin = burst_banks(B, kind, 70, 2)
    feed([burst, btwin], burst_signals(kind)[:, :BURST[kind][3]], 8192)
    assert _refused(K, burst, K.BANK_STATUS_LOG) == K.E_NOTSUP
    assert _refused(K, burst, K.BANK_SYMBOLS) == K.E_INVAL
    buf = np.zeros((70, 64), np.int16)
    counts = np.zeros(70, np.int32)
    assert burst.L.jaero_read_softbits_all(burst.h, buf.ctypes.data, 64, counts.ctypes.data) == K.E_NOTSUP  # as before
    check_whole(K, burst, btwin, K.BANK_SOFTBITS)
    check_whole(K, burst, btwin, K.BANK_EVENTS)
    burst.close(); btwin.close()


# ---- 7. read_status_all ----------------------------------------------------------------------------------------------------------------
def status_equals_per_channel(bank):
    st = bank.read_status_all()
    assert st.shape == (bank.nch,) and st.dtype.itemsize == 40
    for c in range(bank.nch):
        assert st[c].tobytes() == bytes(bank.read_status(c)), c
    return st


def test_status_all_continuous_257(B, K):
    (bank, twin), pcm = continuous(B, "oqpsk", W + 1, 20000)
    twin.close()
    feed([bank], pcm, 10000)
    st = status_equals_per_channel(bank)
    assert st["n_estimates"].min() > 0 and len(set(st["freq_est"])) > 1
    bank.close()


@pytest.mark.parametrize("kind", list(BURST))
def test_status_all_burst_mid_burst(B, K, burst_signals, kind):
    bank, = burst_banks(B, kind, 70, 1)
    feed([bank], burst_signals(kind)[:, :BURST[kind][3]], 8192)
    st = status_equals_per_channel(bank)
    assert set(st["signal"]) == {0, 1}  # some channels are inside their burst
    bank.close()


def test_status_all_8400(B, K):
    pcm = np.stack([G.oqpsk(20000, fb=8400.0, fc=8000.0 + 5.0 * c, seed=G.SEED_BASE + 1400 + c)[0] for c in range(5)])
    bank = B.DemodulatorBank(B.OqpskSettings(fb=8400.0, lockingbw=8400.0), 5, max_write_samples=4096)
    feed([bank], pcm, 4096)
    status_equals_per_channel(bank)
    bank.close()


# ---- 8. untouched banks and rate changes -----------------------------------------------------------------------------------------------
def test_an_unswept_bank_is_the_bank_it_was_and_a_rate_change(B, K):
    nch = 5
    sig = [G.msk(24000, fb=1200.0, fc=1000.0 + 7.0 * k, seed=G.SEED_BASE + 1500 + k)[0] for k in range(nch)]
    slow = [G.msk(24000, fb=600.0, fc=1000.0 + 7.0 * k, seed=G.SEED_BASE + 1510 + k)[0] for k in range(nch)]
    pcm, pcm600 = np.stack(sig), np.stack(slow)
    st = B.MskSettings(fb=1200.0, lockingbw=1800.0)
    plain, swept, twin = [B.DemodulatorBank(st, nch, max_write_samples=8192, softbit_capacity=20000) for _ in range(3)]
    for b in (plain, swept, twin):
        b.profile_enable(True)
    sweeps = 0
    for s in range(0, 24000, 8000):
        feed([plain, swept, twin], pcm[:, s:s + 8000], 8000)
        check_whole(K, swept, twin, K.BANK_SOFTBITS)
        swept.read_status_all()
        sweeps += 1
    for k in range(5):
        assert plain.profile_read(k)[1] == swept.profile_read(k)[1], k
    assert plain.profile_read(0)[1] > 0
    assert plain.read_all_bytes() == 0 and plain.profile2_read(5) == (0.0, 0)
    assert swept.read_all_bytes() > 0
    ms5, n5 = swept.profile2_read(5)
    assert n5 >= 3 * sweeps and ms5 > 0  # per sweep: the sizing call, the offsets, the gather (and the status kernel)
    with pytest.raises(K.JaeroError):
        swept.profile_read(5)  # the older entry point keeps its range
    with pytest.raises(K.JaeroError):
        swept.profile2_read(6)
    # 1200 -> 600 bps: a new bank behind the handle; the scratch went with the old one and is allocated afresh
    for b in (swept, twin):
        b.set_settings(B.MskSettings())
    assert swept.read_all_bytes() == 0
    assert swept.profile2_read(5)[1] == n5
    feed([swept, twin], pcm600, 8000)
    st_all = swept.read_status_all()
    for c in range(nch):
        assert st_all[c].tobytes() == bytes(twin.read_status(c)), c
    rows, _ = check_whole(K, swept, twin, K.BANK_SOFTBITS)
    assert sum(len(r) for r in rows) > 0
    assert swept.read_all_bytes() > 0 and swept.profile2_read(5)[1] > n5
    for b in (plain, swept, twin):
        b.close()


# ---- 9. one end-to-end use -------------------------------------------------------------------------------------------------------------
def test_pcm_to_signal_units_with_status_polled_between_the_writes(B):
    """tests/test_gpu_aerol_read_all.py::test_pcm_to_signal_units_with_link_and_one_call_reads's chain with every channel's status polled in one
    call between the bank's write and the linked Aero-L bank's write on the same stream."""
    fb, nch, nfr = 10500, 3, 14
    pays, pcms = [], []
    for c in range(nch):
        pay = AF.random_payloads(nfr, fb, seed=50 + c)
        bits, _ = AF.p_channel_bits(pay, fb)
        n = int(len(bits) / 2 * 48000 / 5250) + 2000
        pcm, _ = G.oqpsk(n, fc=8000.0 + 11.0 * c, ebno_db=13.0, seed=70 + c, bits=np.concatenate([bits, np.zeros(64, np.uint8)]))
        pays.append(pay)
        pcms.append(pcm)
    n = min(len(p) for p in pcms)
    pcm = np.stack([p[:n] for p in pcms])
    chunk = 24000
    demod = B.DemodulatorBank(B.OqpskSettings(), nch, device=0, max_write_samples=chunk, softbit_capacity=8192)
    aerol = B.AeroLBank(nch, fb, max_softbits_per_write=8192, su_capacity=26 * nfr + 8)
    aerol.link_dcd(demod)
    got = [[] for _ in range(nch)]
    locked = 0
    for s in range(0, n, chunk):
        demod.write(pcm[:, s:s + chunk])
        st = demod.read_status_all()
        for c in range(nch):
            one = demod.read_status(c)
            assert st["signal"][c] == one.signal and st[c].tobytes() == bytes(one), (s, c)
        locked += int(st["signal"].sum())
        aerol.write_from_bank(demod, 8192)
        off, rows, ov = aerol.read_sus_all()
        assert not ov.any()
        for c in range(nch):
            got[c].append(rows[off[c]:off[c + 1]])
    assert locked > nch
    for c in range(nch):
        sus = np.concatenate(got[c])
        good = [bytes(r[2:12].astype(np.uint8)) for r in sus if r[14]]
        sent = [p for fr in pays[c] for p in fr]
        assert len(good) >= 26 * 6, (c, len(good))
        i0 = sent.index(good[0])
        assert good == sent[i0:i0 + len(good)], c
    aerol.close()
    demod.close()
