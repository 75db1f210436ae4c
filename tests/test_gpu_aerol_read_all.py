"""GPU (-m gpu): jaero_aerol_read_all, every channel of one output class of an Aero-L bank in one call, against a twin bank that is fed the
same writes and read channel by channel through jaero_aerol_read_* (the path every other Aero-L test checks against the oracle).  Integer
rows: bit for bit.

Sizes follow the sweep kernels' workgroup of W = 256 channels: 1, 70 (part of one workgroup), 257 (a second workgroup holding one channel),
and 16 400 (65 workgroups: the strided loop that adds up the block sums in front of a workgroup wraps once; the bank decodes one block per
lane).  Counts are skewed: a third of the channels see noise only (no signal units), one kind of stream fills a channel's buffer exactly,
longer ones overflow it."""
import ctypes as C

import numpy as np
import pytest

from jaero_amd import aerol_frames as AF
from jaero_amd import signalgen as G

pytestmark = pytest.mark.gpu

W = 256  # SWEEP_W of k_aerol_sweep.h
PER_FRAME = {600: 6, 1200: 6, 10500: 26}


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
    return {K.AEROL_SUS: ("jaero_aerol_read_sus", np.int32, 16), K.AEROL_PACKETS: ("jaero_aerol_read_packets", np.int32, 16),
            K.AEROL_EVENTS: ("jaero_aerol_read_events", np.int64, 3), K.AEROL_VOICE: ("jaero_aerol_read_voice", np.uint8, 304)}


def read_channel(K, bank, what, ch, cap=4096):
    """The existing path: (rc, rows) of one channel."""
    fn, dt, width = classes(K)[what]
    buf = np.empty((cap, width), dt)
    n = C.c_int(0)
    rc = getattr(bank.L, fn)(bank.h, ch, buf.ctypes.data, cap, C.byref(n))
    assert rc in (K.E_OK, K.E_OVERFLOW), (rc, bank.L.jaero_last_error())
    return rc, buf[: n.value].copy()


def read_twin(K, twin, what, channels=None):
    rows, ov = [], []
    for c in range(twin.nch) if channels is None else channels:
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
    rc, off, got, taken, pending, o = bank.read_all_raw(what, caprows)
    etaken, eoff, epacked, epending = expect(rows, caprows)
    assert taken == etaken and pending == epending, (taken, etaken, pending, epending)
    assert np.array_equal(off, eoff)
    assert got.shape == epacked.shape and got.tobytes() == epacked.tobytes()
    eo = ov.copy()
    eo[taken:] = False
    assert np.array_equal(o, eo)
    assert rc == (K.E_OVERFLOW if eo.any() else K.E_OK)
    return taken


def p_streams(fb, ndistinct_seed=0):
    """Seven distinct soft-bit streams: noise only, and 2 .. 7 frames at different noise levels and arm inversions."""
    rng = np.random.default_rng(1000 + fb + ndistinct_seed)
    flen = {1200: 1200, 600: 1200, 10500: 5250}[fb]
    out = [np.clip(np.round(128 + rng.normal(0, 45, 3 * flen + 17)), 0, 255).astype(np.int16)]
    for nfr in range(2, 8):
        bits, _ = AF.p_channel_bits(AF.random_payloads(nfr, fb, seed=40 + nfr), fb, invert_i=bool(nfr & 1), invert_q=bool(nfr & 2))
        out.append(AF.to_soft(np.concatenate([bits, np.zeros(64, np.uint8)]), sigma=5.0 * nfr, seed=nfr))
    return out


def stream_of(c):
    return 0 if c % 3 == 1 else 1 + (c // 3 * 2 + (c % 3 == 2)) % 6  # a third of the channels: noise only; the others go round the six signals


def feed(banks, streams, which, width, rng=None):
    nch = len(which)
    lens = np.array([len(streams[k]) for k in which])
    pos = np.zeros(nch, dtype=np.int64)
    while (pos < lens).any():
        cnt = np.minimum(width if rng is None else rng.integers(width // 2, width + 1, size=nch), lens - pos).astype(np.int32)
        buf = np.zeros((nch, width), np.int16)
        for c in range(nch):
            buf[c, :cnt[c]] = streams[which[c]][pos[c]:pos[c] + cnt[c]]
        for b in banks:
            b.write(buf, cnt)
        pos += cnt


@pytest.mark.parametrize("fb", [1200, 10500])
@pytest.mark.parametrize("nch", [1, 70, W + 1])
def test_sus_and_events_equal_the_twin(B, K, oracle_mod, nch, fb):
    streams = p_streams(fb)
    # the signal units the 3-frame stream decodes to: that stream fills a channel's buffer exactly, the longer ones overflow it
    cap = len(oracle_mod.run_aerol(fb, streams[2], 1 << 20)["sus"])
    assert cap > PER_FRAME[fb]
    which = [stream_of(c) if nch > 1 else 3 for c in range(nch)]
    bank = B.AeroLBank(nch, fb, max_softbits_per_write=4000, su_capacity=cap)
    twin = B.AeroLBank(nch, fb, max_softbits_per_write=4000, su_capacity=cap)
    feed([bank, twin], streams, which, 4000, np.random.default_rng(nch))
    for what in (K.AEROL_SUS, K.AEROL_EVENTS):
        rows, ov = read_twin(K, twin, what)
        cnt = np.array([len(r) for r in rows])
        if what == K.AEROL_SUS and nch > 1:
            assert ((cnt == cap) & ~ov).any() and ov.any() and (cnt == 0).sum() >= nch // 3, (cnt, ov)
        total = int(cnt.sum())
        rc, _, _, taken, pending, _ = bank.read_all_raw(what, 0)  # the sizing call takes nothing that holds rows
        assert pending == total and taken == expect(rows, 0)[0] and rc == K.E_OK
        assert check_call(K, bank, what, total, rows, ov) == nch
        # left as the per-channel readers leave a channel: nothing to read, nothing to report
        for c in sorted({0, nch // 2, nch - 1}):
            rc, r = read_channel(K, bank, what, c)
            assert rc == K.E_OK and len(r) == 0
        assert bank.read_all_raw(what, 0)[3:5] == (nch, 0)
    bank.close(); twin.close()


def test_capacity_rule(B, K):
    """caprows = cnt_0 - 1 (nothing is taken, nothing touched), 0 (the sizing call), total - 1 (everything up to the last channel that holds
    rows), then the channels not taken read per channel exactly as the twin's."""
    nch, fb = 70, 1200
    streams = p_streams(fb)
    which = [stream_of(c) for c in range(nch)]
    bank = B.AeroLBank(nch, fb, max_softbits_per_write=6000, su_capacity=400)
    twin = B.AeroLBank(nch, fb, max_softbits_per_write=6000, su_capacity=400)
    feed([bank, twin], streams, which, 6000)
    rows, ov = read_twin(K, twin, K.AEROL_SUS)
    cnt = np.array([len(r) for r in rows])
    total = int(cnt.sum())
    assert cnt[0] > 1 and not ov.any()
    for caprows in (int(cnt[0]) - 1, 0):
        assert check_call(K, bank, K.AEROL_SUS, caprows, rows, ov) == 0
    last = int(np.nonzero(cnt)[0][-1])
    assert check_call(K, bank, K.AEROL_SUS, total - 1, rows, ov) == last
    for c in range(nch):
        rc, r = read_channel(K, bank, K.AEROL_SUS, c)
        assert rc == K.E_OK
        assert np.array_equal(r, rows[c]) if c >= last else len(r) == 0, c
    # a capacity in the middle: a prefix, and the next call hands over the rest behind it
    rows, ov = read_twin(K, twin, K.AEROL_EVENTS)
    cnt = np.array([len(r) for r in rows])
    mid = int(cnt[:37].sum()) + 1
    t = check_call(K, bank, K.AEROL_EVENTS, mid, rows, ov)
    assert 37 <= t < nch
    rest = [r[:0] if c < t else r for c, r in enumerate(rows)]
    assert check_call(K, bank, K.AEROL_EVENTS, int(cnt.sum()), rest, ov) == nch
    bank.close(); twin.close()


def test_state_continues_across_writes_and_readers_mix(B, K):
    """write, sweep, write, sweep on one bank = write, write, per-channel reads on the twin; and a per-channel read of channel 3 before a
    sweep leaves the sweep the twin's rows minus channel 3's."""
    nch, fb = 70, 1200
    streams = p_streams(fb)
    which = [stream_of(c) for c in range(nch)]
    bank = B.AeroLBank(nch, fb, max_softbits_per_write=2400, su_capacity=100)
    twin = B.AeroLBank(nch, fb, max_softbits_per_write=2400, su_capacity=100)
    n = max(len(s) for s in streams)
    parts = {K.AEROL_SUS: [[] for _ in range(nch)], K.AEROL_EVENTS: [[] for _ in range(nch)]}
    ch3 = {}
    for k, s0 in enumerate(range(0, n, 2400)):
        buf = np.zeros((nch, 2400), np.int16)
        cnt = np.zeros(nch, np.int32)
        for c in range(nch):
            seg = streams[which[c]][s0:s0 + 2400]
            buf[c, :len(seg)] = seg
            cnt[c] = len(seg)
        bank.write(buf, cnt)
        twin.write(buf, cnt)
        for what in parts:
            if k >= 1:  # mixing readers: channel 3 is read on its own first, the sweep then finds it empty
                r3 = read_channel(K, bank, what, 3)[1]
                ch3[what] = ch3.get(what, 0) + len(r3)
                parts[what][3].append(r3)
            off, rows, ov = bank.read_all(what)
            assert not ov.any()
            if k >= 1:
                assert off[4] == off[3]
            for c in range(nch):
                parts[what][c].append(rows[off[c]:off[c + 1]])
    for what in parts:
        rows, ov = read_twin(K, twin, what)
        assert not ov.any()
        assert sum(len(r) for r in rows) > nch
        for c in range(nch):
            assert np.array_equal(np.concatenate(parts[what][c]), rows[c]), (what, c)
    assert ch3[K.AEROL_EVENTS] > 0 and ch3[K.AEROL_SUS] > 0
    # classes this bank's mode does not have: the per-channel readers' own errors
    for what, code in ((K.AEROL_PACKETS, K.E_NOTSUP), (K.AEROL_VOICE, K.E_INVAL)):
        with pytest.raises(K.JaeroError) as e:
            _raw_what(K, bank, what)
        assert e.value.code == code
    bank.close(); twin.close()


def _raw_what(K, bank, what):
    off = np.zeros(bank.nch + 1, np.int32)
    n = C.c_int(0)
    K.check(bank.L.jaero_aerol_read_all(bank.h, what, None, 0, off.ctypes.data, C.byref(n), None, None))


def test_packets_and_events_of_a_burst_bank(B, K):
    nch = 70
    rng = np.random.default_rng(9)
    rb = lambda k: bytes(rng.integers(0, 256, k, dtype=np.uint8))
    distinct = [np.clip(np.round(128 + rng.normal(0, 40, 9000)), 0, 255).astype(np.int16)]
    for k in range(4):
        pk = [("R", rb(17)), ("T", (rb(4), [rb(10) for _ in range(2 + k)]))][: 1 + k % 2] + [("R", rb(17))] * (k // 2)
        distinct.append(AF.rt_burst_stream(pk, gap=3000, sigma=10.0 + 5 * k, seed=k, invert_i=bool(k & 1), invert_q=bool(k & 2)))
    which = [0 if c % 3 == 1 else 1 + c % 4 for c in range(nch)]
    bank = B.AeroLBank(nch, 10500, max_softbits_per_write=3000, su_capacity=700, burst=True)
    twin = B.AeroLBank(nch, 10500, max_softbits_per_write=3000, su_capacity=700, burst=True)
    feed([bank, twin], distinct, which, 3000, np.random.default_rng(4))
    for what in (K.AEROL_PACKETS, K.AEROL_EVENTS):
        rows, ov = read_twin(K, twin, what)
        total = sum(len(r) for r in rows)
        assert total > nch
        assert check_call(K, bank, what, total, rows, ov) == nch
    with pytest.raises(K.JaeroError) as e:
        _raw_what(K, bank, K.AEROL_SUS)
    assert e.value.code == K.E_NOTSUP
    bank.close(); twin.close()


def test_voice_sus_and_events_of_a_c_channel_bank(B, K):
    nch = 5
    streams = [AF.c_channel_case(7000 + c, 3 + c % 3, 10.0 + 4 * c, inv=(bool(c & 1), bool(c & 2)), lead=100 + 900 * c)[1] for c in range(nch)]
    streams[1] = np.clip(np.round(128 + np.random.default_rng(1).normal(0, 45, 9000)), 0, 255).astype(np.int16)
    bank = B.AeroLBank(nch, 8400, max_softbits_per_write=4096, su_capacity=9)  # three frames' units, three voice rows: the longest streams overflow
    twin = B.AeroLBank(nch, 8400, max_softbits_per_write=4096, su_capacity=9)
    feed([bank, twin], streams, list(range(nch)), 4096, np.random.default_rng(2))
    seen_ov = False
    for what in (K.AEROL_VOICE, K.AEROL_SUS, K.AEROL_EVENTS):
        rows, ov = read_twin(K, twin, what)
        total = sum(len(r) for r in rows)
        assert total > 0
        seen_ov |= bool(ov.any())
        assert check_call(K, bank, what, total, rows, ov) == nch
    assert seen_ov
    with pytest.raises(K.JaeroError) as e:
        _raw_what(K, bank, K.AEROL_PACKETS)
    assert e.value.code == K.E_NOTSUP
    bank.close(); twin.close()


def test_16400_channels(B, K):
    """65 workgroups, the lane-layout Viterbi, su_capacity 8 and three frames in three writes without a read in between: channels with two
    decoded frames (12 units) overflow.  The twin holds each distinct stream once (a bank's channels are independent: test_gpu_aerol.py,
    test_gpu_scale_aerol.py) and is read per channel; the sweep of the large bank must return, for every channel, its stream's rows."""
    nch, fb = 16400, 1200
    streams = [s[:3600] for s in p_streams(fb)]
    which = np.array([stream_of(c) for c in range(nch)])
    bank = B.AeroLBank(nch, fb, max_softbits_per_write=1200, su_capacity=8)
    twin = B.AeroLBank(len(streams), fb, max_softbits_per_write=1200, su_capacity=8)
    for s0 in range(0, 3600, 1200):
        small = np.stack([np.pad(s[s0:s0 + 1200], (0, 1200 - len(s[s0:s0 + 1200]))) for s in streams]).astype(np.int16)
        cnt = np.array([len(s[s0:s0 + 1200]) for s in streams], np.int32)
        twin.write(small, cnt)
        bank.write(small[which], cnt[which])
    for what in (K.AEROL_SUS, K.AEROL_EVENTS):
        trows, tov = read_twin(K, twin, what)
        tcnt = np.array([len(r) for r in trows])
        cnt = tcnt[which]
        if what == K.AEROL_SUS:
            assert tov.any() and (tcnt == 0).any() and (tcnt > 0).any()
        rc, off, got, taken, pending, ov = bank.read_all_raw(what, int(cnt.sum()))
        assert taken == nch and pending == int(cnt.sum())
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32))
        assert np.array_equal(ov, tov[which]) and rc == (K.E_OVERFLOW if tov[which].any() else K.E_OK)
        want = np.concatenate([trows[k] for k in which])
        assert got.shape == want.shape and got.tobytes() == want.tobytes()
        assert bank.read_all_raw(what, 0)[3:5] == (nch, 0)
    bank.close(); twin.close()


def test_an_unswept_unlinked_bank_is_the_bank_it_was(B, K):
    """A bank that is never swept or linked launches and allocates what it did before: its three kernel classes count the same launches as a twin
    that is swept after every write, and its slots 3 (sweep) and 4 (link) stay empty."""
    nch, fb = 70, 1200
    streams = p_streams(fb)
    which = [stream_of(c) for c in range(nch)]
    plain = B.AeroLBank(nch, fb, max_softbits_per_write=2400, su_capacity=100)
    swept = B.AeroLBank(nch, fb, max_softbits_per_write=2400, su_capacity=100)
    for b in (plain, swept):
        b.profile_enable(True)
    n = max(len(s) for s in streams)
    nwrites = 0
    for s0 in range(0, n, 2400):
        buf = np.zeros((nch, 2400), np.int16)
        cnt = np.zeros(nch, np.int32)
        for c in range(nch):
            seg = streams[which[c]][s0:s0 + 2400]
            buf[c, :len(seg)] = seg
            cnt[c] = len(seg)
        plain.write(buf, cnt)
        swept.write(buf, cnt)
        swept.read_sus_all()
        plain.tick_dcd(); swept.tick_dcd()
        nwrites += 1
    for which_slot in (0, 1, 2):
        a, b = plain.profile_read(which_slot), swept.profile_read(which_slot)
        assert a[1] == b[1] > 0
        assert plain.profile2_read(which_slot)[1] == a[1]
    assert plain.profile2_read(3) == (0.0, 0) and plain.profile2_read(4) == (0.0, 0)
    # and allocates what it did: the mark column, the sweep's scratch and its pack buffer exist only once they are used
    extra = lambda b: b.L.jaero_aerol_debug_extra_bytes(b.h)
    assert extra(plain) == 0 and extra(swept) > 0
    assert swept.profile2_read(3)[1] >= nwrites and swept.profile2_read(4) == (0.0, 0)
    with pytest.raises(K.JaeroError):
        plain.profile_read(3)  # the older entry point keeps its range
    plain.close(); swept.close()


def test_pcm_to_signal_units_with_link_and_one_call_reads(B):
    """test_gpu_aerol.py::test_pcm_to_signal_units_on_device's chain as a receiver runs it: the Aero-L bank linked to the demodulator bank
    (carrier detect fed back on the device) and every channel's signal units read in one call per chunk."""
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
    for s in range(0, n, chunk):
        demod.write(pcm[:, s:s + chunk])
        aerol.write_from_bank(demod, 8192)
        off, rows, ov = aerol.read_sus_all()
        assert not ov.any()
        for c in range(nch):
            got[c].append(rows[off[c]:off[c + 1]])
    for c in range(nch):
        sus = np.concatenate(got[c])
        good = [bytes(r[2:12].astype(np.uint8)) for r in sus if r[14]]
        sent = [p for fr in pays[c] for p in fr]
        assert len(good) >= 26 * 6, (c, len(good))
        i0 = sent.index(good[0])
        assert good == sent[i0:i0 + len(good)], c
    aerol.close()
    demod.close()
