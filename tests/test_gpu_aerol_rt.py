"""GPU (-m gpu): the R / T reassembly of a burst Aero-L bank (jaero_aerol_rt_enable, jaero_amd/csrc/k_aerolb_isu.h) against the definition as
tests/rt_isu_oracle.py states it, over the case streams of tests/rt_isu_cases.py: message rows, the eight counters, the three rates, both
Viterbi layouts, logs without room, the one-call read, enabling and disabling, the refusals, and the chain from PCM to defragmented ACARS
text.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import rt_isu_cases as RC
import rt_isu_oracle as RO
from jaero_amd import acars
from jaero_amd import aerol_frames as AF
from jaero_amd import signalgen as G

pytestmark = pytest.mark.gpu


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


def feed(banks, streams, width, rng=None, start=None, stop=None):
    """Ragged per-channel counts in every write (rng) or full-width writes, of streams[c][start[c]:stop[c]]."""
    nch = len(streams)
    lens = np.array([len(s) for s in streams]) if stop is None else np.asarray(stop)
    pos = np.zeros(nch, dtype=np.int64) if start is None else np.asarray(start).astype(np.int64)
    while (pos < lens).any():
        cnt = np.minimum(width if rng is None else rng.integers(1, width + 1, size=nch), lens - pos).astype(np.int32)
        buf = np.zeros((nch, width), np.int16)
        for c in range(nch):
            buf[c, :cnt[c]] = streams[c][pos[c]:pos[c] + cnt[c]]
        for b in banks:
            b.write(buf, cnt)
        pos += cnt


def extra(b):
    return b.L.jaero_aerol_debug_extra_bytes(b.h)


def check_bank(bank, twin, plan, fb, O, cap=None, packet_rows=True):
    """Messages (one call for all channels) and counters against the restatement run on the oracle's packets; packets and events -- the
    feature changes neither -- against the oracle's and, bit for bit, a twin bank's that never enabled."""
    off, rows, ovf = bank.read_msgs_all()
    stats = bank.rt_stats()
    total = 0
    for c, (name, inv) in enumerate(plan):
        msgs, st, _, pk, ev, _ = RC.expected(O, name, fb, inv)
        want = msgs if cap is None else msgs[:cap]
        got = rows[off[c]:off[c + 1]]
        assert len(got) == len(want) and got.tobytes() == want.tobytes(), (c, name)
        assert bool(ovf[c]) == (cap is not None and len(msgs) > cap), (c, name)
        assert np.array_equal(stats[c], st), (c, name, stats[c], st)
        total += len(got)
    if packet_rows:
        for what in ("read_packets_all", "read_events_all"):
            (o1, r1, v1), (o2, r2, v2) = getattr(bank, what)(), getattr(twin, what)()
            assert np.array_equal(o1, o2) and r1.tobytes() == r2.tobytes() and np.array_equal(v1, v2) and not v1.any(), what
            for c, (name, inv) in enumerate(plan):
                want = RC.expected(O, name, fb, inv)[3 if what == "read_packets_all" else 4]
                assert np.array_equal(r1[o1[c]:o1[c + 1]], want), (c, name, what)
    return total


def run_plan(B, O, fb, nch, width, seed, msg_cap=64, su_cap=700, noise_every=7):
    plan = RC.channel_plan(nch, fb, noise_every)
    streams = [RC.stream(name, fb, inv) for name, inv in plan]
    bank, twin = (B.AeroLBank(nch, fb, max_softbits_per_write=width, su_capacity=su_cap, burst=True) for _ in range(2))
    bank.rt_enable(msg_cap)
    feed([bank, twin], streams, width, np.random.default_rng(seed))
    return bank, twin, plan


@pytest.mark.parametrize("layout,width", [("wave", 3000), ("lanes", 2996)])
def test_10500_bps_both_viterbi_layouts(B, oracle_mod, force_viterbi_layout, layout, width):
    """70 channels, two wave groups with the last one partial; every case with arm inversions, every seventh channel noise only; rows of
    3000 entries are 16-byte aligned (the walk takes eight at a time), rows of 2996 are not."""
    force_viterbi_layout(layout)
    fb, nch = 10500, 70
    bank, twin, plan = run_plan(B, oracle_mod, fb, nch, width, 5)
    assert len({inv for _, inv in plan}) >= 3
    assert check_bank(bank, twin, plan, fb, oracle_mod) >= 300
    bank.close(); twin.close()


@pytest.mark.parametrize("fb,nch,width", [(1200, 66, 2500), (600, 20, 2504)])
def test_600_and_1200_bps(B, oracle_mod, fb, nch, width):
    """The unit sent with a wrong CRC is fed, the last unit sent is not (case t_msk); width 2500: single loads in the walk, 2504: groups of eight."""
    bank, twin, plan = run_plan(B, oracle_mod, fb, nch, width, fb)
    assert check_bank(bank, twin, plan, fb, oracle_mod) >= 80
    bank.close(); twin.close()


def test_a_packet_log_without_room_loses_no_message(B, K, oracle_mod):
    """su_capacity = 2: the packet log overflows at once, every message still completes (the bytes come from the decoded bits, not the log)."""
    fb, nch = 10500, 9
    bank, twin, plan = run_plan(B, oracle_mod, fb, nch, 3000, 8, su_cap=2, noise_every=0)
    assert check_bank(bank, twin, plan, fb, oracle_mod, packet_rows=False) >= 60
    with pytest.raises(K.JaeroError) as e:
        bank.read_packets(0)
    assert e.value.code == K.E_OVERFLOW
    bank.close(); twin.close()


def test_a_full_message_log_drops_rows_and_keeps_counting(B, K, oracle_mod):
    """msg_capacity = 3 where channels complete more: the first three rows, overflow bit 8 (the per-channel reader says JAERO_EOVERFLOW), the
    counters complete."""
    fb, nch = 10500, 9
    bank, twin, plan = run_plan(B, oracle_mod, fb, nch, 3000, 9, msg_cap=3, noise_every=0)
    full = [c for c, (name, inv) in enumerate(plan) if len(RC.expected(oracle_mod, name, fb, inv)[0]) > 3]
    assert len(full) >= 4
    buf, n = np.zeros(8, dtype=acars.MSG_DTYPE), C.c_int(0)
    probe = B.AeroLBank(1, fb, max_softbits_per_write=3000, su_capacity=700, burst=True)
    probe.rt_enable(3)
    name, inv = plan[full[0]]
    feed([probe], [RC.stream(name, fb, inv)], 3000)
    assert probe.L.jaero_aerol_read_msgs(probe.h, 0, buf.ctypes.data, 8, C.byref(n)) == K.E_OVERFLOW and n.value == 3
    assert buf[:3].tobytes() == RC.expected(oracle_mod, name, fb, inv)[0][:3].tobytes()
    assert probe.L.jaero_aerol_read_msgs(probe.h, 0, buf.ctypes.data, 8, C.byref(n)) == K.E_OK and n.value == 0  # read and cleared
    probe.close()
    assert check_bank(bank, twin, plan, fb, oracle_mod, cap=3) == sum(min(3, len(RC.expected(oracle_mod, nm, fb, iv)[0])) for nm, iv in plan)
    bank.close(); twin.close()


def test_one_call_read_equals_the_twin(B, K, oracle_mod):
    """257 channels (a second sweep workgroup holding one channel), a third of them empty, against a twin bank read channel by channel; a
    caprows in the middle takes a prefix, the next call the rest; capacity 5 overflows the log of the channels that complete more."""
    fb, nch, cap = 10500, 257, 5
    names = ("r_acars", "t_basic", "mixed")  # 4, 5 and 4 messages: a log of five holds them
    over = "r_keys"                          # 12 messages: overflowed on purpose, on one channel
    plan = [("noise", (False, False)) if c % 3 == 1 else ((over if c == 30 else names[(c // 3) % 3]), (False, False)) for c in range(nch)]
    streams = [RC.stream(name, fb, inv) for name, inv in plan]
    one, twin = (B.AeroLBank(nch, fb, max_softbits_per_write=4096, su_capacity=64, burst=True) for _ in range(2))
    for b in (one, twin):
        b.rt_enable(cap)
    feed([one, twin], streams, 4096)
    rows, ov = [], []
    for c in range(nch):
        buf, n = np.zeros(16, dtype=acars.MSG_DTYPE), C.c_int(0)
        rc = twin.L.jaero_aerol_read_msgs(twin.h, c, buf.ctypes.data, 16, C.byref(n))
        assert rc in (K.E_OK, K.E_OVERFLOW)
        rows.append(buf[: n.value].copy())
        ov.append(rc == K.E_OVERFLOW)
        want = RC.expected(oracle_mod, plan[c][0], fb)[0][:cap]
        assert rows[-1].tobytes() == want.tobytes(), c
    ov, cnt = np.array(ov), np.array([len(r) for r in rows])
    assert list(np.flatnonzero(ov)) == [30] and (cnt[1::3] == 0).all() and cnt[30] == cap
    P = np.cumsum(cnt)
    mid = int(P[nch // 2]) + 1
    rc, off, got, taken, pending, o = one.read_all_raw(K.AEROL_MESSAGES, mid)
    assert taken == int((P <= mid).sum()) and 30 < taken < nch and pending == int(P[-1])
    assert np.array_equal(off[: taken + 1], np.concatenate([[0], P[:taken]])) and (off[taken:] == off[taken]).all()
    assert got.tobytes() == np.concatenate(rows[:taken]).tobytes()
    assert np.array_equal(o, ov) and rc == K.E_OVERFLOW
    off2, rest, o2 = one.read_msgs_all()
    assert np.array_equal(np.diff(off2), np.where(np.arange(nch) < taken, 0, cnt)) and rest.tobytes() == np.concatenate(rows[taken:]).tobytes()
    assert not o2.any()
    assert one.read_all_raw(K.AEROL_MESSAGES, 0)[4] == 0 and np.array_equal(one.rt_stats(), twin.rt_stats())
    one.close(); twin.close()


def test_enabled_between_two_bursts_then_disabled_and_a_twin_that_never_enables(B, K, oracle_mod):
    """Enabled between the two bursts of a two-burst T message (case t_basic's second message): its ISU was not seen, the SSUs of the second
    burst are missing.  Disabled again: nothing more is launched, the log stays readable.  The twin never enables: the same launches in the
    three kernel classes, none in slot 5, no extra memory, the readers refuse, and packets and events are bit for bit the same."""
    fb, nch = 10500, 70
    plan = [("t_basic", (bool(c & 1), bool(c & 2))) for c in range(nch)]
    streams = [RC.stream(name, fb, inv) for name, inv in plan]
    # behind the second packet (the first burst of the two-burst message), in its gap: every stream has the same packet lengths
    marks = np.flatnonzero(streams[0] == -1)
    cut = int(marks[2]) - 500
    assert all(np.array_equal(np.flatnonzero(s == -1), marks) for s in streams)
    on, plain = (B.AeroLBank(nch, fb, max_softbits_per_write=3000, su_capacity=700, burst=True) for _ in range(2))
    for b in (on, plain):
        b.profile_enable(True)
    feed([on, plain], streams, 3000, stop=[cut] * nch)
    assert extra(on) == 0 and on.profile2_read(5) == (0.0, 0)
    on.rt_enable(16)
    assert extra(on) >= 64 * 2 * (11 * 528 + 11 * 64 + 16 * 544) and not on.rt_stats().any()
    feed([on, plain], streams, 3000, start=[cut] * nch)
    # the restatement, enabled at the same place: packets 0 and 1 are not seen
    want = RO.Channel(fb)
    pk = RC.expected(oracle_mod, "t_basic", fb)[3]
    want.rows(pk[pk[:, 0] >= 2])
    wmsgs = want.take()
    assert len(want.missing) == 3 and len(wmsgs) == 3  # the three SSUs of the second burst; the three later messages
    off, rows, ovf = on.read_msgs_all()
    stats = on.rt_stats()
    for c in range(nch):
        assert rows[off[c]:off[c + 1]].tobytes() == wmsgs.tobytes() and np.array_equal(stats[c], want.stats), c
    for slot in (0, 1, 2):
        assert plain.profile2_read(slot)[1] == on.profile2_read(slot)[1] > 0
    assert plain.profile2_read(5) == (0.0, 0) and 0 < on.profile2_read(5)[1] < on.profile2_read(2)[1]
    assert extra(plain) == 0
    n, buf = C.c_int(0), np.zeros(4, dtype=acars.MSG_DTYPE)
    assert plain.L.jaero_aerol_read_msgs(plain.h, 0, buf.ctypes.data, 4, C.byref(n)) == K.E_INVAL
    assert plain.L.jaero_aerol_rt_stats(plain.h, buf.ctypes.data) == K.E_INVAL
    assert plain.L.jaero_aerol_isu_stats(on.h, buf.ctypes.data) == K.E_INVAL  # the P banks' counters stay the P banks'
    with pytest.raises(K.JaeroError) as e:
        plain.read_all_raw(K.AEROL_MESSAGES, 0)
    assert e.value.code == K.E_INVAL and extra(plain) == 0
    for what in ("read_packets_all", "read_events_all"):
        (o1, r1, v1), (o2, r2, v2) = getattr(on, what)(), getattr(plain, what)()
        assert np.array_equal(o1, o2) and r1.tobytes() == r2.tobytes() and np.array_equal(v1, v2) and len(r1) > nch
    # disabled: the next writes launch nothing in slot 5; the counters stand
    on.rt_enable(0)
    on.profile2_read(5, reset=True); on.profile2_read(2, reset=True)
    feed([on], streams, 3000, stop=[cut] * nch)
    assert on.profile2_read(5) == (0.0, 0) and on.profile2_read(2)[1] > 0 and np.array_equal(on.rt_stats(), stats)
    on.close(); plain.close()


def test_refusals(B, K):
    """A P bank and an fb = 8400 bank: JAERO_ENOTSUP and nothing allocated; a negative capacity: JAERO_EINVAL, before the kind of bank is
    looked at; jaero_aerol_isu_enable on a burst bank: still JAERO_ENOTSUP, now naming the call that does it."""
    for bank in (B.AeroLBank(2, 10500, max_softbits_per_write=4096), B.AeroLBank(2, 1200, max_softbits_per_write=4096), B.AeroLBank(2, 8400, max_softbits_per_write=4096)):
        assert bank.L.jaero_aerol_rt_enable(bank.h, 4) == K.E_NOTSUP and b"jaero_aerol_rt_enable" in bank.L.jaero_last_error() and extra(bank) == 0
        assert bank.L.jaero_aerol_rt_enable(bank.h, 0) == K.E_NOTSUP
        assert bank.L.jaero_aerol_rt_enable(bank.h, -1) == K.E_INVAL and extra(bank) == 0
        st = np.zeros((2, 8), np.int64)
        assert bank.L.jaero_aerol_rt_stats(bank.h, st.ctypes.data) == K.E_INVAL
        bank.close()
    for fb in (600, 1200, 10500):
        bank = B.AeroLBank(2, fb, max_softbits_per_write=4096, burst=True)
        assert bank.L.jaero_aerol_rt_enable(bank.h, -1) == K.E_INVAL and extra(bank) == 0
        assert bank.L.jaero_aerol_isu_enable(bank.h, 4) == K.E_NOTSUP and b"jaero_aerol_rt_enable" in bank.L.jaero_last_error() and extra(bank) == 0
        bank.rt_enable(0)  # disabling what was never enabled allocates nothing
        assert extra(bank) == 0
        bank.rt_enable(4)
        first = extra(bank)
        bank.rt_enable(4); bank.rt_enable(0)
        assert extra(bank) == first > 0
        bank.rt_enable(9)
        assert extra(bank) == first + 64 * 5 * 544  # two channels are one wave group of 64; the log alone is allocated anew
        assert bank.L.jaero_aerol_isu_enable(bank.h, 4) == K.E_NOTSUP
        bank.close()


def test_pcm_to_acars_text_on_the_device(B):
    """R and T packets carrying ACARS blocks -> burst OQPSK passband PCM -> burst demodulator bank -> the emitted soft bits stay in HBM ->
    burst Aero-L bank with rt_enable -> parse_msg / AcarsDefragmenter.  Five channels, each sending one message in two blocks: block A (ETB)
    as an ISU and its SSUs in a T packet, block B (ETX) in two R packets.  The defragmented text is what was sent."""
    nch, n = 5, 48000 * 5
    uw = np.repeat(np.array([(AF.UW >> (31 - k)) & 1 for k in range(32)], dtype=np.uint8), 2)
    texts = [[f"CH{c} DOWNLINK REPORT {'KLMNO'[c] * (1 + c)} /", f"{c}Z"] for c in range(nch)]
    pcm = np.zeros((nch, n), np.int16)
    # (Eb/N0, noise seed) per channel at which the reference's burst demodulator acquires all three bursts: it loses most bursts of a
    # synthetic signal at any Eb/N0 -- its property, the same in the oracle's restatement -- and a lost burst is a lost block
    runs = [(16.0, 608), (16.0, 606), (16.0, 605), (14.0, 610), (16.0, 608)]
    for c in range(nch):
        reg, aes = f".A6-ED{'YZXWV'[c]}", 0x896000 + c
        ua = acars.acars_userdata(reg, "2", "\x15", "H1", "A", texts[c][0], more=True)
        ub = acars.acars_userdata(reg, "2", "\x15", "H1", "B", texts[c][1])
        units = acars.isu_payloads(aes, 0x90, 1 + c, 3, ua)
        pk = [("T", p) for p in acars.t_packets(aes, 0x90, units, len(units))] + [("R", p) for p in acars.r_isu_payloads(aes, 0x90, 1 + c, 4, ub)]
        assert [k for k, _ in pk] == ["T", "R", "R"]
        data = [np.concatenate([uw, AF.rt_packet_bits(k, p)]) for k, p in pk]
        pcm[c], _ = G.burst_oqpsk(n, burst_starts=[40000 + 777 * c, 100000 + 555 * c, 185000], ndata_sym=900, fc=8000.0 + 15.0 * c, ebno_db=runs[c][0],
                                  seed=G.SEED_BASE + runs[c][1], data=data)
    chunk = 4096
    demod = B.DemodulatorBank(B.BurstOqpskSettings(), nch, device=0, max_write_samples=chunk, softbit_capacity=16384)
    aerol = B.AeroLBank(nch, 10500, max_softbits_per_write=16384, su_capacity=400, burst=True)
    aerol.rt_enable(8)
    defrag = [acars.AcarsDefragmenter() for _ in range(nch)]
    out = [[] for _ in range(nch)]
    for s in range(0, n, chunk):
        demod.write(pcm[:, s:s + chunk])
        aerol.write_from_bank(demod, 4096)
        off, rows, ovf = aerol.read_msgs_all()
        assert not ovf.any()
        for c in range(nch):
            for r in rows[off[c]:off[c + 1]]:
                it = acars.parse_msg(r, downlink=True)
                assert it.valid and not it.nonacars and it.downlink, (c, it.error)
                whole = defrag[c].push(it)
                if whole is not None:
                    out[c].append(whole)
    for c in range(nch):
        assert [(w.message, chr(w.BI), w.PLANEREG, w.aesid, w.downlink) for w in out[c]] == [
            ("".join(texts[c]), "B", f".A6-ED{'YZXWV'[c]}".encode(), 0x896000 + c, True)], c
    assert aerol.rt_stats()[:, [3, 6]].tolist() == [[1, 1]] * nch
    aerol.close(); demod.close()
