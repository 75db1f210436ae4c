"""GPU (-m gpu): the ISU reassembly of an Aero-L bank (jaero_aerol_isu_enable, jaero_amd/csrc/k_aerol_isu.h) against the definition as
tests/isu_oracle.py states it, over the case streams of tests/isu_cases.py: message rows, counters, both post kernels, the jumping 10.5 kbps
walk, the one-call read, enabling and disabling, and the chain from PCM to defragmented ACARS text.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import isu_cases as IC
import isu_oracle as IO
from conftest import bank_settings, load_golden
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


def feed(banks, streams, width, rng=None):
    """Ragged per-channel counts in every write (rng) or full-width writes."""
    nch = len(streams)
    lens = np.array([len(s) for s in streams])
    pos = np.zeros(nch, dtype=np.int64)
    while (pos < lens).any():
        cnt = np.minimum(width if rng is None else rng.integers(1, width, size=nch), lens - pos).astype(np.int32)
        buf = np.zeros((nch, width), np.int16)
        for c in range(nch):
            buf[c, :cnt[c]] = streams[c][pos[c]:pos[c] + cnt[c]]
        for b in banks:
            b.write(buf, cnt)
        pos += cnt


def check_bank(bank, plan, fb, O, su_rows=True):
    """Messages (one call for all channels), counters and -- the feature changes neither -- signal units and events, per channel."""
    off, rows, ovf = bank.read_msgs_all()
    stats = bank.isu_stats()
    assert not ovf.any()
    total = 0
    for c, (name, inv, lead) in enumerate(plan):
        msgs, st, missing, sus, ev = IC.expected(O, name, fb, inv, lead)
        got = rows[off[c]:off[c + 1]]
        assert len(got) == len(msgs) and got.tobytes() == msgs.tobytes(), (c, name)
        assert np.array_equal(stats[c], st), (c, name, stats[c], st)
        if su_rows:
            assert np.array_equal(bank.read_sus(c), sus) and np.array_equal(bank.read_events(c), ev), (c, name)
        total += len(got)
    return total


@pytest.mark.parametrize("width", [700, 6000])
@pytest.mark.parametrize("layout", ["wave", "lanes"])
def test_1200_bps_both_post_kernels(B, oracle_mod, force_viterbi_layout, layout, width):
    """70 channels, ragged counts; width 700 is less than a block per write.  "lanes" makes the bank keep its decoded bits packed
    (k_aerol_post_packed in front of k_aerol_isu), "wave" one per byte (k_aerol_post)."""
    fb, nch = 1200, 70
    force_viterbi_layout(layout)
    plan = IC.channel_plan(nch, fb)
    bank = B.AeroLBank(nch, fb, max_softbits_per_write=width, su_capacity=500)
    bank.isu_enable(16)
    feed([bank], [IC.stream(*((n, fb) + (i, l))) for n, i, l in plan], width, np.random.default_rng(width))
    assert check_bank(bank, plan, fb, oracle_mod) >= 20 * (nch // 4)
    bank.close()


def test_10500_bps_jumping_walk(B, oracle_mod):
    """12 channels, 26 units per frame, every combination of arm inversions, garbage prefixes: k_aerol_scan / k_aerol_bits<true> / k_aerol_bulk."""
    fb, nch = 10500, 12
    plan = IC.channel_plan(nch, fb)
    assert len({inv for _, inv, _ in plan}) >= 3
    bank = B.AeroLBank(nch, fb, max_softbits_per_write=6000, su_capacity=500)
    bank.isu_enable(16)
    feed([bank], [IC.stream(n, fb, i, l) for n, i, l in plan], 6000, np.random.default_rng(3))
    assert check_bank(bank, plan, fb, oracle_mod) >= 60
    bank.close()


def test_600_bps_and_a_signal_unit_log_without_room(B, K, oracle_mod):
    """20 channels; the signal-unit log holds 8 rows and overflows at once: the reassembly sees every unit all the same."""
    fb, nch = 600, 20
    plan = IC.channel_plan(nch, fb)
    bank = B.AeroLBank(nch, fb, max_softbits_per_write=2500, su_capacity=8)
    bank.isu_enable(16)
    feed([bank], [IC.stream(n, fb, i, l) for n, i, l in plan], 2500, np.random.default_rng(6))
    assert check_bank(bank, plan, fb, oracle_mod, su_rows=False) >= 100
    with pytest.raises(K.JaeroError) as e:
        bank.read_sus(0)
    assert e.value.code == K.E_OVERFLOW
    bank.close()


def test_the_off_air_recording(B):
    """The soft bits the reference's demodulator made of its own recording, through a 10 500 bps bank: the ten messages."""
    soft = load_golden("recording_oqpsk_10k5")["soft"]
    bank = B.AeroLBank(1, 10500, max_softbits_per_write=8192, su_capacity=600)
    bank.isu_enable(32)
    for s in range(0, len(soft), 8192):
        bank.write(soft[None, s:s + 8192])
    msgs = bank.read_msgs(0)
    assert [(int(m["aesid"]), int(m["gesid"]), int(m["qno"]), int(m["refno"]), int(m["nbytes"])) for m in msgs] == IC.RECORDING_MESSAGES
    items = [acars.parse_msg(m) for m in msgs]
    assert [it.PLANEREG for it in items if not it.nonacars] == IC.RECORDING_REGS and all(it.valid for it in items)
    assert list(bank.isu_stats()[0, 2:]) == [0, 10]
    bank.close()


def noise(fb, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.round(128 + rng.normal(0, 45, 7000)), 0, 255).astype(np.int16)


@pytest.mark.parametrize("cap", [16, 5])
def test_one_call_read_equals_the_twin(B, K, oracle_mod, cap):
    """257 channels (a second sweep workgroup holding one channel), a third of them noise only, against a twin bank read channel by
    channel.  cap 16: a caprows in the middle takes a prefix, the next call the rest.  cap 5: every signal channel completes more than
    the log holds -- JAERO_EOVERFLOW, overflowed[] says where, the rows that fitted are the first five."""
    fb, nch = 1200, 257
    names = ("quirks", "acars")
    streams = [noise(fb, c) if c % 3 == 1 else IC.stream(names[(c // 3) % 2], fb) for c in range(nch)]
    one, twin = (B.AeroLBank(nch, fb, max_softbits_per_write=6000, su_capacity=8) for _ in range(2))
    for b in (one, twin):
        b.isu_enable(cap)
    feed([one, twin], streams, 6000)
    rows, ov = [], []
    for c in range(nch):
        buf = np.zeros(64, dtype=acars.MSG_DTYPE)
        n = C.c_int(0)
        rc = twin.L.jaero_aerol_read_msgs(twin.h, c, buf.ctypes.data, 64, C.byref(n))
        assert rc in (K.E_OK, K.E_OVERFLOW)
        rows.append(buf[: n.value].copy())
        ov.append(rc == K.E_OVERFLOW)
        want = [] if c % 3 == 1 else IC.expected(oracle_mod, names[(c // 3) % 2], fb)[0][:cap]
        assert len(rows[-1]) == len(want) and rows[-1].tobytes() == (want.tobytes() if len(want) else b""), c
    ov = np.array(ov)
    cnt = np.array([len(r) for r in rows])
    assert ov.any() == (cap == 5) and (cnt[1::3] == 0).all() and np.array_equal(ov, (cnt == cap) if cap == 5 else np.zeros(nch, bool))
    P = np.cumsum(cnt)
    mid = int(P[nch // 2]) + 1
    rc, off, got, taken, pending, o = one.read_all_raw(K.AEROL_MESSAGES, mid)
    etaken = int((P <= mid).sum())
    assert taken == etaken and 0 < taken < nch and pending == int(P[-1])
    assert np.array_equal(off[: taken + 1], np.concatenate([[0], P[:taken]])) and (off[taken:] == off[taken]).all()
    assert got.tobytes() == np.concatenate(rows[:taken]).tobytes()
    eo = ov.copy(); eo[taken:] = False
    assert np.array_equal(o, eo) and rc == (K.E_OVERFLOW if eo.any() else K.E_OK)
    off2, rest, o2 = one.read_msgs_all()
    assert np.array_equal(np.diff(off2), np.where(np.arange(nch) < taken, 0, cnt)) and rest.tobytes() == np.concatenate(rows[taken:]).tobytes()
    eo2 = ov.copy(); eo2[:taken] = False
    assert np.array_equal(o2, eo2)
    assert one.read_all_raw(K.AEROL_MESSAGES, 0)[4] == 0 and np.array_equal(one.isu_stats(), twin.isu_stats())
    one.close(); twin.close()


def test_enabled_in_mid_stream_it_starts_empty(B, oracle_mod):
    """Enabled with half of the stream gone -- in the middle of a message: what was open is not known, its SSUs are missing."""
    fb = 1200
    soft = IC.stream("quirks", fb)
    cut = 6 * 1200 + 500
    bank = B.AeroLBank(1, fb, max_softbits_per_write=4096, su_capacity=500)
    a = oracle_mod.AeroL(fb)
    for s in range(0, cut, 4096):
        bank.write(soft[None, s:min(s + 4096, cut)])
        a.write(soft[s:min(s + 4096, cut)])
    a.take_sus(); a.take_events()
    bank.isu_enable(16)
    assert len(bank.read_msgs(0)) == 0 and not bank.isu_stats().any()
    chan, _, _ = IO.run_stream(oracle_mod, fb, soft[cut:], IO.Channel(), aerol=a)
    for s in range(cut, len(soft), 4096):
        bank.write(soft[None, s:s + 4096])
    want = chan.take()
    assert 0 < len(want) < len(IC.expected(oracle_mod, "quirks", fb)[0])
    assert bank.read_msgs(0).tobytes() == want.tobytes() and np.array_equal(bank.isu_stats()[0], chan.stats)
    # enabling again clears the list, the log and the counters once more
    bank.write(IC.stream("acars", fb)[None, :4096])
    bank.isu_enable(4)
    assert len(bank.read_msgs(0)) == 0 and not bank.isu_stats().any()
    bank.close()


def test_a_bank_that_never_enables_is_the_bank_it_was(B, K, oracle_mod):
    """Never enabled: the same launches in the three kernel classes as an enabled twin, none in slot 5, no extra memory, and the readers
    refuse.  Enabled: signal units and events bit for bit the plain bank's.  Disabled again: no further launch, the log stays readable."""
    fb, nch = 1200, 70
    plan = IC.channel_plan(nch, fb)
    streams = [IC.stream("quirks" if n in ("sizes", "tail") else n, fb, i, l) for n, i, l in plan]
    plain, on = (B.AeroLBank(nch, fb, max_softbits_per_write=2400, su_capacity=200) for _ in range(2))
    for b in (plain, on):
        b.profile_enable(True)
    on.isu_enable(16)
    feed([plain, on], streams, 2400)
    for slot in (0, 1, 2):
        assert plain.profile2_read(slot)[1] == on.profile2_read(slot)[1] > 0
    assert plain.profile2_read(5) == (0.0, 0) and on.profile2_read(5)[1] == on.profile2_read(2)[1]
    extra = lambda b: b.L.jaero_aerol_debug_extra_bytes(b.h)
    assert extra(plain) == 0 and extra(on) >= 64 * 2 * (11 * 528 + 16 * 544)
    for what in (K.AEROL_SUS, K.AEROL_EVENTS):
        (o1, r1, v1), (o2, r2, v2) = plain.read_all(what), on.read_all(what)
        assert np.array_equal(o1, o2) and r1.tobytes() == r2.tobytes() and np.array_equal(v1, v2) and len(r1) > nch
    n = C.c_int(0)
    buf = np.zeros(4, dtype=acars.MSG_DTYPE)
    swept = extra(plain)  # (the one-call reads above allocated the sweep's scratch; the refusals below allocate nothing)
    assert plain.L.jaero_aerol_read_msgs(plain.h, 0, buf.ctypes.data, 4, C.byref(n)) == K.E_INVAL
    assert plain.L.jaero_aerol_isu_stats(plain.h, buf.ctypes.data) == K.E_INVAL
    with pytest.raises(K.JaeroError) as e:
        plain.read_all_raw(K.AEROL_MESSAGES, 0)
    assert e.value.code == K.E_INVAL and extra(plain) == swept
    assert plain.L.jaero_aerol_isu_enable(plain.h, -1) == K.E_INVAL and extra(plain) == swept
    # disabled: the next writes launch nothing in slot 5; what the log holds can still be read
    before = on.isu_stats()
    on.isu_enable(0)
    on.profile2_read(5, reset=True); on.profile2_read(2, reset=True)
    feed([on], streams[:nch], 2400)
    assert on.profile2_read(5) == (0.0, 0) and on.profile2_read(2)[1] > 0 and np.array_equal(on.isu_stats(), before)
    off, rows, ovf = on.read_msgs_all()
    assert len(rows) == sum(len(IC.expected(oracle_mod, "quirks" if n in ("sizes", "tail") else n, fb, i, l)[0]) for n, i, l in plan)
    plain.close(); on.close()
    # banks the reference has no ISUData for
    for bank in (B.AeroLBank(2, 10500, max_softbits_per_write=4096, burst=True), B.AeroLBank(2, 8400, max_softbits_per_write=4096)):
        assert bank.L.jaero_aerol_isu_enable(bank.h, 4) == K.E_NOTSUP and extra(bank) == 0
        assert bank.L.jaero_aerol_isu_enable(bank.h, -1) == K.E_INVAL
        bank.close()


def test_pcm_to_acars_text_on_the_device(B):
    """PCM -> a 1200 bps MSK bank -> an Aero-L bank with link_dcd -> messages.  Five channels, each carrying one ACARS message in three blocks
    (ETB, ETB, ETX; block ids A, B, C) behind three frames of fill-in units; the defragmented text is what was sent."""
    fb, nch = 1200, 5
    texts = [[f"CH{c} BLOCK ONE /", f" TWO {'ABCDEFG'[c] * (3 + c)} /", f" THREE {c * 1111}"] for c in range(nch)]
    pcms = []
    for c in range(nch):
        units = [IC.FILL] * 18
        for k, t in enumerate(texts[c]):
            u = acars.acars_userdata(f".A6-ED{'YZXWV'[c]}", "2", "\x15", "H1", "ABC"[k], t, more=k < 2)
            units += acars.isu_payloads(0x896000 + c, 0x90, 1 + c, k, u) + [IC.FILL]
        bits, _ = AF.p_channel_bits(IC.frames_of(units, fb) + [[IC.FILL] * 6] * 2, fb)
        n = int(len(bits) * 48000 / 1200) + 4000
        pcms.append(G.msk(n, fb=1200.0, fc=1007.0, ebno_db=16.0, seed=31 + c, bits=np.concatenate([bits, np.zeros(16, np.uint8)]))[0])
    n = min(len(p) for p in pcms)
    pcm = np.stack([p[:n] for p in pcms])
    chunk = 24000
    demod = B.DemodulatorBank(bank_settings("msk", {}), nch, device=0, max_write_samples=chunk, softbit_capacity=8192)
    aerol = B.AeroLBank(nch, fb, max_softbits_per_write=8192)
    aerol.isu_enable(8)
    aerol.link_dcd(demod)
    defrag = [acars.AcarsDefragmenter() for _ in range(nch)]
    out = [[] for _ in range(nch)]
    for s in range(0, n, chunk):
        demod.write(pcm[:, s:s + chunk])
        aerol.write_from_bank(demod, 8192)
        off, rows, ovf = aerol.read_msgs_all()
        assert not ovf.any()
        for c in range(nch):
            for r in rows[off[c]:off[c + 1]]:
                it = acars.parse_msg(r)
                assert it.valid and not it.nonacars, (c, it.error)
                whole = defrag[c].push(it)
                if whole is not None:
                    out[c].append(whole)
    for c in range(nch):
        assert [(w.message, chr(w.BI), w.PLANEREG, w.aesid) for w in out[c]] == [("".join(texts[c]), "C", f".A6-ED{'YZXWV'[c]}".encode(), 0x896000 + c)], c
    assert aerol.isu_stats()[:, 3].tolist() == [3] * nch
    aerol.close(); demod.close()
