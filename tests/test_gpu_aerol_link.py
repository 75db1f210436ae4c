"""GPU (-m gpu): jaero_aerol_link_dcd, the device wire from the Aero-L bank's DataCarrierDetect emissions to the demodulator bank's dcd.

The reference of every case is a closed-loop oracle assembled here, per channel and write: demodulator.write(pcm); all of take_soft() goes
into AeroL.write; the last kind-0 row of take_events(), if any, goes to set_dcd before the next write; tick_dcd() where the test ticks, its
emission applied by the same rule.  The GPU chain hands the Aero-L bank the soft bits in the reference's groups (32 / 12, what take_soft()
holds: the Qt adaptors' behaviour the link is defined by) and never touches dcd from the host.

Tolerances are the bank tests' own (tests/test_gpu_parity.py compare()): hard bits equal; soft bytes |d| <= 1 and counted
(conftest.assert_soft_bytes, none allowed); status rows' sample index and signal flag equal, freq_est / freq_center / mse within 1e-6;
signal units and Aero-L events exact.

Each case also shows on the CPU that it can fail: the closed loop and the open loop (dcd never set) of the oracle differ in the compared
quantity for at least one of its signals."""
import numpy as np
import pytest

from conftest import assert_soft_bytes, bank_settings, oracle_settings
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


# ---------------------------------------------------------------------------------------------- the closed-loop oracle
def oracle_chain(O, settings, afc, fb, pcm, writes, tick_every=0, closed=True, dcd0=None):
    """One channel: returns dict(soft, status, sus, events, dcd) of the chain fed `pcm` in the given write sizes."""
    d = O.Demod(settings, afc=afc)
    a = O.AeroL(fb)
    a.take_events()  # the constructor's DataCarrierDetect(false): before any link, not replayed
    if dcd0 is not None:
        d.set_dcd(dcd0)
    soft, events, pos, next_tick, dcd = [], [], 0, tick_every, []

    def apply(ev):
        events.append(ev)
        k0 = ev[ev[:, 1] == 0] if len(ev) else ev
        if closed and len(k0):
            d.set_dcd(bool(k0[-1, 2]))

    for n in writes:
        if pos >= len(pcm):
            break
        d.write(pcm[pos:pos + n])
        pos += n
        s = d.take_soft()
        soft.append(s)
        a.write(s)
        apply(a.take_events())
        while tick_every and pos >= next_tick:
            a.tick_dcd()
            apply(a.take_events())
            next_tick += tick_every
    out = dict(soft=np.concatenate(soft), status=d.take_status(), sus=a.take_sus(), events=np.concatenate(events), freq_center=d.freq_center)
    if fb == 8400:
        out["voice"] = a.take_voice()
    return out


def oracle_chains(jobs):
    """oracle_chain for every argument tuple of `jobs`, on a few threads (every oracle object is its own; the calls release the GIL)."""
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(8) as ex:
        return list(ex.map(lambda j: oracle_chain(*j), jobs))


def cycle(sizes, total):
    out, k, s = [], 0, 0
    while s < total:
        out.append(sizes[k % len(sizes)])
        s += out[-1]
        k += 1
    return out


class Handoff:
    """Hands a continuous bank's soft bits to an Aero-L bank in the reference's groups (what the oracle's take_soft() holds after a write);
    the rest waits for the next write, as in the Qt adaptors."""

    def __init__(self, demod, aerol, group):
        self.demod, self.aerol, self.group, self.nch = demod, aerol, group, demod.nch
        self.pend = [np.zeros(0, np.int16) for _ in range(self.nch)]
        self.soft = [[] for _ in range(self.nch)]

    def step(self):
        buf, cnt = self.demod.read_softbits_all(8192)
        out = np.zeros((self.nch, 8192), np.int16)
        ocnt = np.zeros(self.nch, np.int32)
        for c in range(self.nch):
            x = np.concatenate([self.pend[c], buf[c, :cnt[c]]])
            k = len(x) // self.group * self.group
            out[c, :k] = x[:k]
            ocnt[c] = k
            self.pend[c] = x[k:]
            self.soft[c].append(x[:k])
        self.aerol.write(out, ocnt)


def gpu_chain(B, settings, nch, afc_mask, fb, group, pcm, writes, tick_every=0, link=True, max_write=24000):
    """The bank chain; returns per channel (soft, status, sus, events) and the banks' final dcd-independent state."""
    demod = B.DemodulatorBank(settings, nch, device=0, status_log=True, max_write_samples=max_write, softbit_capacity=1 << 17)  # (the status log's room follows it)
    aerol = B.AeroLBank(nch, fb, max_softbits_per_write=8192, su_capacity=26 * 16)
    for c in range(nch):
        if afc_mask[c]:
            demod.set_flags(afc=True, channel=c)
    aerol.read_events_all()  # the constructor's row
    if link:
        aerol.link_dcd(demod)
    hand = Handoff(demod, aerol, group)
    pos, next_tick, n = 0, tick_every, pcm.shape[1]
    for w in writes:
        if pos >= n:
            break
        demod.write(pcm[:, pos:pos + w])
        pos += w
        hand.step()
        while tick_every and pos >= next_tick:
            aerol.tick_dcd()
            next_tick += tick_every
    soft = hand.soft
    off_s, sus, _ = aerol.read_sus_all()
    off_e, ev, ovf = aerol.read_events_all()
    assert not ovf.any()
    if fb == 8400:
        off_v, vrows, _ = aerol.read_voice_all()
    res = []
    for c in range(nch):
        res.append(dict(soft=np.concatenate(soft[c]), status=demod.read_status_log(c, 1 << 14), sus=sus[off_s[c]:off_s[c + 1]], events=ev[off_e[c]:off_e[c + 1]],
                        freq_center=demod.read_status(c).freq_center))
        if fb == 8400:
            v = vrows[off_v[c]:off_v[c + 1]]
            res[-1]["voice"] = (v[:, :4].copy().view(np.uint32).reshape(-1), v[:, 4:])
    aerol.close()
    demod.close()
    return res


def same(got, ref, allow=0):
    """compare() of tests/test_gpu_parity.py on the chain's outputs; returns None or what differs."""
    try:
        assert len(got["soft"]) == len(ref["soft"]), "soft length"
        assert np.array_equal(got["soft"] >= 128, ref["soft"] >= 128), "hard decisions differ"
        assert_soft_bytes(got["soft"], ref["soft"], allow=allow)
        assert got["status"].shape == ref["status"].shape, "status rows"
        if len(ref["status"]):
            assert np.array_equal(got["status"][:, [0, 5]], ref["status"][:, [0, 5]]), "status index / signal"
            assert np.max(np.abs(got["status"][:, 1:4] - ref["status"][:, 1:4])) < 1e-6, "freq_est / freq_center / mse"
        assert np.array_equal(got["sus"], ref["sus"]), "signal units"
        assert np.array_equal(got["events"], ref["events"]), "Aero-L events"
        if "voice" in ref:
            assert np.array_equal(got["voice"][0], ref["voice"][0]) and np.array_equal(got["voice"][1], ref["voice"][1]), "voice frames"
    except AssertionError as e:
        return str(e)[:200]
    return None


def differ(a, b):
    """The oracle's closed and open loops differ in a compared quantity (beyond the tolerance)."""
    if len(a["soft"]) != len(b["soft"]) or (a["soft"] != b["soft"]).any():
        return True
    if a["status"].shape != b["status"].shape or (len(a["status"]) and np.max(np.abs(a["status"][:, 1:4] - b["status"][:, 1:4])) >= 1e-6):
        return True
    return not (np.array_equal(a["sus"], b["sus"]) and np.array_equal(a["events"], b["events"]))


# ---------------------------------------------------------------------------------------------- case 1: OQPSK 10.5k
NFR = 12
NTOTAL = 436000


def oqpsk_signals():
    """Four signals x AFC off / on: the 12-frame signal; one starting after 2 s of noise; one ending after 3 s, followed by noise;
    noise only."""
    fb = 10500
    sig = []
    for k in range(4):
        pay = AF.random_payloads(NFR, fb, seed=50 + k)
        bits, _ = AF.p_channel_bits(pay, fb)
        n = int(len(bits) / 2 * 48000 / 5250) + 2000
        pcm, _ = G.oqpsk(n, fc=8000.0 + 11.0 * k, ebno_db=13.0, seed=70 + k, bits=np.concatenate([bits, np.zeros(64, np.uint8)]))
        # 9 s in all: six ticks of the 1 s timer behind the end of the signal that stops after 3 s, what its carrier detect needs to drop
        noise = np.clip(np.round(np.random.default_rng(90 + k).normal(0.0, 0.1 * 32768 * 0.3, NTOTAL)), -32768, 32767).astype(np.int16)
        if k == 0:
            pcm = np.concatenate([pcm, noise[len(pcm):]])
        elif k == 1:
            pcm = np.concatenate([noise[:96000], pcm, noise[96000 + len(pcm):]])
        elif k == 2:
            pcm = np.concatenate([pcm[:144000], noise[144000:]])
        else:
            pcm = noise
        sig.append(pcm)
    return sig


@pytest.fixture(scope="module")
def case1(oracle_mod):
    sig = oqpsk_signals()
    n = len(sig[0])
    return dict(sig=sig, n=n)


@pytest.mark.parametrize("pattern", ["even", "ragged"])
def test_oqpsk_chain_follows_the_closed_loop(B, oracle_mod, case1, pattern):
    """70 channels (two wavefront groups, the second ragged): linked chain = closed-loop oracle on every channel.  The same chain unlinked
    -- its first 8 channels, one of each signal and AFC setting, to keep the test short -- fails the same comparison: without the feature
    this test fails.  Both write patterns show on the CPU that the oracle's closed and open loops differ."""
    nch, n = 70, case1["n"]
    writes = cycle([24000] if pattern == "even" else [9000, 24000, 1, 4097], n)
    kinds = [(c % 4, bool((c // 4) & 1)) for c in range(nch)]
    pcm = np.stack([case1["sig"][k] for k, _ in kinds])
    O, uniq = oracle_mod, sorted(set(kinds))
    job = lambda kd, closed: (O, oracle_settings(O, "oqpsk", {}), kd[1], 10500, case1["sig"][kd[0]], writes, 48000, closed)
    ref = dict(zip(uniq, oracle_chains([job(kd, True) for kd in uniq])))
    assert len(uniq) == 8
    k0 = ref[(2, False)]["events"]
    assert k0[k0[:, 1] == 0][-1, 2] == 0, "the carrier detect of the signal that ends does not drop"
    opened = oracle_chains([job(kd, False) for kd in uniq[:2]])  # the 12-frame signal (DESIGN.md section 19's oracle runs), AFC off and on
    assert any(differ(ref[kd], o) for kd, o in zip(uniq, opened)), "the oracle's closed and open loops agree: this case cannot fail"
    got = gpu_chain(B, bank_settings("oqpsk", {}), nch, [a for _, a in kinds], 10500, 32, pcm, writes, tick_every=48000)
    bad = {c: same(got[c], ref[kinds[c]]) for c in range(nch)}
    assert not any(bad.values()), {c: v for c, v in bad.items() if v}
    assert sum(int(r["sus"][:, 14].sum()) for r in got if len(r["sus"])) > 26 * 6 * nch // 4
    unlinked = gpu_chain(B, bank_settings("oqpsk", {}), 8, [a for _, a in kinds[:8]], 10500, 32, pcm[:8], writes, tick_every=48000, link=False)
    assert any(same(unlinked[c], ref[kinds[c]]) for c in range(8)), "the unlinked chain passes too"


# ---------------------------------------------------------------------------------------------- case 2: MSK 1200
def msk_signals():
    sig = []
    for nfr, seed in ((4, 31), (6, 33)):
        bits, _ = AF.p_channel_bits(AF.random_payloads(nfr, 1200, seed=9 + nfr), 1200)
        n = int(len(bits) * 48000 / 1200) + 4000
        sig.append(G.msk(n, fb=1200.0, fc=1007.0, ebno_db=16.0, seed=seed, bits=np.concatenate([bits, np.zeros(16, np.uint8)]))[0])
    n = max(len(s) for s in sig)
    return [np.concatenate([s, np.zeros(n - len(s), np.int16)]) for s in sig]


def test_msk_chain_follows_the_closed_loop(B, oracle_mod):
    """MSK 1200 at 48 kHz, 70 channels, AFC on for half: the AFC clause is `afc && dcd` (mskdemodulator.cpp:498), so freq_center moves only
    when dcd arrives."""
    O = oracle_mod
    nch = 70
    sig = msk_signals()
    writes = cycle([9000], len(sig[0]))
    kinds = [(c % 2, bool((c // 2) & 1)) for c in range(nch)]
    uniq = sorted(set(kinds))
    ref = dict(zip(uniq, oracle_chains([(O, oracle_settings(O, "msk", {}), kd[1], 1200, sig[kd[0]], writes, 0, True) for kd in uniq])))
    opened = dict(zip(uniq, oracle_chains([(O, oracle_settings(O, "msk", {}), kd[1], 1200, sig[kd[0]], writes, 0, False) for kd in uniq])))
    assert any(differ(ref[kd], opened[kd]) for kd in ref), "the oracle's closed and open loops agree: this case cannot fail"
    moved = [kd for kd in ref if kd[1] and abs(ref[kd]["freq_center"] - opened[kd]["freq_center"]) > 1.0]
    assert moved, "freq_center does not follow dcd in the oracle"
    got = gpu_chain(B, bank_settings("msk", {}), nch, [a for _, a in kinds], 1200, 12, np.stack([sig[k] for k, _ in kinds]), writes, max_write=9000)
    bad = {c: same(got[c], ref[kinds[c]]) for c in range(nch)}
    assert not any(bad.values()), {c: v for c, v in bad.items() if v}
    for c in range(nch):
        assert abs(got[c]["freq_center"] - ref[kinds[c]]["freq_center"]) < 1e-6, c


# ---------------------------------------------------------------------------------------------- case 4: the 8400 bps C channel
# tests/test_gpu_parity.py: the 8400 bps prefilter is an FFT filter on both sides whose round-off differs; a soft byte on a rounding edge may
# differ by one, counted, at most this many per comparison (SILENCE_8400_ALLOW there)
SILENCE_8400_ALLOW = 2
O8 = {"fb": 8400.0, "lockingbw": 8400.0}


def c_channel_pcm(c, nfr=8):
    """8 C-channel frames (voice + three signal units each, AF.c_channel_bits) behind a few hundred random bits, as 8400 bps OQPSK passband."""
    rng = np.random.default_rng(7300 + c)
    frames = [(rng.integers(0, 256, 300, dtype=np.uint8), [bytes([0x22] + list(rng.integers(0, 256, 9, dtype=np.uint8))) for _ in range(3)])
              for _ in range(nfr)]
    bits = np.concatenate([rng.integers(0, 2, 200 + 300 * c, dtype=np.uint8), AF.c_channel_bits(frames), np.zeros(64, np.uint8)])
    n = int(len(bits) / 2 * 48000 / 4200) + 2000
    return G.oqpsk(n, fb=8400.0, fc=8000.0 + 9.0 * c, ebno_db=14.0, seed=7400 + c, bits=bits)[0]


def test_c_channel_chain_follows_the_closed_loop(B, oracle_mod):
    """8400 bps, 5 channels, AFC on for the odd ones, writes of 24 000 (one frame): PCM -> 8400 bps bank (prefilter, k_oqpsk_fb) -> C-channel
    Aero-L bank linked to it, against the closed-loop oracle: status log, soft bytes, signal units, voice frames, events."""
    O, nch = oracle_mod, 5
    sig = [c_channel_pcm(c) for c in range(nch)]
    n = min(len(x) for x in sig)
    pcm = np.stack([x[:n] for x in sig])
    writes = cycle([24000], n)
    job = lambda c, closed: (O, oracle_settings(O, "oqpsk", O8), bool(c & 1), 8400, pcm[c], writes, 48000, closed)
    ref = oracle_chains([job(c, True) for c in range(nch)])
    opened = oracle_chains([job(c, False) for c in range(nch)])
    assert any(differ(r, o) for r, o in zip(ref, opened)), "the oracle's closed and open loops agree: this case cannot fail"
    assert all(len(r["voice"][0]) >= 5 and int(r["sus"][:, 14].sum()) >= 9 for r in ref), "the oracle chain does not decode the frames"
    got = gpu_chain(B, bank_settings("oqpsk", O8), nch, [bool(c & 1) for c in range(nch)], 8400, 32, pcm, writes, tick_every=48000)
    bad = {c: same(got[c], ref[c], allow=SILENCE_8400_ALLOW) for c in range(nch)}
    assert not any(bad.values()), {c: v for c, v in bad.items() if v}
    unlinked = gpu_chain(B, bank_settings("oqpsk", O8), nch, [bool(c & 1) for c in range(nch)], 8400, 32, pcm, writes, tick_every=48000, link=False)
    assert any(same(unlinked[c], ref[c], allow=SILENCE_8400_ALLOW) for c in range(nch)), "the unlinked chain passes too"


# ---------------------------------------------------------------------------------------------- case 5: the interface
def test_link_interface(B, K, oracle_mod, case1):
    O = oracle_mod
    L = K.lib()
    nch = 3
    sig = case1["sig"][0][:5 * 24000]
    pcm = np.stack([sig] * nch)
    o8 = {"fb": 8400.0, "lockingbw": 8400.0}
    demod = B.DemodulatorBank(bank_settings("oqpsk", {}), nch, status_log=True, max_write_samples=24000, softbit_capacity=1 << 17)
    aerol = B.AeroLBank(nch, 10500, max_softbits_per_write=8192)
    other = B.AeroLBank(nch, 10500, max_softbits_per_write=8192)
    code = lambda f: pytest.raises(K.JaeroError, f).value.code
    # refused links, in the documented order where two faults meet
    four = B.AeroLBank(4, 1200, max_softbits_per_write=64)
    assert code(lambda: four.link_dcd(demod)) == K.E_INVAL and b"channels" in L.jaero_last_error()  # counts before fb
    slow = B.AeroLBank(nch, 1200, max_softbits_per_write=64)
    assert code(lambda: slow.link_dcd(demod)) == K.E_INVAL and b"bps" in L.jaero_last_error()
    bursty = B.AeroLBank(nch, 10500, max_softbits_per_write=64, burst=True)
    assert code(lambda: bursty.link_dcd(demod)) == K.E_INVAL and b"burst" in L.jaero_last_error()
    bo = B.DemodulatorBank(B.BurstOqpskSettings(), nch, max_write_samples=4096)
    assert code(lambda: bursty.link_dcd(bo)) == K.E_NOTSUP
    bm = B.DemodulatorBank(B.BurstMskSettings(), nch, max_write_samples=4096)
    bursty12 = B.AeroLBank(nch, int(bm.fb), max_softbits_per_write=64, burst=True)
    assert code(lambda: bursty12.link_dcd(bm)) == K.E_NOTSUP  # burst banks are not linked (include/jaero_hip.h)
    for x in (four, slow, bursty, bo, bm, bursty12):
        x.close()
    aerol.link_dcd(demod)
    assert code(lambda: other.link_dcd(demod)) == K.E_INVAL and b"already linked" in L.jaero_last_error()
    # a rate change that re-creates the bank is refused while linked, and the bank still works
    assert code(lambda: demod.set_settings(bank_settings("oqpsk", o8))) == K.E_INVAL and b"unlink" in L.jaero_last_error()
    # a stream mismatch consumes nothing
    import torch
    st = torch.cuda.Stream()
    fbits, _ = AF.p_channel_bits(AF.random_payloads(2, 10500, seed=5), 10500)
    framed = np.stack([AF.to_soft(fbits[:6000], sigma=5.0, seed=1)] * nch)  # holds a unique word: consumed, it would log events
    assert code(lambda: aerol.write(framed, stream=st.cuda_stream)) == K.E_INVAL and b"stream" in L.jaero_last_error()
    for what in (K.AEROL_EVENTS, K.AEROL_SUS):  # as many rows as the twin that was never written
        assert aerol.read_all_raw(what, 0)[4] == other.read_all_raw(what, 0)[4]
    other.write(framed)
    assert other.read_all_raw(K.AEROL_EVENTS, 0)[4] > aerol.read_all_raw(K.AEROL_EVENTS, 0)[4]  # (consumed, they do show)
    other.close()
    other = B.AeroLBank(nch, 10500, max_softbits_per_write=8192)
    # a write without an emission leaves the caller's dcd in place; the next emission overwrites it.  The oracle is told the same.
    orc = [O.Demod(oracle_settings(O, "oqpsk", {})) for _ in range(nch)]
    oa = [O.AeroL(10500) for _ in range(nch)]
    for a in oa:
        a.take_events()
    demod.set_dcd(True, channel=1)
    orc[1].set_dcd(True)
    quiet = np.full((nch, 64), 128, np.int16)
    aerol.write(quiet)  # erasures: no emission, so the caller's dcd of channel 1 stands through the first write of PCM
    for a in oa:
        a.write(quiet[0])
        assert len(a.take_events()) == 0
    saw_emission = False
    hand = Handoff(demod, aerol, 32)
    for w in range(5):
        seg = pcm[:, w * 24000:(w + 1) * 24000]
        demod.write(seg)
        hand.step()
        for c in range(nch):
            orc[c].write(seg[c])
            oa[c].write(orc[c].take_soft())
            ev = oa[c].take_events()
            k0 = ev[ev[:, 1] == 0] if len(ev) else ev
            if len(k0):
                orc[c].set_dcd(bool(k0[-1, 2]))
                saw_emission = True
        if w == 1:  # between emissions: the caller's word counts until the next one
            demod.set_dcd(False, channel=2)
            orc[2].set_dcd(False)
    assert saw_emission
    for c in range(nch):
        got, ref = demod.read_status_log(c), orc[c].take_status()
        assert got.shape == ref.shape and np.max(np.abs(got[:, 1:4] - ref[:, 1:4])) < 1e-6, c
    # unlink, then the rate change goes through and the bank carries the device's last dcd: the oracle that had it agrees
    aerol.unlink_dcd()
    other.link_dcd(demod)
    other.unlink_dcd()
    demod.set_settings(bank_settings("oqpsk", o8))  # 10500 -> 8400 bps: tests/test_gpu_parity.py::test_oqpsk_live_rate_change_carries_state_over's pair
    tail = case1["sig"][0][5 * 24000:7 * 24000]
    for t0 in (0, 24000):
        demod.write(np.stack([tail[t0:t0 + 24000]] * nch))
        demod.read_softbits_all(8192)
    for c in range(nch):
        orc[c].set_settings(oracle_settings(O, "oqpsk", o8))
        for t0 in (0, 24000):
            orc[c].write(tail[t0:t0 + 24000])
        got, ref = demod.read_status_log(c), orc[c].take_status()
        assert len(ref) > 4 and got.shape == ref.shape and np.max(np.abs(got[:, 1:4] - ref[:, 1:4])) < 1e-6, c
    # both orders of destruction
    d1 = B.DemodulatorBank(bank_settings("oqpsk", {}), nch, max_write_samples=4096)
    aerol.link_dcd(d1)
    d1.close()
    aerol.close()
    d2 = B.DemodulatorBank(bank_settings("oqpsk", {}), nch, max_write_samples=4096)
    other.link_dcd(d2)
    d2.write(np.zeros((nch, 64), np.int16), stream=st.cuda_stream)  # the bank moves to another stream: a tick there would race with it
    assert code(lambda: other.tick_dcd()) == K.E_INVAL and b"stream" in L.jaero_last_error()
    other.close()
    d2.close()
    demod.close()


# ---------------------------------------------------------------------------------------------- the wire itself, C channel
def c_streams(nch=5):
    streams = [AF.c_channel_case(7100 + c, 3 + c % 2, 10.0 + 4 * c, inv=(bool(c & 1), bool(c & 2)), lead=100 + 700 * c)[1] for c in range(nch)]
    streams[3] = np.clip(np.round(128 + np.random.default_rng(3).normal(0, 45, 9000)), 0, 255).astype(np.int16)
    return streams


def c_oracle_dcd(O, streams, width, nticks):
    """Per call (writes of `width`, then `nticks` ticks of the 1 s timer): the dcd each channel's last emission so far asks for (None: none yet)."""
    orc = [O.AeroL(8400) for _ in streams]
    want, calls = [None] * len(streams), []
    for a in orc:
        a.take_events()

    def note():
        for c, a in enumerate(orc):
            ev = a.take_events()
            k0 = ev[ev[:, 1] == 0] if len(ev) else ev
            if len(k0):
                want[c] = int(k0[-1, 2])
        calls.append(list(want))

    for s0 in range(0, max(len(s) for s in streams), width):
        for c, a in enumerate(orc):
            a.write(streams[c][s0:s0 + width])
        note()
    for _ in range(nticks):
        for a in orc:
            a.tick_dcd()
        note()
    return calls


def test_c_channel_bank_sets_the_flag_its_emissions_ask_for(B, K, oracle_mod):
    """A C-channel (fb = 8400) Aero-L bank of 5 channels linked to an 8400 bps bank: after every write and every tick the bank's dcd flag of
    each channel is the value of that channel's last DataCarrierDetect emission (oracle.AeroL(8400) fed the same soft bits), and a
    channel that never emitted keeps what the caller set.  The flag is read through the coarse-estimate test hook."""
    import ctypes as C

    nch, width, nticks = 5, 4096, 8
    streams = c_streams(nch)
    calls = c_oracle_dcd(oracle_mod, streams, width, nticks)
    seen = [[w[c] for w in calls] for c in range(nch)]
    assert any(1 in s and s[-1] == 0 for s in seen), "no channel's carrier detect rises and falls"
    assert seen[3][-1] is None, "the noise-only channel emitted"
    demod = B.DemodulatorBank(bank_settings("oqpsk", {"fb": 8400.0, "lockingbw": 8400.0}), nch, max_write_samples=4096)
    aerol = B.AeroLBank(nch, 8400, max_softbits_per_write=width)
    aerol.link_dcd(demod)
    demod.set_dcd(True, channel=3)
    caller = [0, 0, 0, 1, 0]

    def flags():
        out = []
        for c in range(nch):
            st = K.CoarseState()
            K.check(demod.L.jaero_debug_coarse_peek(demod.h, c, None, None, C.byref(st)))
            out.append(1 if st.flags & 8 else 0)  # JF_DCD
        return out

    k = 0
    for s0 in range(0, max(len(s) for s in streams), width):
        buf = np.zeros((nch, width), np.int16)
        cnt = np.zeros(nch, np.int32)
        for c in range(nch):
            seg = streams[c][s0:s0 + width]
            buf[c, :len(seg)] = seg
            cnt[c] = len(seg)
        aerol.write(buf, cnt)
        assert flags() == [caller[c] if w is None else w for c, w in enumerate(calls[k])], k
        k += 1
    for _ in range(nticks):
        aerol.tick_dcd()
        assert flags() == [caller[c] if w is None else w for c, w in enumerate(calls[k])], k
        k += 1
    aerol.close()
    demod.close()
